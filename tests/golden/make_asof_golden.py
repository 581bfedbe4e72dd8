#!/usr/bin/env python
"""Golden asof joins, bin and binr from the compiled reference library -- build container only.

    python tests/golden/make_asof_golden.py     # writes tests/golden/asof_golden.npz

Calls the reference's own index_asof_join_obj (core/index.c:3194-3267), ray_asof_join (core/join.c:300-356) and ray_bin / ray_binr
(core/items.c:1552-1644) through ctypes on oracle/_ref/librayforce_ref.so.  The fixture is data only: every input in full (cells as int64, 4-byte
TIME cells sign-extended, with the reference's type codes) and the answers.
  i<k>_*   index cases: equality key columns and times of both sides, the join index the reference returned
  t<k>_*   table cases: both tables, and per result column its type, its cells and a null flag per row (a right-only column with an unmatched row
           comes back as a generic LIST holding Null objects: recorded as type 0, the atoms' cells, flag 1 where the object is Null)
  b<k>_*   bin / binr cases: x, y, both answers
Index cases: sorted and unsorted right times, left rows in random order, ties in time, times before a group's first, tuples absent from the right,
null keys and null times on both sides, one / two / three equality keys, groups of 1, 2, 3, 64, 65 rows and one group holding every row, row
counts 0, 1, 63, 64, 65, 4097, 20011 on either side."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
T_LIST, T_I64, T_SYMBOL, T_TIME, T_TIMESTAMP, T_F64, T_TABLE, T_NULL = 0, 5, 6, 8, 9, 10, 98, 126
NULL = -(2**63)
NULL32 = -(2**31)


class Obj(C.Structure):
    _fields_ = [("mmod", C.c_uint8), ("order", C.c_uint8), ("type", C.c_int8), ("attrs", C.c_uint8), ("rc", C.c_uint32), ("len", C.c_int64)]


def f64_bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def sides(rng, nl, nr, nkeys=1, krange=8, trange=100, sort_right=True, nulls=0.0, absent=0.0):
    """random equality keys and times for both sides; the right side ascending by time on request (ties stay)"""
    lk = [rng.integers(0, krange, nl) for _ in range(nkeys)]
    rk = [rng.integers(0, krange, nr) for _ in range(nkeys)]
    lt, rt = rng.integers(0, trange, nl), rng.integers(0, trange, nr)
    if sort_right:
        rt = np.sort(rt)
    if absent:
        lk[0] = np.where(rng.random(nl) < absent, krange + 5, lk[0])
    if nulls:
        for k in lk:
            k[rng.random(nl) < nulls] = NULL
        for k in rk:
            k[rng.random(nr) < nulls] = NULL
        lt[rng.random(nl) < nulls] = NULL
        rt[rng.random(nr) < nulls] = NULL
    return lk, lt, rk, rt


def index_cases():
    """(name, left keys, left times, right keys, right times)"""
    rng = np.random.default_rng(20261017)
    out = []
    # the issue's own example: rows 0 1 2 5 of s = 1 hold times 4 2 6 3; (s = 1, t = 5) answers row 1
    out.append(("issue_example", [np.array([1, 1, 2, 1, 9])], np.array([5, 1, 7, 100, 3]), [np.array([1, 1, 1, 2, 2, 1])], np.array([4, 2, 6, 1, 9, 3])))
    for n in (0, 1, 63, 64, 65, 4097):
        for m in (0, 1, 63, 64, 65, 4097):
            if (n in (63, 64) and m in (63, 64, 65)) or (n == 4097 and m not in (0, 1, 65)) or (m == 4097 and n not in (0, 1, 65)):
                continue  # (a sample of the pairs is enough; every size appears on both sides)
            out.append((f"sorted_{n}x{m}", *sides(rng, n, m, krange=5, trange=60)))
    out.append(("sorted_20011x1000", *sides(rng, 20011, 1000, krange=20, trange=1000)))
    out.append(("sorted_1000x20011", *sides(rng, 1000, 20011, krange=20, trange=1000)))
    out.append(("unsorted_4097x1500", *sides(rng, 4097, 1500, krange=7, trange=300, sort_right=False)))
    out.append(("unsorted_65x4097", *sides(rng, 65, 4097, krange=3, trange=500, sort_right=False)))
    out.append(("unsorted_two_keys", *sides(rng, 1500, 1500, nkeys=2, krange=6, trange=500, sort_right=False)))
    out.append(("sorted_two_keys", *sides(rng, 1500, 1500, nkeys=2, krange=6, trange=500, absent=0.1)))
    out.append(("sorted_three_keys", *sides(rng, 1500, 1500, nkeys=3, krange=4, trange=500, absent=0.1)))
    out.append(("nulls_sorted", *sides(rng, 2000, 2000, nkeys=2, krange=4, trange=200, nulls=0.08)))
    out.append(("nulls_unsorted", *sides(rng, 2000, 2000, krange=4, trange=200, nulls=0.08, sort_right=False)))
    out.append(("ties", *sides(rng, 1000, 1000, krange=3, trange=6)))
    out.append(("all_equal_times", [rng.integers(0, 3, 500)], np.full(500, 7), [rng.integers(0, 3, 700)], np.full(700, 7)))
    out.append(("before_first", [rng.integers(0, 4, 400)], rng.integers(0, 50, 400), [rng.integers(0, 4, 400)], np.sort(rng.integers(40, 90, 400))))
    # wide tuples: key ranges that do not multiply into 64 bits
    wide = [rng.integers(-(2**62), 2**62, 40) for _ in range(3)]
    pick_l, pick_r = rng.integers(0, 40, 1500), rng.integers(0, 40, 1500)
    out.append(("wide_three_keys", [w[pick_l] for w in wide], rng.integers(0, 300, 1500), [w[pick_r] for w in wide], np.sort(rng.integers(0, 300, 1500))))
    # groups of 1, 2, 3, 64, 65 rows, scattered over the table; then ONE group holding every row
    lens = [1, 2, 3, 64, 65, 1, 2, 3, 64, 65]
    rk = rng.permutation(np.repeat(np.arange(len(lens)), lens))
    for srt in (True, False):
        rt = rng.integers(0, 400, rk.size)
        out.append((f"group_lengths_{'sorted' if srt else 'unsorted'}", [rng.integers(0, len(lens) + 1, 1200)], rng.integers(-5, 410, 1200), [rk], np.sort(rt) if srt else rt))
        rt = rng.integers(0, 9000, 4097)
        out.append((f"one_group_{'sorted' if srt else 'unsorted'}", [np.full(900, 3)], rng.integers(-5, 9010, 900), [np.full(4097, 3)], np.sort(rt) if srt else rt))
    return [(n, [np.ascontiguousarray(k, dtype=np.int64) for k in lk], np.ascontiguousarray(lt, dtype=np.int64),
             [np.ascontiguousarray(k, dtype=np.int64) for k in rk], np.ascontiguousarray(rt, dtype=np.int64)) for n, lk, lt, rk, rt in out]


SYMS = ["apple", "pear", "fig", "kiwi", "plum"]


def table_cases():
    """(name, key names (the last one the asof column), left {name: (cells, type)}, right {...}); SYMBOL cells index SYMS"""
    rng = np.random.default_rng(77)
    out = []

    def base(nl, nr, ttype=T_I64, sort_right=True, all_match=False, nkeys=1):
        lk, lt, rk, rt = sides(rng, nl, nr, nkeys=nkeys, krange=len(SYMS), trange=1000, sort_right=sort_right)
        if all_match:  # every symbol's first right row at time -1, before every left time: every left row has a match
            for j in range(len(SYMS)):
                rk[0][j], rt[j] = j, -1
        if nkeys > 1:  # (the second key follows the first so that the tuples of both sides meet)
            lk[1], rk[1] = lk[0] % 3, rk[0] % 3
        left = {"s": (lk[0], T_SYMBOL), "t": (lt, ttype), "a": (rng.integers(-9, 9, nl), T_I64), "both": (rng.integers(0, 100, nl), T_I64),
                "bf": (f64_bits(rng.integers(-999, 999, nl) / 8.0), T_F64)}
        right = {"t": (rt, ttype), "s": (rk[0], T_SYMBOL), "both": (rng.integers(100, 200, nr), T_I64), "b": (rng.integers(1000, 2000, nr), T_I64),
                 "bf": (f64_bits(rng.integers(-999, 999, nr) / 8.0), T_F64), "f": (f64_bits(rng.integers(-999, 999, nr) / 8.0), T_F64)}
        keys = ["s", "t"]
        if nkeys > 1:
            left["k2"], right["k2"] = (lk[1], T_I64), (rk[1], T_I64)
            keys = ["s", "k2", "t"]
        return keys, left, right

    out.append(("mixed_i64", *base(500, 400)))
    out.append(("mixed_unsorted", *base(500, 400, sort_right=False)))
    out.append(("all_matched", *base(600, 300, all_match=True)))
    out.append(("all_matched_two_keys", *base(600, 300, all_match=True, nkeys=2)))
    out.append(("timestamp", *base(300, 300, ttype=T_TIMESTAMP)))
    out.append(("time_4_bytes", *base(300, 300, ttype=T_TIME)))
    out.append(("time_4_bytes_all_matched", *base(300, 300, ttype=T_TIME, all_match=True)))
    k, l, r = base(300, 300, ttype=T_TIME, sort_right=False)
    l["t"][0][::17] = NULL32
    r["t"][0][::13] = NULL32
    out.append(("time_4_bytes_nulls_unsorted", k, l, r))
    out.append(("empty_right", *base(50, 0)))
    out.append(("empty_left", *base(0, 50)))
    out.append(("two_keys", *base(400, 400, nkeys=2)))
    return out


def bin_cases():
    rng = np.random.default_rng(5)
    out = [("issue_example", np.array([5, 1, 7, 3, 9, 2]), np.array([4, 0, 9, 6]), T_I64)]
    x = np.sort(rng.integers(-1000, 1000, 4097))
    out.append(("sorted", x, rng.integers(-1100, 1100, 1000), T_I64))
    out.append(("sorted_duplicates", np.sort(rng.integers(0, 20, 1000)), rng.integers(-2, 23, 500), T_I64))
    out.append(("unsorted", rng.integers(-1000, 1000, 4097), rng.integers(-1100, 1100, 1000), T_I64))
    out.append(("all_equal", np.full(65, 4), np.array([3, 4, 5, NULL, 2**63 - 1]), T_I64))
    out.append(("empty_x", np.empty(0, np.int64), np.array([1, 2, NULL]), T_I64))
    out.append(("empty_y", np.arange(10), np.empty(0, np.int64), T_I64))
    out.append(("below_and_above", np.arange(100, 164), np.array([-5, 99, 164, 10**12, NULL]), T_I64))
    xn = np.sort(rng.integers(0, 500, 700))
    xn[:9] = NULL
    out.append(("nulls_sorted", xn, np.where(rng.random(400) < 0.1, NULL, rng.integers(-5, 505, 400)), T_I64))
    xu = rng.integers(0, 500, 700)
    xu[rng.random(700) < 0.05] = NULL
    out.append(("nulls_unsorted", xu, np.where(rng.random(400) < 0.1, NULL, rng.integers(-5, 505, 400)), T_I64))
    out.append(("timestamp", np.sort(rng.integers(0, 2**50, 500)), rng.integers(0, 2**50, 300), T_TIMESTAMP))
    for n in (1, 2, 3, 63, 64, 65):
        out.append((f"len_{n}", np.sort(rng.integers(0, 50, n)), rng.integers(-2, 53, 200), T_I64))
    return [(n, np.ascontiguousarray(x, dtype=np.int64), np.ascontiguousarray(y, dtype=np.int64), t) for n, x, y, t in out]


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "librayforce_ref.so"))
    lib.ray_init.restype = C.c_int32
    assert lib.ray_init() == 0
    lib.vector.restype = C.c_void_p
    lib.vector.argtypes = [C.c_int8, C.c_int64]
    lib.table.restype = C.c_void_p
    lib.table.argtypes = [C.c_void_p, C.c_void_p]
    lib.symbols_intern.restype = C.c_int64
    lib.symbols_intern.argtypes = [C.c_char_p, C.c_int64]
    lib.index_asof_join_obj.restype = C.c_void_p
    lib.index_asof_join_obj.argtypes = [C.c_void_p] * 4
    lib.ray_asof_join.restype = C.c_void_p
    lib.ray_asof_join.argtypes = [C.POINTER(C.c_void_p), C.c_int64]
    for v in ("ray_bin", "ray_binr"):
        getattr(lib, v).restype = C.c_void_p
        getattr(lib, v).argtypes = [C.c_void_p, C.c_void_p]

    def vec(cells, t):
        o = lib.vector(t, cells.size)
        data = np.ascontiguousarray(cells.astype(np.int32) if t == T_TIME else cells)
        if cells.size:
            C.memmove(o + 16, data.ctypes.data, data.nbytes)
        return o

    def lst(objs):
        o = lib.vector(T_LIST, len(objs))
        for i, p in enumerate(objs):
            C.c_void_p.from_address(o + 16 + 8 * i).value = p
        return o

    def slot(o, i):
        return C.c_void_p.from_address(o + 16 + 8 * i).value

    def cells(o):
        """(cells as int64, null flags, type): a typed vector, or a LIST of atoms and Null objects"""
        h = Obj.from_address(o)
        if h.type == T_LIST:
            vals, nul = np.zeros(h.len, np.int64), np.zeros(h.len, np.int8)
            for i in range(h.len):
                e = slot(o, i)
                et = Obj.from_address(e).type
                if et == T_NULL:
                    nul[i] = 1
                else:
                    assert et in (-T_I64, -T_F64, -T_SYMBOL, -T_TIMESTAMP), et
                    vals[i] = C.c_int64.from_address(e + 8).value
            return vals, nul, T_LIST
        if h.type == T_TIME:
            return np.frombuffer((C.c_char * (h.len * 4)).from_address(o + 16), dtype=np.int32).astype(np.int64), np.zeros(h.len, np.int8), T_TIME
        assert h.type in (T_I64, T_F64, T_TIMESTAMP, T_SYMBOL), h.type
        return np.frombuffer((C.c_char * (h.len * 8)).from_address(o + 16), dtype=np.int64).copy(), np.zeros(h.len, np.int8), int(h.type)

    arrays = {}
    names = []
    for ci, (name, lk, lt, rk, rt) in enumerate(index_cases()):
        res = lib.index_asof_join_obj(lst([vec(k, T_I64) for k in lk]), vec(lt, T_I64), lst([vec(k, T_I64) for k in rk]), vec(rt, T_I64))
        ids, _, t = cells(res)
        assert t == T_I64 and ids.size == lt.size, (name, t)
        for j, (a, b) in enumerate(zip(lk, rk)):
            arrays[f"i{ci}_lk{j}"], arrays[f"i{ci}_rk{j}"] = a, b
        arrays[f"i{ci}_lt"], arrays[f"i{ci}_rt"], arrays[f"i{ci}_ids"] = lt, rt, ids
        names.append(f"{name}|{len(lk)}")
        print(name, lt.size, rt.size, "matched", int((ids != NULL).sum()))
    arrays["index_cases"] = np.array(names)

    symids = np.array([lib.symbols_intern(s.encode(), len(s)) for s in SYMS], np.int64)
    back = {int(s): i for i, s in enumerate(symids)}

    def sym(s):
        return lib.symbols_intern(s.encode(), len(s))

    def make_table(cols):
        return lib.table(vec(np.array([sym(n) for n in cols], np.int64), T_SYMBOL), lst([vec(symids[v] if t == T_SYMBOL else v, t) for v, t in cols.values()]))

    names = []
    for ci, (name, keys, left, right) in enumerate(table_cases()):
        kv = vec(np.array([sym(k) for k in keys], np.int64), T_SYMBOL)
        Obj.from_address(kv).rc = 2  # (ray_asof_join shortens a key vector it holds the only reference to IN PLACE and then reads it again)
        args = (C.c_void_p * 3)(kv, make_table(left), make_table(right))
        res = lib.ray_asof_join(args, 3)
        assert Obj.from_address(res).type == T_TABLE, (name, Obj.from_address(res).type)
        rnames, _, _ = cells(slot(res, 0))
        rcols = slot(res, 1)
        want_names = keys + [c for c in left if c not in keys] + [c for c in right if c not in keys and c not in left]
        assert [int(s) for s in rnames] == [sym(n) for n in want_names], name
        for side, cols in (("l", left), ("r", right)):
            for n, (v, t) in cols.items():
                arrays[f"t{ci}_{side}_{n}"] = np.ascontiguousarray(v, dtype=np.int64)
            arrays[f"t{ci}_{side}_names"] = np.array(list(cols))
            arrays[f"t{ci}_{side}_types"] = np.array([t for _, t in cols.values()], np.int64)
        types = []
        for i, n in enumerate(want_names):
            v, nul, t = cells(slot(rcols, i))
            if t == T_SYMBOL or (t == T_LIST and (left.get(n) or right.get(n))[1] == T_SYMBOL):
                v = np.array([back[int(x)] if not f else 0 for x, f in zip(v, nul)], np.int64)
            arrays[f"t{ci}_out_{n}"], arrays[f"t{ci}_null_{n}"] = v, nul
            types.append(t)
        arrays[f"t{ci}_out_names"] = np.array(want_names)
        arrays[f"t{ci}_out_types"] = np.array(types, np.int64)
        names.append(f"{name}|{','.join(keys)}")
        print(name, dict(zip(want_names, types)))
    arrays["table_cases"] = np.array(names)
    arrays["symbols"] = np.array(SYMS)

    names = []
    for ci, (name, x, y, t) in enumerate(bin_cases()):
        arrays[f"b{ci}_x"], arrays[f"b{ci}_y"] = x, y
        for verb in ("bin", "binr"):
            got, _, rt = cells(getattr(lib, "ray_" + verb)(vec(x, t), vec(y, t)))
            assert rt == T_I64 and got.size == y.size, (name, verb, rt)
            arrays[f"b{ci}_{verb}"] = got
        names.append(f"{name}|{t}")
        print(name, arrays[f"b{ci}_bin"][:6], arrays[f"b{ci}_binr"][:6])
    arrays["bin_cases"] = np.array(names)
    path = os.path.join(HERE, "asof_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
