#!/usr/bin/env python
"""Golden set verbs from the compiled reference -- build container only.

    python tests/golden/make_set_golden.py     # writes tests/golden/set_golden.npz

Every case is a Rayfall script run by the reference BINARY (oracle/ref.py Session; not ctypes: index_scope_i64 called bare dereferences a null
pool): the operands go in as column files carrying their type code (5 I64, 6 SYMBOL, 9 TIMESTAMP), one of
(distinct x) (in x y) (find x y) (sect x y) (except x y) (union x y) is evaluated, and the answer comes back as a column file whose header also
gives the answer's type code and attributes.  SYMBOL cells are raw ids the reference never resolves; a SYMBOL answer cannot be written to a file
(that would resolve them), so it is read back as (find source answer) -- the rows of the source holding the answer's cells, in the answer's order --
and its type as (== (type answer) (type x)); its attributes are not observable that way (recorded as -1).
Each case runs with one thread and with eight; only cases where both runs agree bit for bit are kept (a dropped case is printed).
The cases named host_* are the shapes for which the reference indexes outside its own tables (a hash route over a negative key, find's over a
null, a range beyond 64 bits): inputs only, never run, never answered by the device.  WHICH cases are host_ cases is decided here, from the
reference's source, not by any test at run time.

The fixture is data only:
  cases      "name|verb|type code|atom (1: y is one cell)|route|answer type code|answer attrs|threads"    route: tests/set_ref.py's names
  c<k>_x c<k>_y c<k>_out    the cells as eight byte planes (uint8, shape (8, cells)); in's answer is 0 / 1 cells"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
import set_ref  # noqa: E402

NULL = -(2**63)
I64, SYM, TS = 5, 6, 9
LENS = (0, 1, 63, 64, 65, 4097, 20011)
PAIRS = ((0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (4097, 20011), (20011, 4097))


def spread(rng, n, pool=None, hi=10**12):
    """n cells drawn from `pool` distinct keys spread over [0, hi): heavy duplicates when pool << n"""
    if n == 0:
        return np.empty(0, np.int64)
    keys = rng.integers(0, hi, max(1, pool or n))
    keys[0], keys[-1] = 0, hi - 1  # (the spread itself is certain: the hash route whatever else is drawn)
    return keys[rng.integers(0, keys.size, n)] if n > 2 else keys[:n]


def tiled(a):
    """a long operand as a pattern of 800 random cells repeated: the answers repeat with it, which keeps the fixture small on disk"""
    return np.resize(a[:800], a.size) if a.size > 2000 else a


def cases():
    rng = np.random.default_rng(20261019)
    out = []

    def add(name, verb, x, y=None, tp=I64, atom=False, whole=False):
        x, y = np.ascontiguousarray(x, dtype=np.int64), None if y is None else np.ascontiguousarray(y, dtype=np.int64)
        if not whole:  # (the first two cells stay what they are: the cells that pin a case's scope lead the operand)
            x = np.concatenate([x[:2], tiled(x[2:])])
            y = None if y is None else np.concatenate([y[:2], tiled(y[2:])])
        out.append((name, verb, tp, atom, x, y))

    # ---- distinct
    for n in LENS:
        add(f"distinct_dense_len{n}", "distinct", tiled(rng.integers(-50, 300, n)))
        if n >= 63:
            add(f"distinct_hash_len{n}", "distinct", np.concatenate([[0, 10**12], tiled(spread(rng, n - 2, max(1, n // 4)))]))
    add("distinct_dense_negative", "distinct", rng.integers(-1000, 1000, 4097))
    add("distinct_dense_range_2p20", "distinct", np.concatenate([[0, 2**20 - 1], rng.integers(0, 2**20, 98)]))
    add("distinct_hash_range_2p20_plus1", "distinct", np.concatenate([[2**20, 0], rng.integers(0, 2**20, 98)]))
    n = 2**20 + 5  # range == len beyond 2^20: dense because of the rows, and one more: hash
    perm = n - 1 - np.arange(n, dtype=np.int64)  # (descending: rows in an order that is not the answer's, and byte planes that compress)
    add("distinct_dense_range_eq_len", "distinct", perm, whole=True)
    add("distinct_hash_range_len_plus1", "distinct", np.where(perm == n - 1, n, perm), whole=True)
    add("distinct_all_equal", "distinct", np.full(100, 7))
    add("distinct_one_null_only", "distinct", np.full(3, NULL))
    add("distinct_dense_null_low", "distinct", np.array([NULL + 3, NULL, NULL + 1, NULL + 3, NULL]))
    n = 4097
    P = set_ref.table_cells(n)
    add("distinct_hash_clustered", "distinct", 11 + P * rng.integers(0, 10**6, n), whole=True)  # every key's home is cell 11
    homes = np.array([P - 1, P - 2, P - 3, 0, 1])
    add("distinct_hash_wrap", "distinct", homes[rng.integers(0, 5, n)] + P * 1000 * rng.integers(0, 40, n), whole=True)  # 200 keys homed around the table's end
    add("distinct_ts_dense", "distinct", rng.integers(0, 500, 4097), tp=TS)
    add("distinct_ts_hash", "distinct", spread(rng, 4097, 900), tp=TS)
    add("distinct_sym_dense", "distinct", rng.integers(100, 600, 4097), tp=SYM)
    add("distinct_sym_hash", "distinct", spread(rng, 4097, 900), tp=SYM)
    add("host_distinct_null_overflow", "distinct", np.array([NULL, 5, 7]))
    add("host_distinct_hash_negative", "distinct", np.array([-5, 10**12, 3]))
    add("host_distinct_null_hash_negative", "distinct", np.array([NULL, -5, -(10**12)]))

    # ---- the binary verbs
    for verb in ("in", "find", "sect", "except", "union"):
        for nx, ny in PAIRS:
            add(f"{verb}_dense_{nx}x{ny}", verb, tiled(rng.integers(-40, 400, nx)), tiled(rng.integers(-100, 300, ny)))
            if nx >= 63:
                pool = spread(rng, 3000, 3000)
                add(f"{verb}_hash_{nx}x{ny}", verb, np.concatenate([[0, 10**12], tiled(pool[rng.integers(0, 2000, nx - 2)])]),
                    np.concatenate([[0, 10**12], tiled(pool[rng.integers(1000, 3000, ny - 2)])]))
        add(f"{verb}_all_equal", verb, np.full(70, 9), np.full(33, 9))
        add(f"{verb}_disjoint", verb, rng.integers(0, 100, 500), rng.integers(1000, 1100, 300))
        if verb != "union":
            add(f"{verb}_hash_small_table", verb, spread(rng, 5, 5), np.concatenate([[0, 10**12 - 1], spread(rng, 4095, 4000)]))  # in: ht_oa_create(5) rehashes
    for verb in ("in", "find", "union"):
        add(f"{verb}_ts_dense", verb, rng.integers(0, 500, 4097), rng.integers(250, 750, 300), tp=TS)
        add(f"{verb}_ts_hash", verb, spread(rng, 4097, 900), spread(rng, 500, 400), tp=TS)
    for verb in ("in", "find", "sect", "except", "union"):
        add(f"{verb}_sym_dense", verb, rng.integers(100, 600, 4097), rng.integers(350, 850, 300), tp=SYM)
        pool = spread(rng, 1500, 1500)
        add(f"{verb}_sym_hash", verb, np.concatenate([[0, 10**12 - 1], pool[rng.integers(0, 1000, 4095)]]), np.concatenate([[0, 10**12 - 1], pool[rng.integers(500, 1500, 500)]]), tp=SYM)
    # nulls: dense with a null on one side; both sides -> the intersection starts at the null and spans to a non-negative key: the hash route
    small = rng.integers(0, 200, 300)
    add("in_null_x_dense", "in", np.concatenate([[NULL], small]), rng.integers(0, 200, 100))
    add("in_null_y_dense", "in", small, np.concatenate([rng.integers(0, 200, 100), [NULL]]))
    add("in_null_both_hash", "in", np.concatenate([[NULL, 3], small, [NULL]]), np.concatenate([rng.integers(0, 200, 100), [NULL]]))
    add("in_null_x_hash", "in", np.concatenate([[NULL], spread(rng, 300, 100)]), spread(rng, 300, 100))
    add("in_null_y_hash", "in", spread(rng, 300, 100), np.concatenate([[NULL], spread(rng, 300, 100)]))
    add("in_null_both_low_dense", "in", np.array([NULL, NULL + 2, NULL + 5]), np.array([NULL + 5, NULL, NULL + 1]))
    add("find_null_x_dense", "find", np.concatenate([[NULL], small]), rng.integers(0, 200, 100))
    add("find_null_y_dense", "find", small, np.concatenate([rng.integers(0, 200, 100), [NULL]]))
    add("find_empty_x", "find", np.empty(0, np.int64), rng.integers(0, 200, 100))
    add("sect_null_both_hash", "sect", np.concatenate([[NULL, 3], small, [NULL]]), np.concatenate([rng.integers(0, 200, 100), [NULL]]))
    add("except_null_both_hash", "except", np.concatenate([[NULL, 3], small, [NULL]]), np.concatenate([rng.integers(0, 200, 100), [NULL]]))
    # except with an atom
    add("except_atom_present", "except", rng.integers(0, 10, 4097), np.array([3]), atom=True)
    add("except_atom_absent", "except", rng.integers(0, 10, 65), np.array([77]), atom=True)
    add("except_atom_null", "except", np.concatenate([[NULL], rng.integers(0, 10, 65), [NULL]]), np.array([NULL]), atom=True)
    add("except_atom_sym", "except", rng.integers(100, 110, 4097), np.array([103]), tp=SYM, atom=True)
    # union whose halves take another route alone than together
    add("union_dense_halves_hash_together", "union", rng.integers(0, 100, 500), 10**12 + rng.integers(0, 100, 500))
    add("union_dense_half_joins_sparse_half", "union", rng.integers(0, 2**20, 4097), np.array([0, 2**21]))  # (x alone dense, y alone hash, together hash)
    # the undefined shapes: the host's, never the device's
    add("host_in_hash_negative_x", "in", np.array([-7, 10**12, 5]), np.array([5, 0, 10**12]))
    add("host_in_hash_negative_y", "in", np.array([0, 10**12, 5]), np.array([5, -7, 10**12]))
    add("host_find_hash_negative", "find", np.array([-7, 10**12, 5]), np.array([5, -7, 10**12]))
    add("host_find_hash_null_x", "find", np.array([NULL, 10**12, 5]), np.array([5, 0, 10**12]))
    add("host_find_hash_null_y", "find", np.array([0, 10**12, 5]), np.array([5, NULL, 10**12]))
    add("host_find_range_overflow", "find", np.array([NULL, 2**63 - 1, 5]), np.array([2**63 - 1, NULL]))
    add("host_sect_hash_negative", "sect", np.array([-7, 10**12, 5]), np.array([5, 0, 10**12]))
    add("host_except_hash_negative", "except", np.array([-7, 10**12, 5]), np.array([5, 0, 10**12]))
    add("host_union_hash_negative", "union", np.array([-5, 3]), np.array([10**12]))
    add("host_union_null_overflow", "union", np.array([NULL, 3]), np.array([5]))

    # ---- the binary verbs at their own route boundary (a generator of their own: the cases above stay what they were)
    rng = np.random.default_rng(20261020)
    M = 2**20
    for verb in ("in", "find", "sect", "except"):
        # the INTERSECTION of the two scopes spans 2^20 cells (dense) and one more (hash); x's scope is the narrower one.  find looks y up in x.
        def both(name, lo, hi, null_x=False):
            a = np.concatenate([[lo, hi], rng.integers(lo, hi + 1, 120), [NULL] if null_x else []]).astype(np.int64)  # the operand whose scope is [lo, hi]
            # (a null makes a's own minimum the null: there the intersection's lower end is b's)
            b = np.concatenate([[lo if null_x else lo - 50, hi + M], rng.integers(lo, hi + 1, 90), a[5:40]]).astype(np.int64)
            add(name, verb, *((b, a) if verb == "find" and not null_x else (a, b)))
        both(f"{verb}_dense_isect_2p20", 0, M - 1)
        both(f"{verb}_hash_isect_2p20_plus1", 50, M + 50)
        both(f"{verb}_dense_isect_2p20_negative", -7, M - 8)
        both(f"host_{verb}_isect_2p20_plus1_negative", -7, M - 7)
        if verb != "find":  # a null in x lies below y's scope: outside the intersection, the route is y's and x's non-null cells'
            both(f"{verb}_dense_isect_2p20_null_x", 50, M + 49, null_x=True)
            both(f"{verb}_hash_isect_2p20_plus1_null_x", 50, M + 50, null_x=True)
    # union: distinct over both spans -- the same boundaries with the scope's ends in DIFFERENT operands, rows of y counted from len x
    add("union_dense_range_2p20", "union", np.concatenate([[0], rng.integers(0, M, 60)]), np.concatenate([[M - 1], rng.integers(0, M, 40)]))
    add("union_hash_range_2p20_plus1", "union", np.concatenate([[0], rng.integers(0, M, 60)]), np.concatenate([[M], rng.integers(0, M, 40)]))
    n = M + 6
    perm = n - 1 - np.arange(n, dtype=np.int64)
    add("union_dense_range_eq_len", "union", perm[: n // 2], perm[n // 2 :], whole=True)
    add("union_hash_range_len_plus1", "union", np.where(perm == n - 1, n, perm)[: n // 2], perm[n // 2 :], whole=True)
    nx, ny = 2500, 1597
    P = set_ref.table_cells(nx + ny)
    mult = rng.integers(0, 3000, nx + ny)  # (3000 multipliers over 4097 cells: keys met again inside x, inside y and across the two)
    add("union_hash_clustered", "union", 11 + P * mult[:nx], 11 + P * mult[nx:], whole=True)  # every key's home is cell 11
    homes = np.array([P - 1, P - 2, P - 3, 0, 1])
    keys = homes[rng.integers(0, 5, nx + ny)] + P * 1000 * rng.integers(0, 40, nx + ny)  # 200 keys homed around the table's end
    add("union_hash_wrap", "union", keys[:nx], keys[nx:], whole=True)
    return out


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    if tp == 1:
        return np.frombuffer(body, np.int8, n).astype(np.int64), tp, attrs
    assert tp in (I64, TS), tp
    return np.frombuffer(body, np.int64, n).copy(), tp, attrs


def run_case(verb, tp, atom, x, y, threads):
    with ref.Session() as s:
        s.put("x", x, tp=tp)
        if y is not None:
            s.put("y", y, tp=tp)
        yy = "(first y)" if atom else "y"
        e = "(distinct x)" if verb == "distinct" else f"({verb} x {yy})"
        via_find = tp == SYM and verb in ("distinct", "sect", "except", "union")
        if via_find:
            s.eval("(set src (concat x y))" if verb == "union" else "(set src x)")
            s.out("r", f"(find src {e})")
            s.out("ty", f"(as 'I64 (enlist (== (type {e}) (type x))))")
        else:
            s.out("r", e)
        s.run(threads=threads)
        r, rt, attrs = read_file(os.path.join(s.dir, "out_r"))
        if via_find:
            src = np.concatenate([x, y]) if verb == "union" else x
            assert rt == I64 and (r.size == 0 or (r.min() >= 0 and r.max() < src.size)), (verb, r)
            ok, _, _ = read_file(os.path.join(s.dir, "out_ty"))
            assert ok.tolist() == [1]
            return src[r], tp, -1
        return r, rt, attrs


def planes(a):
    return np.ascontiguousarray(np.ascontiguousarray(a, dtype=np.int64).reshape(-1).view(np.uint8).reshape(-1, 8).T)


def main():
    assert ref.build() or ref.available()
    arrays, names, dropped = {}, [], []
    for name, verb, tp, atom, x, y in cases():
        k = len(names)
        if name.startswith("host_"):
            want, reason = set_ref.VERBS[verb](x, y) if y is not None else set_ref.distinct(x)
            assert want == set_ref.UNDEFINED, name  # (the maker's own reading of the source and the restatement's must be the same list)
            meta = f"{name}|{verb}|{tp}|{int(atom)}|undefined|0|0|"
        else:
            try:
                one = run_case(verb, tp, atom, x, y, 1)
                eight = run_case(verb, tp, atom, x, y, 8)
            except Exception as e:  # the reference did not answer at all
                dropped.append((name, "no answer: " + str(e)[:200]))
                continue
            if not (np.array_equal(one[0], eight[0]) and one[1:] == eight[1:]):
                dropped.append((name, "1 and 8 threads differ"))
                continue
            route = (set_ref.VERBS[verb](x, int(y[0]) if atom else y) if y is not None else set_ref.distinct(x))[1]
            arrays[f"c{k}_out"] = planes(one[0])
            meta = f"{name}|{verb}|{tp}|{int(atom)}|{route}|{one[1]}|{one[2]}|1,8"
            print(name, x.size, 0 if y is None else y.size, "->", one[0].size, route, "type", one[1], "attrs", one[2])
        arrays[f"c{k}_x"] = planes(x)
        if y is not None:
            arrays[f"c{k}_y"] = planes(y)
        names.append(meta)
    arrays["cases"] = np.array(names)
    path = os.path.join(HERE, "set_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(names), "cases,", os.path.getsize(path), "bytes; dropped:", dropped)


if __name__ == "__main__":
    main()
