#!/usr/bin/env python
"""Golden sorts from the compiled reference library -- build container only.

    python tests/golden/make_sort_golden.py     # writes tests/golden/sort_golden.npz

Calls the reference's own ray_iasc / ray_idesc / ray_asc / ray_desc / ray_rank (core/order.c) on vectors and ray_xasc / ray_xdesc on tables through
ctypes on oracle/_ref/librayforce_ref.so.  The fixture is data only: every input in full (cells as int64 bit patterns, with type and attrs) and per
verb the answer's cells, type and attrs.  Vector cases: nulls, both NaN signs and a payload NaN, +-0.0, +-inf, subnormals, INT64_MIN+1, INT64_MAX,
all-equal, sorted data without the attribute, vectors carrying ATTR_ASC / ATTR_DESC (/ ATTR_DISTINCT), lengths 0, 1, 2, 63, 64, 65, 4097, 20011, keys
that differ in one byte only (each of the eight), heavy ties.  Table cases: by one, two and three columns, by an empty symbol vector and an empty [],
with a SYMBOL and a TIMESTAMP passenger column."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
T_I64, T_SYMBOL, T_TIMESTAMP, T_F64, T_TABLE = 5, 6, 9, 10, 98
NULL = -(2**63)
VERBS = ("iasc", "idesc", "asc", "desc", "rank")


class Obj(C.Structure):
    _fields_ = [("mmod", C.c_uint8), ("order", C.c_uint8), ("type", C.c_int8), ("attrs", C.c_uint8), ("rc", C.c_uint32), ("len", C.c_int64)]


def f64_bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def vector_cases():
    """(name, cells as int64 bits, type, attrs)"""
    rng = np.random.default_rng(20261016)
    nan_neg, nan_pay = np.int64(-0x0008000000000000), np.int64(0x7FF0000000000123)
    special_f = np.concatenate([f64_bits([np.nan, 0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, -1e-310, 1.5, -1.5, 1e308, -1e308]), [nan_neg, nan_pay]]).astype(np.int64)
    special_i = np.array([NULL, NULL + 1, 2**63 - 1, 0, -1, 1, 2**62, -(2**62), 255, 256, -256], np.int64)
    out = []
    for n in (0, 1, 2, 63, 64, 65):
        out.append((f"i64_n{n}", rng.integers(-50, 50, n), T_I64, 0))
        out.append((f"f64_n{n}", rng.choice(special_f, n), T_F64, 0))
    out.append(("i64_special", rng.choice(special_i, 4097), T_I64, 0))
    out.append(("i64_full", rng.integers(-(2**63), 2**63 - 1, 4097), T_I64, 0))
    out.append(("ts_nulls", np.where(rng.random(4097) < 0.1, NULL, rng.integers(0, 2**50, 4097)), T_TIMESTAMP, 0))
    f = f64_bits(rng.standard_normal(4097) * 1e3)
    out.append(("f64_special", np.where(rng.random(4097) < 0.3, rng.choice(special_f, 4097), f), T_F64, 0))
    out.append(("i64_ties", rng.integers(0, 7, 20011), T_I64, 0))
    out.append(("i64_narrow_nulls", np.where(rng.random(6001) < 0.01, NULL, rng.integers(0, 1000, 6001)), T_I64, 0))
    out.append(("i64_equal", np.full(300, 42), T_I64, 0))
    out.append(("f64_equal_nan", np.full(130, nan_pay), T_F64, 0))
    out.append(("i64_sorted_up", np.sort(rng.integers(-1000, 1000, 500)), T_I64, 0))
    out.append(("i64_sorted_down", np.sort(rng.integers(-1000, 1000, 500))[::-1], T_I64, 0))
    for d in range(8):
        out.append((f"i64_digit{d}", (rng.integers(0, 256, 700) << (8 * d)).astype(np.uint64).view(np.int64) + (0 if d == 7 else 0), T_I64, 0))
    up = np.sort(rng.integers(-100, 100, 200))
    for attrs in (2, 3, 4, 5, 1):
        # (the attribute is what the reference trusts: the data under ATTR_DESC here is ascending on purpose)
        out.append((f"i64_attrs{attrs}", up if attrs != 1 else rng.integers(-100, 100, 200), T_I64, attrs))
    out.append(("f64_attrs2", np.sort(rng.standard_normal(100)).view(np.int64), T_F64, 2))
    out.append(("i64_attrs2_empty", np.empty(0, np.int64), T_I64, 2))
    return [(n, np.ascontiguousarray(v, dtype=np.int64), t, a) for n, v, t, a in out]


def table_case():
    rng = np.random.default_rng(99)
    n = 1500
    names = ["apple", "pear", "fig", "kiwi"]
    a = np.where(rng.random(n) < 0.05, NULL, rng.integers(0, 5, n))
    b = f64_bits(rng.choice([np.nan, -0.0, 0.0, 1.5, -2.5, np.inf], n))
    c = rng.integers(-3, 3, n)
    ts = rng.integers(0, 2**40, n) // 2**30
    return {"a": (a, T_I64), "b": (b, T_F64), "c": (c, T_I64), "s": (rng.integers(0, len(names), n), T_SYMBOL), "ts": (ts, T_TIMESTAMP),
            "r": (np.arange(n), T_I64)}, names


TABLE_KEYS = (("a",), ("b",), ("ts",), ("a", "b"), ("b", "a"), ("c", "a", "b"), ())


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
    lib.symboli64.restype = C.c_void_p
    lib.symboli64.argtypes = [C.c_int64]
    for v in VERBS:
        getattr(lib, "ray_" + v).restype = C.c_void_p
        getattr(lib, "ray_" + v).argtypes = [C.c_void_p]
    for v in ("xasc", "xdesc"):
        getattr(lib, "ray_" + v).restype = C.c_void_p
        getattr(lib, "ray_" + v).argtypes = [C.c_void_p, C.c_void_p]

    def vec(bits, t, attrs=0):
        o = lib.vector(t, bits.size)
        if bits.size:
            C.memmove(o + 16, bits.ctypes.data, bits.nbytes)
        Obj.from_address(o).attrs = attrs
        return o

    def cells(o):
        h = Obj.from_address(o)
        assert h.type in (T_I64, T_F64, T_TIMESTAMP, T_SYMBOL), h.type
        return np.frombuffer((C.c_char * (h.len * 8)).from_address(o + 16), dtype=np.int64).copy(), int(h.type), int(h.attrs)

    def slot(o, i):
        return C.c_void_p.from_address(o + 16 + 8 * i).value

    arrays, meta = {}, []
    for ci, (name, bits, t, attrs) in enumerate(vector_cases()):
        arrays[f"v{ci}_in"] = bits
        row = [ci, t, attrs]
        for v in VERBS:
            got, rt, ra = cells(getattr(lib, "ray_" + v)(vec(bits, t, attrs)))
            arrays[f"v{ci}_{v}"] = got
            row += [rt, ra]
        meta.append(row)
        print(name, row)
    arrays["vector_cases"] = np.array(meta, np.int64)
    arrays["vector_names"] = np.array([c[0] for c in vector_cases()])

    cols, names = table_case()
    ids = np.array([lib.symbols_intern(s.encode(), len(s)) for s in names], np.int64)
    back = {int(i): k for k, i in enumerate(ids)}
    colnames = list(cols)
    colsyms = np.array([lib.symbols_intern(s.encode(), len(s)) for s in colnames], np.int64)

    def make_table():
        lst = lib.vector(0, len(cols))
        for i, (nm, (v, t)) in enumerate(cols.items()):
            data = ids[v] if t == T_SYMBOL else np.ascontiguousarray(v, dtype=np.int64)
            C.c_void_p.from_address(lst + 16 + 8 * i).value = vec(np.ascontiguousarray(data), t)
        return lib.table(vec(colsyms, T_SYMBOL), lst)

    for nm, (v, t) in cols.items():
        arrays[f"t_in_{nm}"] = np.ascontiguousarray(v, dtype=np.int64)
    arrays["t_types"] = np.array([t for _, t in cols.values()], np.int64)
    arrays["t_names"] = np.array(colnames)
    arrays["t_symbols"] = np.array(names)
    tk = []
    for ki, keys in enumerate(TABLE_KEYS):
        for form in (("atom", "vector") if len(keys) == 1 else ("vector", "empty_i64") if len(keys) == 0 else ("vector",)):
            for verb in ("xasc", "xdesc"):
                if form == "atom":
                    y = lib.symboli64(int(colsyms[colnames.index(keys[0])]))
                elif form == "empty_i64":
                    y = lib.vector(T_I64, 0)
                else:
                    y = vec(np.array([colsyms[colnames.index(k)] for k in keys], np.int64), T_SYMBOL)
                res = getattr(lib, "ray_" + verb)(make_table(), y)
                assert Obj.from_address(res).type == T_TABLE, Obj.from_address(res).type
                rc = slot(res, 1)
                tag = f"t{len(tk)}"
                for i, nm in enumerate(colnames):
                    got, rt, _ = cells(slot(rc, i))
                    assert rt == cols[nm][1]
                    arrays[f"{tag}_{nm}"] = np.array([back[int(x)] for x in got], np.int64) if rt == T_SYMBOL else got
                tk.append(f"{verb}|{form}|{','.join(keys)}")
                print(tk[-1])
    arrays["table_cases"] = np.array(tk)
    np.savez_compressed(os.path.join(HERE, "sort_golden.npz"), **arrays)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    main()
