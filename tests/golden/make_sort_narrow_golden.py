#!/usr/bin/env python
"""Golden sorts of 1-, 2- and 4-byte keys from the compiled reference library -- build container only.

    python tests/golden/make_sort_narrow_golden.py     # writes tests/golden/sort_narrow_golden.npz

Calls the reference's own ray_iasc / ray_idesc / ray_asc / ray_desc / ray_rank (core/order.c, core/sort.c) on B8, U8, I16, I32, DATE and TIME
vectors through ctypes on oracle/_ref/librayforce_ref.so.  The fixture is data only: every input in its own dtype (uint8 / int16 / int32) with type
and attrs, and per verb the answer's cells (permutations as int32, sorted cells in the input's dtype), type and attrs -- or, where the reference
answers an error object (its reverse has no I16 arm), that it did.  Cases: lengths 0, 1, 2, 63, 64, 65, 4097 (20011 for the I32 and I16 heavy
ties), full-range values with INT32_MIN (the null), INT32_MAX, -1, 0, INT16_MIN and 255, a null share of about 10 % in a DATE and a TIME case,
keys that differ in exactly one byte (each of the four for I32, each of the two for I16), all-equal cells, sorted data without the attribute,
vectors carrying attrs 2, 3, 4, 5 and 1 (the data under ATTR_DESC ascending on purpose), B8 cells other than 0 / 1."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
T_B8, T_U8, T_I16, T_I32, T_I64, T_DATE, T_TIME, T_ERR = 1, 2, 3, 4, 5, 7, 8, 127
DTYPE = {T_B8: np.uint8, T_U8: np.uint8, T_I16: np.int16, T_I32: np.int32, T_DATE: np.int32, T_TIME: np.int32}
I32_MIN, I32_MAX, I16_MIN, I16_MAX = -(2**31), 2**31 - 1, -(2**15), 2**15 - 1
VERBS = ("iasc", "idesc", "asc", "desc", "rank")


class Obj(C.Structure):
    _fields_ = [("mmod", C.c_uint8), ("order", C.c_uint8), ("type", C.c_int8), ("attrs", C.c_uint8), ("rc", C.c_uint32), ("len", C.c_int64)]


def vector_cases():
    """(name, cells, type, attrs)"""
    rng = np.random.default_rng(20261020)
    special32 = np.array([I32_MIN, I32_MIN + 1, I32_MAX, 0, -1, 1, 255, 256, -256, 65536, -65536], np.int64)
    special16 = np.array([I16_MIN, I16_MIN + 1, I16_MAX, 0, -1, 1, 255, 256, -256], np.int64)
    out = []
    for n in (0, 1, 2, 63, 64, 65):
        out.append((f"b8_n{n}", rng.integers(0, 2, n), T_B8, 0))
        out.append((f"u8_n{n}", rng.integers(0, 256, n), T_U8, 0))
        out.append((f"i16_n{n}", rng.integers(-300, 300, n), T_I16, 0))
        out.append((f"i32_n{n}", rng.integers(-50, 50, n), T_I32, 0))
        out.append((f"date_n{n}", rng.integers(-100_000, 100_000, n), T_DATE, 0))
        out.append((f"time_n{n}", rng.integers(0, 86_400_000, n), T_TIME, 0))
    n = 4097
    out.append(("i32_full", rng.integers(I32_MIN, I32_MAX + 1, n), T_I32, 0))
    out.append(("i32_special", rng.choice(special32, n), T_I32, 0))
    out.append(("i16_full", rng.integers(I16_MIN, I16_MAX + 1, n), T_I16, 0))
    out.append(("i16_special", rng.choice(special16, n), T_I16, 0))
    out.append(("u8_full", rng.integers(0, 256, n), T_U8, 0))
    out.append(("u8_special", rng.choice(np.array([0, 1, 127, 128, 255]), n), T_U8, 0))
    out.append(("b8_bytes", rng.choice(np.array([0, 1, 2, 7, 128, 255]), n), T_B8, 0))  # (cells other than 0 / 1: ordered as bytes)
    out.append(("b8_flags", rng.integers(0, 2, n), T_B8, 0))
    out.append(("date_nulls", np.where(rng.random(n) < 0.1, I32_MIN, rng.integers(-200_000, 200_000, n)), T_DATE, 0))
    out.append(("time_nulls", np.where(rng.random(n) < 0.1, I32_MIN, rng.integers(0, 86_400_000, n)), T_TIME, 0))
    out.append(("i32_ties", rng.integers(0, 7, 20011), T_I32, 0))
    out.append(("i16_ties", rng.integers(-3, 4, 20011), T_I16, 0))
    for d in range(4):
        out.append((f"i32_digit{d}", (rng.integers(0, 256, 700) << (8 * d)).astype(np.uint32).view(np.int32), T_I32, 0))
    for d in range(2):
        out.append((f"i16_digit{d}", (rng.integers(0, 256, 700) << (8 * d)).astype(np.uint16).view(np.int16), T_I16, 0))
    out.append(("i32_equal", np.full(300, 42), T_I32, 0))
    out.append(("date_equal_null", np.full(130, I32_MIN), T_DATE, 0))
    out.append(("i16_equal", np.full(300, -7), T_I16, 0))
    out.append(("u8_equal", np.full(300, 200), T_U8, 0))
    out.append(("b8_equal", np.full(300, 1), T_B8, 0))
    out.append(("i32_sorted_up", np.sort(rng.integers(-1000, 1000, 500)), T_I32, 0))
    out.append(("time_sorted_down", np.sort(rng.integers(0, 86_400_000, 500))[::-1], T_TIME, 0))
    out.append(("i16_sorted_up", np.sort(rng.integers(-1000, 1000, 500)), T_I16, 0))
    out.append(("u8_sorted_down", np.sort(rng.integers(0, 256, 500))[::-1], T_U8, 0))
    for t, tag, lo, hi in ((T_I32, "i32", -100, 100), (T_DATE, "date", -100, 100), (T_I16, "i16", -100, 100), (T_U8, "u8", 0, 200), (T_B8, "b8", 0, 2)):
        up = np.sort(rng.integers(lo, hi, 200))
        for attrs in (2, 3, 4, 5, 1):
            # (the attribute is what the reference trusts: the data under ATTR_DESC here is ascending on purpose)
            out.append((f"{tag}_attrs{attrs}", up if attrs != 1 else rng.integers(lo, hi, 200), t, attrs))
    out.append(("time_attrs2_empty", np.empty(0, np.int64), T_TIME, 2))
    out.append(("i16_attrs4_empty", np.empty(0, np.int64), T_I16, 4))
    return [(n, np.ascontiguousarray(np.asarray(v, np.int64).astype(DTYPE[t])), t, a) for n, v, t, a in out]


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "librayforce_ref.so"))
    lib.ray_init.restype = C.c_int32
    assert lib.ray_init() == 0
    lib.vector.restype = C.c_void_p
    lib.vector.argtypes = [C.c_int8, C.c_int64]
    for v in VERBS:
        getattr(lib, "ray_" + v).restype = C.c_void_p
        getattr(lib, "ray_" + v).argtypes = [C.c_void_p]

    def vec(cells, t, attrs=0):
        o = lib.vector(t, cells.size)
        if cells.size:
            C.memmove(o + 16, cells.ctypes.data, cells.nbytes)
        Obj.from_address(o).attrs = attrs
        return o

    def answer(o):
        """(cells or None for an error, type, attrs)"""
        h = Obj.from_address(o)
        if h.type == T_ERR:
            return None, T_ERR, 0
        assert h.type == T_I64 or h.type in DTYPE, h.type
        dt = np.dtype(np.int64 if h.type == T_I64 else DTYPE[h.type])
        return np.frombuffer((C.c_char * (h.len * dt.itemsize)).from_address(o + 16), dtype=dt).copy(), int(h.type), int(h.attrs)

    arrays, meta = {}, []
    cases = vector_cases()
    for ci, (name, cells, t, attrs) in enumerate(cases):
        arrays[f"v{ci}_in"] = cells
        row = [ci, t, attrs]
        for v in VERBS:
            got, rt, ra = answer(getattr(lib, "ray_" + v)(vec(cells, t, attrs)))
            if got is not None:
                if rt == T_I64:
                    assert got.size == 0 or (got.min() >= 0 and got.max() < 2**31)
                    got = got.astype(np.int32)
                arrays[f"v{ci}_{v}"] = got
            row += [rt, ra]
        meta.append(row)
        print(name, row)
    arrays["vector_cases"] = np.array(meta, np.int64)  # ci, type, attrs, then per verb (answer's type -- 127: an error --, answer's attrs)
    arrays["vector_names"] = np.array([c[0] for c in cases])
    path = os.path.join(HERE, "sort_narrow_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
