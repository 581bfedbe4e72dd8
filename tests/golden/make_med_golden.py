#!/usr/bin/env python
"""Golden medians from the compiled reference library -- build container only.

    python tests/golden/make_med_golden.py     # writes tests/golden/med_golden.npz

Calls the reference's own index_group(keys, filter), aggr_med(val, index) (core/aggr.c:2136-2247) and ray_med(x) (core/math.c:2529-2626)
through ctypes on oracle/_ref/librayforce_ref.so.  Per grouped case: the inputs (keys, values, optional filter ids), the index's slots
(type, group count, group ids or key table, shift) and aggr_med's result.  Per scalar case: the I64 vector and ray_med's answer.  The cases
hold odd and even group lengths, NULL_I64 and NaN values, +-0.0, +-inf and subnormals, i64 pairs whose integer sum wraps, all-null,
one-row and all-equal groups, SHIFT and IDS indexes, with and without filter ids.  The fixture is data only (inputs stored in full)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
T_LIST, T_I64, T_TIMESTAMP, T_F64 = 0, 5, 9, 10
NULL = -(2**63)


class Obj(C.Structure):
    _fields_ = [("mmod", C.c_uint8), ("order", C.c_uint8), ("type", C.c_int8), ("attrs", C.c_uint8), ("rc", C.c_uint32), ("len", C.c_int64)]


def group_cases():
    """(name, keys, values, value type, filter ids or None)"""
    rng = np.random.default_rng(20261016)
    out = []
    # group shapes: key 0 one row, key 1 all equal, key 2 all null, key 3 two rows whose i64 sum wraps, the rest random lengths
    base = np.concatenate([[0], [1] * 5, [2] * 4, [3] * 2, rng.integers(4, 60, 1988)]).astype(np.int64)
    order = rng.permutation(len(base))
    dense = base[order]
    vi = rng.choice(np.array([NULL, 2**63 - 1, -(2**63) + 1, 0, -1, 1, 2**62, -(2**62)], np.int64), len(base))
    vi = np.where(rng.random(len(base)) < 0.5, rng.integers(-1000, 1000, len(base)), vi)
    vi = np.where(base[order] == 1, 77, vi)
    vi = np.where(base[order] == 2, NULL, vi)
    vi[np.flatnonzero(base[order] == 3)] = [2**62 + 1, 2**62 + 3]
    vf = rng.standard_normal(len(base)) * 1e3
    r = rng.integers(0, 30, len(base))
    vf[r == 0], vf[r == 1], vf[r == 2], vf[r == 3], vf[r == 4], vf[r == 5], vf[r == 6] = np.nan, 0.0, -0.0, np.inf, -np.inf, 5e-324, -1e-310
    vf = np.where(base[order] == 1, 2.5, vf)
    vf = np.where(base[order] == 2, np.nan, vf)
    sparse = np.array([(int(k) * 0x9E3779B97F4A7C15) & ((1 << 62) - 1) for k in dense], np.int64)  # same groups, keys far apart: the IDS index
    filt = np.sort(rng.choice(len(base), len(base) // 2, replace=False)).astype(np.int64)
    ts = rng.integers(-(2**60), 2**60, len(base))
    ts[r == 0] = NULL
    for kname, keys in (("dense", dense), ("sparse", sparse)):
        for vname, vals, vt in (("i64", vi, T_I64), ("f64", vf, T_F64), ("ts", ts, T_TIMESTAMP)):
            for fl in (None, filt):
                out.append((f"{kname}_{vname}_{'filter' if fl is not None else 'all'}", keys, vals, vt, fl))
    return out


def scalar_cases():
    rng = np.random.default_rng(7)
    return [np.array(v, np.int64) for v in (
        [3, 1, 2], [4, 1, 3, 2], [7, 7, 7, 7], [2**62 + 1, 2**62 + 3], [2**63 - 1, 2**63 - 1, 5], [-(2**63) + 1, -(2**63) + 3],
        [NULL], [NULL, NULL], [NULL, 5], [NULL, 5, 7], [NULL, NULL, 5, 7, 9], [5, NULL, 9, 1], [],
        rng.integers(-(2**62), 2**62, 1001), rng.integers(-(2**62), 2**62, 1000),
        np.where(rng.random(999) < 0.1, NULL, rng.integers(-1000, 1000, 999)))]


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "librayforce_ref.so"))
    lib.ray_init.restype = C.c_int32
    assert lib.ray_init() == 0
    lib.vector.restype = C.c_void_p
    lib.vector.argtypes = [C.c_int8, C.c_int64]
    for f in ("index_group", "aggr_med"):
        getattr(lib, f).restype = C.c_void_p
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p]
    lib.ray_med.restype = C.c_void_p
    lib.ray_med.argtypes = [C.c_void_p]
    null_obj = C.addressof(Obj.in_dll(lib, "__NULL_OBJ"))

    def vec(a, t=None):
        a = np.ascontiguousarray(a)
        o = lib.vector(t if t is not None else (T_F64 if a.dtype == np.float64 else T_I64), a.size)
        if a.size:
            C.memmove(o + 16, a.ctypes.data, a.nbytes)
        return o

    def arr(o):
        h = Obj.from_address(o)
        assert h.type in (T_I64, T_F64, T_TIMESTAMP), h.type
        dt = np.float64 if h.type == T_F64 else np.int64
        return np.frombuffer((C.c_char * (h.len * 8)).from_address(o + 16), dtype=dt).copy()

    def slot(index, i):
        return C.c_void_p.from_address(index + 16 + 8 * i).value

    def atom_i64(o):
        return C.c_int64.from_address(o + 8).value

    arrays, meta = {}, []
    for ci, (name, keys, vals, vt, fl) in enumerate(group_cases()):
        index = lib.index_group(vec(keys), vec(fl) if fl is not None else null_obj)
        assert Obj.from_address(index).type == T_LIST and Obj.from_address(index).len == 7
        itype, groups = atom_i64(slot(index, 0)), atom_i64(slot(index, 1))
        res = arr(lib.aggr_med(vec(vals, vt), index))
        assert len(res) == groups and res.dtype == np.float64
        pre = f"g{ci}_"
        arrays[pre + "keys"], arrays[pre + "vals"], arrays[pre + "ix"] = keys, vals, arr(slot(index, 2))
        if fl is not None:
            arrays[pre + "filter"] = fl
        arrays[pre + "med"] = res
        shift = atom_i64(slot(index, 3)) if itype == 1 else NULL
        meta.append([ci, vt, itype, groups, shift, int(fl is not None)])
        print(name, "index type", itype, "groups", groups)
    for si, v in enumerate(scalar_cases()):
        r = lib.ray_med(vec(v))
        h = Obj.from_address(r)
        assert h.type == -T_F64, h.type
        arrays[f"s{si}_vals"] = v
        arrays[f"s{si}_med"] = np.array([C.c_double.from_address(r + 8).value])
    arrays["group_cases"] = np.array(meta, np.int64)
    arrays["scalar_cases"] = np.array(len(scalar_cases()), np.int64)
    np.savez_compressed(os.path.join(HERE, "med_golden.npz"), **arrays)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    main()
