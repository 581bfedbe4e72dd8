#!/usr/bin/env python
"""Golden `last` and `dev` answers from the compiled reference library -- build container only.

    python tests/golden/make_lastdev_golden.py     # writes tests/golden/lastdev_golden.npz

Calls the reference's own index_group(keys, filter), aggr_last / aggr_dev(val, index) (core/aggr.c:851-930, 2250-2350, 2864-2929), ray_last(x)
(core/items.c:1073-1115) and ray_dev(x) (core/math.c:2628-2699) through ctypes on oracle/_ref/librayforce_ref.so, in one child process per executor
count (runtime_create with `-c N`: the pool is made once per process).

Grouped cases (about 2 000 rows each): dense (SHIFT) and sparse (IDS) keys, with and without filter ids, I64 / F64 / TIMESTAMP values; a group of one
row, an all-null group, a group whose last row is null, a group whose only non-null cell is its first row, an all-equal group (dev's clamp), a group
whose mean is far larger than its spread (cancellation), +-0.0, +-inf, subnormals, I64 extremes near +-2^63.  Every one runs with 1 and with 8
executors and the script asserts that the answers agree (fewer than 16 384 selected rows: aggr_map does not split, core/pool.c:36,450-479).
One grouped `last` case of 40 000 rows runs with 1 executor; whether the 8-executor answer differed is recorded in `big_last_differs_c8` -- the
evidence for DESIGN.md section 4 (AGGR_COLLECT keeps the FIRST chunk that has a value, core/aggr.c:909-930).
Scalar cases: empty, one cell, trailing null, all null, I64 sums that wrap (ray_dev's favg).  The fixture is data only (inputs stored in full)."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
T_LIST, T_I64, T_TIMESTAMP, T_F64 = 0, 5, 9, 10
NULL = -(2**63)


class Obj(C.Structure):
    _fields_ = [("mmod", C.c_uint8), ("order", C.c_uint8), ("type", C.c_int8), ("attrs", C.c_uint8), ("rc", C.c_uint32), ("len", C.c_int64)]


def group_cases():
    """(name, keys, values, value type, filter ids or None)"""
    rng = np.random.default_rng(20261017)
    out = []
    # group shapes by key: 0 one row; 1 all equal; 2 all null; 3 the last row null; 4 only the first row non-null; 5 mean >> spread; 6 I64 extremes;
    # the rest random lengths with 30 % nulls
    base = np.concatenate([[0], [1] * 6, [2] * 4, [3] * 5, [4] * 5, [5] * 40, [6] * 6, rng.integers(7, 60, 1933)]).astype(np.int64)
    order = rng.permutation(len(base))
    dense = base[order]
    n = len(dense)
    rows_of = lambda k: np.flatnonzero(dense == k)  # ascending rows
    vi = rng.integers(-1000, 1000, n)
    vi = np.where(rng.random(n) < 0.3, NULL, vi)
    vi[rows_of(0)] = 11
    vi[rows_of(1)] = 77
    vi[rows_of(2)] = NULL
    vi[rows_of(3)] = [5, NULL, 9, 7, NULL]
    vi[rows_of(4)] = [42, NULL, NULL, NULL, NULL]
    vi[rows_of(5)] = 10**15 + rng.integers(0, 3, 40)
    vi[rows_of(6)] = [2**63 - 1, -(2**63) + 1, 2**63 - 2, -(2**63) + 2, 2**62, -(2**62)]
    vf = rng.standard_normal(n) * 1e3
    r = rng.integers(0, 40, n)
    vf[r == 1], vf[r == 2], vf[r == 3], vf[r == 4], vf[r == 5], vf[r == 6] = 0.0, -0.0, np.inf, -np.inf, 5e-324, -1e-310
    vf = np.where(rng.random(n) < 0.3, np.nan, vf)
    vf[rows_of(0)] = -0.0
    vf[rows_of(1)] = 2.5
    vf[rows_of(2)] = np.nan
    vf[rows_of(3)] = [5.0, np.nan, 9.0, 7.5, np.nan]
    vf[rows_of(4)] = [42.0, np.nan, np.nan, np.nan, np.nan]
    vf[rows_of(5)] = 1e9 + rng.standard_normal(40) * 1e-3
    vf[rows_of(6)] = [1e300, -1e300, 1e-300, 5e-324, 0.0, -0.0]
    ts = rng.integers(-(2**60), 2**60, n)
    ts = np.where(rng.random(n) < 0.3, NULL, ts)
    ts[rows_of(2)] = NULL
    ts[rows_of(3)] = [5, NULL, 9, 7, NULL]
    sparse = np.array([(int(k) * 0x9E3779B97F4A7C15) & ((1 << 62) - 1) for k in dense], np.int64)  # same groups, keys far apart: the IDS index
    filt = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)
    for kname, keys in (("dense", dense), ("sparse", sparse)):
        for vname, vals, vt in (("i64", vi, T_I64), ("f64", vf, T_F64), ("ts", ts, T_TIMESTAMP)):
            for fl in (None, filt):
                out.append((f"{kname}_{vname}_{'filter' if fl is not None else 'all'}", keys, vals, vt, fl))
    return out


def big_case():
    """40 000 rows, k = i % 4, v = i: the reference's chunks split here with 8 executors"""
    i = np.arange(40_000, dtype=np.int64)
    return i % 4, i.copy()


def scalar_cases():
    rng = np.random.default_rng(8)
    cases = [np.array(v, np.int64) for v in (
        [], [5], [NULL], [3, 1, 2], [3, 1, NULL], [NULL, NULL, NULL], [NULL, 5], [7, 7, 7, 7],
        [2**62 + 1, 2**62 + 3], [2**63 - 1, 2**63 - 1, 5], [-(2**63) + 1, -(2**63) + 3, -7], [2**62] * 5,
        rng.integers(-(2**62), 2**62, 1001), np.where(rng.random(999) < 0.1, NULL, rng.integers(-1000, 1000, 999)))]
    f = rng.standard_normal(1000) * 1e3
    f[rng.random(1000) < 0.1] = np.nan
    cases += [np.array(v, np.float64) for v in ([], [2.5], [np.nan], [1.0, np.nan], [np.nan, np.nan], [0.0, -0.0], [np.inf, 1.0], [5e-324, -1e-310, 0.0],
                                               [1e9 + 1e-3, 1e9 - 1e-3, 1e9], f)]
    return cases


def child(threads: int, out_path: str):
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "librayforce_ref.so"))
    argv = (C.c_char_p * 3)(b"rayforce", b"-c", str(threads).encode())
    lib.runtime_create.restype = C.c_void_p
    lib.runtime_create.argtypes = [C.c_int32, C.POINTER(C.c_char_p)]
    assert lib.runtime_create(3, argv)
    lib.vector.restype = C.c_void_p
    lib.vector.argtypes = [C.c_int8, C.c_int64]
    for f in ("index_group", "aggr_last", "aggr_dev"):
        getattr(lib, f).restype = C.c_void_p
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p]
    for f in ("ray_last", "ray_dev"):
        getattr(lib, f).restype = C.c_void_p
        getattr(lib, f).argtypes = [C.c_void_p]
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
        return np.frombuffer((C.c_char * (h.len * 8)).from_address(o + 16), dtype=np.float64 if h.type == T_F64 else np.int64).copy(), int(h.type)

    def slot(index, i):
        return C.c_void_p.from_address(index + 16 + 8 * i).value

    def atom_i64(o):
        return C.c_int64.from_address(o + 8).value

    res = {"groups": [], "scalars": []}
    for name, keys, vals, vt, fl in group_cases():
        index = lib.index_group(vec(keys), vec(fl) if fl is not None else null_obj)
        assert Obj.from_address(index).type == T_LIST and Obj.from_address(index).len == 7
        itype, groups = atom_i64(slot(index, 0)), atom_i64(slot(index, 1))
        last, lt = arr(lib.aggr_last(vec(vals, vt), index))
        dev, dt = arr(lib.aggr_dev(vec(vals, vt), index))
        assert len(last) == groups and len(dev) == groups and lt == vt and dt == T_F64, (name, lt, dt)
        res["groups"].append(dict(name=name, itype=itype, groups=groups, ix=arr(slot(index, 2))[0], shift=atom_i64(slot(index, 3)) if itype == 1 else NULL, last=last, dev=dev))
    keys, vals = big_case()
    index = lib.index_group(vec(keys), null_obj)
    res["big"] = dict(itype=atom_i64(slot(index, 0)), groups=atom_i64(slot(index, 1)), ix=arr(slot(index, 2))[0], shift=atom_i64(slot(index, 3)),
                      last=arr(lib.aggr_last(vec(vals), index))[0])
    for v in scalar_cases():
        rl, rd = lib.ray_last(vec(v)), lib.ray_dev(vec(v))
        hl, hd = Obj.from_address(rl), Obj.from_address(rd)
        assert hd.type == -T_F64, hd.type
        assert hl.type == (-T_F64 if v.dtype == np.float64 else -T_I64), hl.type
        res["scalars"].append((bytes((C.c_char * 8).from_address(rl + 8)), C.c_double.from_address(rd + 8).value))
    with open(out_path, "wb") as f:
        pickle.dump(res, f)


def run_child(threads: int):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "answers.pkl")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(threads), path], check=True)
        with open(path, "rb") as f:
            return pickle.load(f)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    r1, r8 = run_child(1), run_child(8)
    arrays, meta = {}, []
    for ci, ((name, keys, vals, vt, fl), g1, g8) in enumerate(zip(group_cases(), r1["groups"], r8["groups"])):
        assert g1["itype"] == g8["itype"] and g1["groups"] == g8["groups"] and same(g1["ix"], g8["ix"]), name
        assert same(g1["last"], g8["last"]), f"{name}: last differs between 1 and 8 executors below 16 384 rows"
        assert same(g1["dev"], g8["dev"]), f"{name}: dev differs between 1 and 8 executors"
        pre = f"g{ci}_"
        arrays[pre + "keys"], arrays[pre + "vals"], arrays[pre + "ix"] = keys, vals, g1["ix"]
        if fl is not None:
            arrays[pre + "filter"] = fl
        arrays[pre + "last"], arrays[pre + "dev"] = g1["last"], g1["dev"]
        meta.append([ci, vt, g1["itype"], g1["groups"], g1["shift"], int(fl is not None)])
        print(name, "index type", g1["itype"], "groups", g1["groups"])
    b1, b8 = r1["big"], r8["big"]
    keys, vals = big_case()
    arrays["big_keys"], arrays["big_vals"], arrays["big_ix"], arrays["big_last"] = keys, vals, b1["ix"], b1["last"]
    arrays["big_meta"] = np.array([T_I64, b1["itype"], b1["groups"], b1["shift"]], np.int64)
    arrays["big_last_differs_c8"] = np.array(int(not same(b1["last"], b8["last"])), np.int64)
    arrays["big_last_c8"] = b8["last"]
    print("40 000 rows: last with 1 executor", b1["last"], "with 8", b8["last"])
    for si, (v, s1, s8) in enumerate(zip(scalar_cases(), r1["scalars"], r8["scalars"])):
        assert s1[0] == s8[0] and np.float64(s1[1]).tobytes() == np.float64(s8[1]).tobytes(), si
        arrays[f"s{si}_vals"] = v
        arrays[f"s{si}_last"] = np.frombuffer(s1[0], dtype=v.dtype).copy()
        arrays[f"s{si}_dev"] = np.array([s1[1]])
    arrays["group_cases"] = np.array(meta, np.int64)
    arrays["scalar_cases"] = np.array(len(scalar_cases()), np.int64)
    np.savez_compressed(os.path.join(HERE, "lastdev_golden.npz"), **arrays)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3])
    else:
        main()
