"""`as` over vectors restated in numpy -- cast_obj's vector arms (core/rayforce.c:2558-2752) as the reference's x86 build computes them -- and the loader
of tests/golden/cast_golden.npz, the compiled reference's own answers.  These are copies: cells, type code and attribute byte must agree bit for bit.
Test infrastructure only."""
import os

import numpy as np

B8, U8, I16, I32, I64, DATE, TIME, TS, F64 = 1, 2, 3, 4, 5, 7, 8, 9, 10
TYPES = (B8, U8, I16, I32, I64, DATE, TIME, TS, F64)
DTYPE = {B8: np.int8, U8: np.uint8, I16: np.int16, I32: np.int32, I64: np.int64, DATE: np.int32, TIME: np.int32, TS: np.int64, F64: np.float64}
VECTOR_NAME = {B8: "B8", U8: "U8", I16: "I16", I32: "I32", I64: "I64", DATE: "DATE", TIME: "TIME", TS: "TIMESTAMP", F64: "F64"}
ATOM_NAME = {t: n.lower() for t, n in VECTOR_NAME.items()}
NULL32, NULL64 = -(2**31), -(2**63)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cast_golden.npz")
# the lengths of the fixture: around a lane's run of cells (4, 8 or 16 by the narrower side), the wave (64 lanes) and the block (256 lanes) of rfx_cast.hip
# -- 16 cells x 64 lanes = 1024, 4 x 256 = 1024, 16 x 256 = 4096 -- whichever of them an arm has
LENS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
BIG = 2**20 + 5


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def has_arm(st, dt):
    """does cast_obj have a vector arm st -> dt (or answer without one: the same type)?  B8 <-> U8 is its type error"""
    return st in TYPES and dt in TYPES and {st, dt} != {B8, U8}


def cast(cells, st, dt):
    """the cells of (as 'dt x) for a vector x of type st: one C cast per cell, nulls not carried"""
    cells = np.ascontiguousarray(cells, dtype=DTYPE[st])
    if st == dt:
        return cells.copy()
    if cells.size == 0:  # (answered before the arms are looked at: an empty B8 casts to an empty U8)
        return np.empty(0, DTYPE[dt])
    assert has_arm(st, dt)
    if st == F64:
        with np.errstate(invalid="ignore"):
            if dt in (I64, TS):  # cvttsd2si r64: outside [-2^63, 2^63), a NaN included -> INT64_MIN
                ok = (cells >= -(2.0**63)) & (cells < 2.0**63)
                return np.where(ok, np.trunc(np.where(ok, cells, 0.0)).astype(np.int64), NULL64).astype(DTYPE[dt])
            ok = (cells > -2147483649.0) & (cells < 2147483648.0)  # cvttsd2si r32: what does not truncate into the i32 range -> INT32_MIN
            v = np.where(ok, np.trunc(np.where(ok, cells, 0.0)).astype(np.int64), NULL32)
        return v.astype(DTYPE[dt])  # I16 / U8 / B8: the 32-bit result's low bits
    v = cells.view(np.uint8).astype(np.int64) if st in (B8, U8) else cells.astype(np.int64)  # B8 / U8 zero-extend, the others sign-extend
    return v.astype(DTYPE[dt])  # (to F64: (double)x, NULL_I64 -> -2^63; to a narrower integer: the low bytes)


# ---- the fixture ----
def planes(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return np.ascontiguousarray(a.view(np.uint8).reshape(-1, a.dtype.itemsize).T)


def unplanes(p, tp):
    return np.ascontiguousarray(p.T).reshape(-1).view(DTYPE[tp]).copy()


def load_cases():
    """-> [dict(name, st, dt, spelling "atom" | "vector", type_name, n, x, attrs, out (None: a host_ case), ot, oattrs, host: the reason the shape is
    handed to the host (the spelling field is then the name itself when it names none of the nine), ref_error: the reference itself answers an error,
    threads)]; cases of one source share their x, both spellings their out"""
    npz = np.load(GOLDEN)
    blob, z, cache = npz["blob"], {}, {}
    for line in npz["index"]:  # "key|dtype|shape|offset|bytes": the arrays, cut out of the one blob
        key, *dt, shape, at, nbytes = str(line).split("|")  # (a dtype string may itself hold a bar: "|u1")
        z[key] = (int(at), int(nbytes), "|".join(dt), [int(d) for d in shape.split("x")])

    def cells(key, tp):
        if key not in cache:
            at, nbytes, dt, shape = z[key]
            cache[key] = unplanes(blob[at:at + nbytes].view(np.dtype(dt)).reshape(shape), tp)
            cache[key].setflags(write=False)
        return cache[key]

    out = []
    for line in npz["cases"]:
        name, st, dt, spelling, n, xkey, attrs, okey, ot, oattrs, host, ref_error, threads = str(line).split("|")
        st, dt, n = int(st), int(dt), int(n)
        type_name = {"atom": ATOM_NAME.get(dt), "vector": VECTOR_NAME.get(dt)}.get(spelling, spelling)
        c = dict(name=name, st=st, dt=dt, spelling=spelling, type_name=type_name, n=n, attrs=int(attrs),
                 x=cells(xkey, st) if n else np.empty(0, DTYPE[st]), out=None, ot=None, oattrs=None, host=host or None, ref_error=ref_error == "1", threads=threads)
        if not host:
            c["ot"], c["oattrs"] = int(ot), int(oattrs)
            c["out"] = cells(okey, c["ot"]) if n else np.empty(0, DTYPE[c["ot"]])
        out.append(c)
    return out
