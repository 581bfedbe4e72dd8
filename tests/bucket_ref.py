"""numpy restatement of the bucket verbs -- xrank, xbar, within, floor, ceil, round, neg -- as the reference computes them (core/order.c:445-649,
core/math.c:1635-1782,2047-2117, core/items.c:848-872, core/ops.h:190-197), held to tests/golden/bucket_golden.npz by test_bucket_cpu.py.

Cells travel as numpy arrays of the type's storage: int32 (I32 4, DATE 7, TIME 8), int64 (I64 5, TIMESTAMP 9), float64 (F64 10), f64 answers compared
by their BITS.  An atom is a 1-cell array with atom=True."""
import numpy as np

I32, I64, DATE, TIME, TS, F64, B8 = 4, 5, 7, 8, 9, 10, 1
NULL32, NULL64 = -(2**31), -(2**63)
NAN_BITS = np.uint64(0x7FF8000000000000)
DTYPE = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}
ATTR_ASC, ATTR_DESC = 2, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def isnan_bits(u):  # ISNANF64, core/ops.h:63-70
    return ((u & np.uint64(0x7FF0000000000000)) == np.uint64(0x7FF0000000000000)) & ((u & np.uint64(0x000FFFFFFFFFFFFF)) != 0)


def sort_key(v, tp):
    """the order the reference's sorts rank by (core/sort.c:266-311): i64 x ^ 2^63; f64 NaN -> 0, negative -> ~bits, else bits | 2^63"""
    if tp == F64:
        u = bits(v)
        neg = (u >> np.uint64(63)) == 1
        k = np.where(neg, ~u, u | np.uint64(1 << 63))
        return np.where(isnan_bits(u), np.uint64(0), k)
    return np.ascontiguousarray(v, dtype=np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def xrank(v, tp, nb, attrs=0):
    """(xrank v nb): (rank * nb) / len; ATTR_ASC / ATTR_DESC answer from the index alone (core/order.c:627-636), ascending first"""
    n = len(v)
    if n == 0:
        return np.empty(0, np.int64)
    idx = np.arange(n, dtype=np.int64)
    if attrs & ATTR_ASC:
        rank = idx
    elif attrs & ATTR_DESC:
        rank = n - 1 - idx
    else:
        rank = np.empty(n, np.int64)
        rank[np.argsort(sort_key(v, tp), kind="stable")] = idx
    return (rank * np.int64(nb)) // np.int64(n)  # (rank * nb < 2^63: non-negative, floor == C's truncation)


def ftz(x):
    """the reference's build runs with denormals-are-zero / flush-to-zero (its unsafe-math link sets MXCSR so): a subnormal operand or result is a signed zero"""
    u = bits(x)
    return np.where((u & np.uint64(0x7FF0000000000000)) == 0, u & np.uint64(1 << 63), u).view(np.float64)


def cvt_x86(x):
    """(i64_t)x as cvttsd2si converts: NaN, infinities and anything outside [-2^63, 2^63) give INT64_MIN"""
    ok = (x >= -9223372036854775808.0) & (x < 9223372036854775808.0)
    with np.errstate(invalid="ignore"):
        return np.where(ok, np.where(ok, x, 0.0).astype(np.int64), np.int64(NULL64))


def _floor_vals(x):  # FLOORF64 for non-NaN cells
    x = ftz(x)
    t = cvt_x86(x)
    td = t.astype(np.float64)
    return np.where((x < 0.0) & (td != x), td - 1.0, td)


def floor(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.where(isnan_bits(bits(x)), NAN_BITS, bits(_floor_vals(x)))


def ceil(x):  # -FLOORF64(-x)
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.where(isnan_bits(bits(x)), NAN_BITS, bits(_floor_vals(-x)) ^ np.uint64(1 << 63))


def round_(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.where(x >= 0.0, cvt_x86(x + 0.5), cvt_x86(x - 0.5)).astype(np.float64)
    return np.where(isnan_bits(bits(x)), NAN_BITS, bits(r))


def neg(x, tp):
    """ray_neg's vector arms: I32 / I64 -> I64 (-(i64)x; the i64 negation wraps), F64 -> the sign flipped"""
    if tp == F64:
        return bits(x) ^ np.uint64(1 << 63)
    with np.errstate(over="ignore"):
        return (np.uint64(0) - np.ascontiguousarray(x).astype(np.int64).view(np.uint64)).view(np.int64)


def within(x, lo, hi):
    x = np.ascontiguousarray(x, dtype=np.int64)
    return ((x >= lo) & (x <= hi)).astype(np.int8)


# ---- xbar: the arm of ray_xbar_partial by (x type, y type) -> (middle type, result type); time_to_timestamp when a TIME meets a TIMESTAMP
def xbar_arm(xt, yt):
    yi = yt in (I32, I64)
    if xt == I32:
        return {I32: (I32, I32), I64: (I64, I64), F64: (F64, F64)}.get(yt)
    if xt == I64:
        return (I64, I64) if yi else ((F64, F64) if yt == F64 else None)
    if xt == F64:
        return (F64, F64) if yi or yt == F64 else None
    if xt == DATE:
        return ((I32 if yt == I32 else I64), DATE) if yi else None
    if xt == TIME:
        return (I32, TIME) if yt in (I32, TIME) else ((I64, TIME) if yt == I64 else None)
    if xt == TS:
        return (I64, TS) if yi or yt == TIME else None
    return None


def _to_mid(a, tp, mid, time_scale=False):
    four = tp in (I32, DATE, TIME)
    null = (a == NULL32) if four else ((a == NULL64) if tp != F64 else None)
    if mid == F64:
        if tp == F64:
            return np.ascontiguousarray(a, dtype=np.float64)
        return np.where(null, np.nan, a.astype(np.float64))
    if mid == I64:
        w = a.astype(np.int64)
        if four:
            w = np.where(null, np.int64(NULL64), w * (1000000 if time_scale else 1))
        return w
    return a.astype(np.int32)


def _xbar_int(x, y, null):
    """XBARI32 / XBARI64: C's truncating division spelt with floor division on magnitudes (the cells the goldens hold never overflow their type)"""
    dt = x.dtype
    bad = (y == 0) | (x == null) | (y == null)
    ys = np.where(bad, 1, y).astype(np.int64)
    xs = np.where(bad, 0, x).astype(np.int64)
    a = np.where(xs < 0, xs + 1 - ys, xs)
    q = (np.abs(a) // np.abs(ys)) * np.where((a < 0) == (ys < 0), 1, -1)
    return np.where(bad, np.int64(null), q * ys).astype(dt)


def xbar(x, xt, y, yt, x_atom=False, y_atom=False):
    """-> (cells in the result's storage (f64 as uint64 bits), result type code)"""
    mid, ot = xbar_arm(xt, yt)
    n = len(y) if x_atom else len(x)
    xs = np.broadcast_to(x, n) if x_atom else x
    ys = np.broadcast_to(y, n) if y_atom else y
    xm = _to_mid(np.ascontiguousarray(xs), xt, mid)
    ym = _to_mid(np.ascontiguousarray(ys), yt, mid, time_scale=(xt == TS and yt == TIME))
    if mid == F64:
        # the reference's build divides by an ATOM through its reciprocal (reciprocal-math: 1 / y once, then x * r); a vector divisor is divided by.
        # A NaN made by the product itself (0 * inf) is x86's default NaN, the sign bit set; a null quotient stays the null.
        with np.errstate(all="ignore"):
            xm, ym = ftz(xm), ftz(ym)
            q = ftz(xm * ftz(1.0 / ym)) if y_atom else ftz(xm / ym)
            fb = floor(q)
            r = bits(ftz(fb.view(np.float64) * ym))
        return np.where(isnan_bits(r), np.where(isnan_bits(fb), NAN_BITS, np.uint64(0xFFF8000000000000)), r), ot
    if mid == I32:
        return _xbar_int(xm, ym, NULL32), ot
    r = _xbar_int(xm, ym, NULL64)
    if ot in (DATE, TIME):  # i64_to_date / i64_to_time: null -> NULL_I32, else truncated
        r = np.where(r == NULL64, np.int64(NULL32), r).astype(np.uint64).astype(np.uint32).view(np.int32) if len(r) else np.empty(0, np.int32)
    return r, ot


# ---- the fixture (tests/golden/make_bucket_golden.py) ----
def _unplane(p, tp):
    dt = np.dtype(DTYPE[tp])
    return np.ascontiguousarray(p.T).reshape(-1).view(dt) if p.size else np.empty(0, dt)


_CASES = None


def load_cases():
    """every golden case as a dict: name verb xt yt xa ya attrs ot, x / y / out as arrays of their type's storage (read once, shared, left unchanged)"""
    global _CASES
    if _CASES is None:
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bucket_golden.npz"))
        _CASES = []
        for k, meta in enumerate(z["cases"]):
            name, verb, xt, yt, xa, ya, attrs, ot, _, tiles = str(meta).split("|")
            tiles = dict(t.split(":") for t in tiles.split(",") if t)
            c = dict(name=name, verb=verb, xt=int(xt), yt=int(yt), xa=xa == "1", ya=ya == "1", attrs=int(attrs), ot=int(ot))
            c["x"] = _unplane(z[f"c{k}_x"], c["xt"])
            c["y"] = _unplane(z[f"c{k}_y"], c["yt"]) if c["yt"] else None
            c["out"] = _unplane(z[f"c{k}_out"], c["ot"])
            for tag, n in tiles.items():  # held as its pattern of 800 cells: repeated to its length
                c[tag] = np.resize(c[tag], int(n))
            for a in (c["x"], c["y"], c["out"]):
                if a is not None:
                    a.setflags(write=False)
            _CASES.append(c)
    return _CASES


def answer(c):
    """the restatement's answer to a golden case: (cells in the answer type's storage, f64 as uint64 bits; answer type code)"""
    v = c["verb"]
    if v == "xrank":
        return xrank(c["x"], c["xt"], int(c["y"][0]), c["attrs"]), I64
    if v == "xbar":
        return xbar(c["x"], c["xt"], c["y"], c["yt"], c["xa"], c["ya"])
    if v == "within":
        return within(c["x"], int(c["y"][0]), int(c["y"][1])), B8
    if v == "neg":
        return neg(c["x"], c["xt"]), (F64 if c["xt"] == F64 else I64)
    return {"floor": floor, "ceil": ceil, "round": round_}[v](c["x"]), F64


def as_bits(a):
    """cells for a bit-for-bit comparison: f64 as uint64"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a
