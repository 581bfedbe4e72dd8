"""The `med` contract restated in numpy (the reference's aggr_med, core/aggr.c:2136-2247, and ray_med, core/math.c:2529-2626): every selected value
counts, nulls included; a group's values are ranked by the reference's 64-bit sort keys (core/sort.c:266-311); the median is the value of rank
l // 2 for odd l, else a fixed formula of the values of ranks l // 2 - 1 and l // 2 -- grouped: both halves as f64 first, scalar i64: added as
wrapping i64 first, and its l counts the non-null values only (the ranks still index the whole sorted vector, nulls first); f64 arithmetic
flushes subnormals as the reference's release build does.  Pinned against the compiled reference by tests/golden/med_golden.npz.  What the
device kernels are held to, bit for bit, at sizes the reference cannot reach."""
import numpy as np

GROUPED, SCALAR = 0, 1
NULL_I64 = -(2**63)
TOP = np.uint64(1 << 63)


def sort_keys(v: np.ndarray) -> np.ndarray:
    """i64: x ^ 2^63 (NULL_I64 first).  f64: NaN -> 0, negative -> ~bits, otherwise bits | 2^63 (-0.0 before +0.0)."""
    if v.dtype == np.float64:
        b = v.view(np.uint64)
        k = np.where((b & TOP) != 0, ~b, b | TOP)
        k[np.isnan(v)] = 0
        return k
    return v.astype(np.int64).view(np.uint64) ^ TOP


def from_keys(k: np.ndarray, f64: bool) -> np.ndarray:
    if not f64:
        return (k ^ TOP).view(np.int64)
    b = np.where((k & TOP) != 0, k & ~TOP, ~k)
    out = b.view(np.float64).copy()
    out[k == 0] = np.nan
    return out


def flush(x: np.ndarray) -> np.ndarray:
    """A subnormal as the zero of its sign: the reference's release build runs with the x86 FTZ / DAZ modes (-funsafe-math-optimizations)."""
    b = np.asarray(x, np.float64).view(np.uint64)
    return np.where((b & np.uint64(0x7FF0000000000000)) == 0, (b & TOP).view(np.float64), np.asarray(x, np.float64))


def finish(lo_k: np.ndarray, hi_k: np.ndarray, length: np.ndarray, f64: bool, rule: int) -> np.ndarray:
    lo, hi = from_keys(lo_k, f64), from_keys(hi_k, f64)
    with np.errstate(all="ignore"):
        if f64:
            even = flush(flush(flush(lo) + flush(hi)) / 2.0)
            odd = hi.copy()
        else:
            even = (lo + hi).astype(np.float64) / 2.0 if rule == SCALAR else (lo.astype(np.float64) + hi.astype(np.float64)) / 2.0
            odd = hi.astype(np.float64)
    out = np.where(length % 2 == 1, odd, even)
    out[length == 0] = np.nan
    return out


def group_median(values: np.ndarray, gids: np.ndarray, groups: int, rule: int = GROUPED) -> np.ndarray:
    """Medians of `values` per group: row i is in group gids[i] (rows outside [0, groups) do not count)."""
    f64 = values.dtype == np.float64
    m = (gids >= 0) & (gids < groups)
    if rule == SCALAR:
        assert groups == 1 and not f64
        return np.array([median(values[m])])
    g, k = gids[m].astype(np.int64), sort_keys(values[m])
    order = np.lexsort((k, g))
    ks = k[order]
    cnt = np.bincount(g, minlength=groups).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    lo_i, hi_i = off + np.maximum(cnt - 1, 0) // 2, off + cnt // 2
    last = max(len(ks) - 1, 0)
    pad = ks if len(ks) else np.zeros(1, np.uint64)
    lo_k, hi_k = pad[np.minimum(lo_i, last)], pad[np.minimum(hi_i, last)]
    return finish(lo_k, hi_k, cnt, f64, rule)


def median(values: np.ndarray) -> float:
    """ray_med of an I64 vector (the scalar rule): l = ray_cnt(x), the NON-NULL count (CNTI64, core/ops.h:151), but the ranks l // 2 (- 1) are
    read in the whole sorted vector, whose nulls sort first."""
    v = np.asarray(values, np.int64)
    l = int((v != NULL_I64).sum())
    if l == 0:
        return float("nan")
    k = np.sort(sort_keys(v))
    return float(finish(k[[(l - 1) // 2]], k[[l // 2]], np.array([l]), False, SCALAR)[0])


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
