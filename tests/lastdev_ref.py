"""numpy restatement of `last` and `dev`, scalar and grouped -- what the device answers (rfx_lastdev.hip) is checked against this, and this against the
compiled reference's own answers (tests/golden/lastdev_golden.npz).

last, scalar (ray_last: at_idx(x, len - 1), core/items.c:1112-1114): the cell at the last selected row, null or not; nothing selected: the typed null.
last, grouped (aggr_last with ONE chunk, core/aggr.c:851-930): per group the cell at the highest selected row whose cell is non-null; no such row: null.
dev, scalar (ray_dev, core/math.c:2628-2699): l = non-null count; 0 -> null, 1 -> 0.0; favg = (f64)(wrapping i64 sum) / l (f64: f64 sum / l);
    sqrt(sum (x - favg)^2 / l) over the non-null cells.
dev, grouped (aggr_dev, core/aggr.c:2250-2350,2864-2929): per group s = sum (f64)x, sq = sum (f64)x * (f64)x, n = non-null count; 0 -> null, 1 -> 0.0;
    mean = s / n, var = sq / n - mean * mean, var < 0 ? 0 : sqrt(var).
Nulls: NULL_I64 for I64 / TIMESTAMP cells, any NaN for F64 cells."""
import numpy as np

NULL_I64 = -(2**63)


def is_null(v: np.ndarray) -> np.ndarray:
    return np.isnan(v) if v.dtype == np.float64 else v == NULL_I64


def null_of(dtype):
    return np.nan if dtype == np.float64 else NULL_I64


def same_bits(a, b) -> bool:
    """bit for bit, except that every NaN is the null"""
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))
    return bool(np.array_equal(a, b))


def last(values: np.ndarray):
    return values[-1] if len(values) else values.dtype.type(null_of(values.dtype))


def group_last(values: np.ndarray, gids: np.ndarray, groups: int) -> np.ndarray:
    """values / gids: the SELECTED rows in row order (gid < 0: the row does not count)"""
    out = np.full(groups, null_of(values.dtype), values.dtype)
    ok = ~is_null(values) & (gids >= 0)
    rows = np.flatnonzero(ok)
    out[gids[rows]] = values[rows]  # (ascending rows: the highest row of a group is written last)
    return out


def group_last_rows(values: np.ndarray, gids: np.ndarray, groups: int) -> np.ndarray:
    """the row each group's answer sits at (-1: none)"""
    out = np.full(groups, -1, np.int64)
    rows = np.flatnonzero(~is_null(values) & (gids >= 0))
    out[gids[rows]] = rows
    return out


def dev(values: np.ndarray) -> float:
    v = values[~is_null(values)]
    l = len(v)
    if l == 0:
        return np.nan
    if l == 1:
        return 0.0
    if v.dtype == np.float64:
        favg = np.float64(np.sum(v)) / np.float64(l)
    else:
        with np.errstate(over="ignore"):
            favg = np.float64(np.sum(v.astype(np.uint64), dtype=np.uint64).astype(np.int64)) / np.float64(l)  # the wrapping integer sum
    with np.errstate(invalid="ignore", over="ignore"):
        t = v.astype(np.float64) - favg
        return float(np.sqrt(np.sum(t * t) / np.float64(l)))


def group_dev(values: np.ndarray, gids: np.ndarray, groups: int) -> np.ndarray:
    ok = ~is_null(values) & (gids >= 0)
    x = values[ok].astype(np.float64)
    g = gids[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.bincount(g, minlength=groups).astype(np.float64)
        s = np.bincount(g, weights=x, minlength=groups)
        sq = np.bincount(g, weights=x * x, minlength=groups)
        out = np.full(groups, np.nan)
        many = n > 1
        mean = s[many] / n[many]
        var = sq[many] / n[many] - mean * mean
        out[many] = np.where(var < 0, 0.0, np.sqrt(np.where(var < 0, 0.0, var)))  # (a NaN variance -- inf - inf -- stays NaN)
        out[n == 1] = 0.0
    return out


# ---- the bounds of the issue: a device f64 sum is within 1e-9 relative of the exact one ----
def group_dev_close(got: np.ndarray, want: np.ndarray, values: np.ndarray, gids: np.ndarray, groups: int):
    """|got^2 - want^2| <= 3e-9 * A with A = sum x^2 / n over the group's non-null cells in extended precision (1e-9 * A from the sum of squares,
    2e-9 * A from mean^2, since (sum |x| / n)^2 <= A); null and count-1 cells exact.  Returns the index of the first cell outside, or None."""
    ok = ~is_null(values) & (gids >= 0)
    x = values[ok].astype(np.longdouble)
    g = gids[ok]
    n = np.bincount(g, minlength=groups)
    A = np.zeros(groups, np.longdouble)
    np.add.at(A, g, x * x)
    for i in range(groups):
        if n[i] <= 1 or np.isnan(want[i]):
            if not same_bits(got[i], want[i]):
                return i
            continue
        if np.isnan(got[i]):
            return i
        if not np.isfinite(want[i]):
            if got[i] != want[i]:
                return i
            continue
        a = A[i] / n[i]
        if not np.isfinite(a):  # (the squares overflow: the reference's inf - inf; anything but the same class of answer is wrong)
            if np.isfinite(got[i]) != np.isfinite(want[i]):
                return i
            continue
        if abs(np.longdouble(got[i]) ** 2 - np.longdouble(want[i]) ** 2) > np.longdouble(3e-9) * a:
            return i
    return None


def dev_close(got: float, want: float, values: np.ndarray) -> bool:
    """|got^2 - want^2| <= 1e-9 * want^2 + (1e-9 * sum |x| / l)^2; exact when l <= 1"""
    v = values[~is_null(values)]
    if len(v) <= 1 or np.isnan(want):
        return same_bits(np.float64(got), np.float64(want))
    if np.isnan(got):
        return False
    if not np.isfinite(want):
        return got == want
    sabs = np.sum(np.abs(v.astype(np.longdouble)))
    lhs = abs(np.longdouble(got) ** 2 - np.longdouble(want) ** 2)
    return bool(lhs <= np.longdouble(1e-9) * np.longdouble(want) ** 2 + (np.longdouble(1e-9) * sabs / len(v)) ** 2)
