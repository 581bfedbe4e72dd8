"""window-join / window-join1 restated in numpy (core/join.c:358-489, core/index.c:3269-3347, the INDEX_TYPE_WINDOW arms of core/aggr.c): what
tests/golden/wj_golden.npz pins bit for bit, and the yardstick of the GPU tests beyond the fixture's sizes.

The right table is ordered by (key tuple, time), stably; a left row's tuple has the run [fi, ti] there; the reference's two binary searches over the
run's 32-bit times (core/aggr.c:39-71, both answering the run's first row when nothing qualifies) give li and ri, its two tests the null rows, and
every aggregate folds rows li .. ri IN ORDER.  The folds below replay that order cell by cell (vectorised over the left rows, one step per position
of the window), with the reference's own null rules (core/ops.h:154-187), so F64 sums round as the reference's do."""
import numpy as np

NULL = -(2**63)
NULL32 = -(2**31)
INF = 2**63 - 1
NAN_BITS = 0x7FF8000000000000
AGGS = ("sum", "min", "max", "count", "avg", "first", "last")


def widen(a):
    """4-byte cells kept in int64 (sign-extended) -> the 8-byte device cells: NULL_I32 becomes NULL_I64 (core/ops.h:240)"""
    a = np.asarray(a, np.int64)
    return np.where(a == NULL32, NULL, a)


def narrow(a):
    """... and back: what the reference's AS_I32 reads"""
    a = np.asarray(a, np.int64)
    return np.where(a == NULL, NULL32, a)


def group_ids(lk, rk):
    """one id per key tuple over both sides (cells compare as raw integers: null equals null)"""
    nl = len(lk[0])
    both = [np.concatenate([np.asarray(l, np.int64), np.asarray(r, np.int64)]) for l, r in zip(lk, rk)]
    if len(both) == 1:
        _, inv = np.unique(both[0], return_inverse=True)
    else:
        _, inv = np.unique(np.stack(both, axis=1), axis=0, return_inverse=True)
    inv = np.asarray(inv, np.int64).reshape(-1)
    return inv[:nl], inv[nl:]


def window_ranges(lk, rk, lo, hi, rt, closed):
    """(perm, li, ri): the right rows by (tuple, time), stable; per left row its window's first and last position there, (-1, -2) for a null row.
    lo, hi, rt: 32-bit values in int64 cells (a null as NULL32 or NULL)."""
    lo, hi, rt = narrow(lo), narrow(hi), narrow(rt)
    nl, nr = len(lo), len(rt)
    li, ri = np.full(nl, -1, np.int64), np.full(nl, -2, np.int64)
    if nr == 0 or nl == 0:
        return np.arange(nr, dtype=np.int64), li, ri
    gl, gr = group_ids(lk, rk)
    comp = lambda g, t: (g << 32) | (t - NULL32)
    cr = comp(gr, rt)
    perm = np.argsort(cr, kind="stable")
    C, G, T = cr[perm], gr[perm], rt[perm]
    fi, end = np.searchsorted(G, gl, "left"), np.searchsorted(G, gl, "right")
    has = end > fi
    r = np.searchsorted(C, comp(gl, hi), "right") - 1
    r = np.where(r < fi, fi, r)  # (nothing <= hi: idx stays 0)
    if closed:
        l = np.searchsorted(C, comp(gl, lo), "left")
        l = np.where(l >= end, fi, l)  # (nothing >= lo: idx stays 0)
    else:
        l = np.searchsorted(C, comp(gl, lo), "right") - 1
        l = np.where(l < fi, fi, l)
    l, r = np.where(has, l, 0), np.where(has, r, 0)
    null = ~has | (T[l] > hi)
    if closed:
        null |= T[r] < lo
    return perm, np.where(null, -1, l), np.where(null, -2, r)


def window_fold(v, li, ri, aggs=AGGS):
    """v: the value column in the sorted order (int64 cells, or float64); -> {agg: cells} with F64 answers as float64"""
    f64 = v.dtype == np.float64
    n = len(li)
    isnull = (lambda x: np.isnan(x)) if f64 else (lambda x: x == NULL)
    nullv = np.float64(np.nan) if f64 else np.int64(NULL)
    length = np.where(li < 0, 0, ri - li + 1)
    order = np.argsort(-length, kind="stable")
    L, start = length[order], li[order]
    asc = L[::-1]
    dt = v.dtype
    s = np.zeros(n, dt)
    mn = np.full(n, np.inf if f64 else INF, dt)
    mx = np.full(n, nullv, dt)
    first, last = np.full(n, nullv, dt), np.full(n, nullv, dt)
    fsum, cnt = np.zeros(n, np.float64), np.zeros(n, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(int(L[0]) if n else 0):
            m = n - int(np.searchsorted(asc, k, "right"))  # rows whose window has a position k
            x = v[start[:m] + k]
            xn = isnull(x)
            a = s[:m]
            s[:m] = np.where(isnull(a) | xn, nullv, a + x)  # ADDI64 / ADDF64
            a = mn[:m]
            mn[:m] = np.where(isnull(a), x, np.where(xn, a, np.where(a < x, a, x)))  # MINI64 / MINF64
            a = mx[:m]
            mx[:m] = np.where(isnull(a), x, np.where(xn, a, np.where(a > x, a, x)))  # MAXI64 / MAXF64
            fsum[:m] = np.where(xn, fsum[:m], fsum[:m] + np.where(xn, 0, x).astype(np.float64))
            cnt[:m] += ~xn
            a = first[:m]
            first[:m] = np.where(isnull(a), x, a)
            last[:m] = np.where(xn, last[:m], x)
    rownull = (li < 0)[order]
    with np.errstate(invalid="ignore", divide="ignore"):
        res = {"sum": np.where(rownull, nullv, s), "min": np.where(rownull, nullv, mn), "max": np.where(rownull, nullv, mx), "count": L.astype(np.int64),
               "avg": np.where(rownull | (cnt == 0), np.nan, fsum / np.where(cnt == 0, 1, cnt)), "first": np.where(rownull, nullv, first),
               "last": np.where(rownull, nullv, last)}
    back = np.empty(n, np.int64)
    back[order] = np.arange(n)
    return {a: res[a][back] for a in aggs}


def window_join(lk, rk, lo, hi, rt, closed, cols, aggs=AGGS):
    """cols: {name: right column}; -> {(agg, name): cells as int64 BITS}"""
    perm, li, ri = window_ranges(lk, rk, lo, hi, rt, closed)
    out = {}
    for name, v in cols.items():
        for a, cells in window_fold(np.asarray(v)[perm], li, ri, aggs).items():
            out[(a, name)] = np.ascontiguousarray(cells).view(np.int64)
    return out


# ---------------------------------------------------------------------------------------------------- the fixture (tests/golden/wj_golden.npz)
def unplanes(p):
    """eight byte planes (uint8, shape (8, cells)) -> the int64 cells"""
    return np.ascontiguousarray(p.T).view(np.int64).reshape(-1)


def load_case(gold, ci):
    """-> dict: name, nk, kinds (per key "i64" / "sym"), threads, lk, rk, lt, lo, hi, rt (int64 cells holding 32-bit values), vi, vf (float64),
    out[verb][column][aggregate] = the reference's cells as int64 bits"""
    name, nk, kind, threads = str(gold["cases"][ci]).split("|")
    nk = int(nk)
    c = {"name": name, "nk": nk, "threads": threads, "kinds": {"i64": ["i64"] * nk, "sym": ["sym"] * nk, "sym+i64": ["sym"] + ["i64"] * (nk - 1)}[kind]}
    for side in "lr":
        c[side + "k"] = [unplanes(gold[f"c{ci}_{side}k{j}"]) for j in range(nk)]
    for n in ("lt", "lo", "hi", "rt", "vi"):
        c[n] = unplanes(gold[f"c{ci}_{n}"])
    c["vf"] = unplanes(gold[f"c{ci}_vf"]).view(np.float64)
    nl = len(c["lt"])
    out = unplanes(gold[f"c{ci}_out"]).reshape(2, 2, len(AGGS), nl)
    c["out"] = [{col: {a: out[w, x, k] for k, a in enumerate(AGGS)} for x, col in enumerate(("vi", "vf"))} for w in (0, 1)]
    return c


# ---------------------------------------------------------------------------------------------------- the fold's launch, and windows at its edges
WAVE, LANE_MAX = 64, 16  # RFX_WAVE, RFX_WINDOW_LANE_MAX (rayforce_amd/csrc/rfx_window.hip)
EDGE_LENGTHS = (1, 2, 15, 16, 17, 18, 127, 128, 129, 255, 256, 257, 258, 259, 511, 512, 513)


def rows_per_wave(n, cus, long_windows):
    """rfx_hip_window_fold's rule: 64 left rows per wave while every window is a lane's; with long windows as few as it takes to give each of the
    device's cus * 32 wave slots a wave"""
    rpw = WAVE
    if long_windows > 0:
        while rpw > 1 and (n + rpw - 1) // rpw < cus * 32:
            rpw >>= 1
    return rpw


def n_lo(r, cus):
    """the smallest n that runs with r rows per wave (r = 1: the largest); one row less runs with r / 2"""
    return cus * 32 * r - r + 1


def sum_by_cumsum(v, li, ri):
    """I64 sums a second way: the difference of two wrapping prefix sums, null where the window holds a null cell or is the null row"""
    v = np.asarray(v, np.int64)
    isn = v == NULL
    with np.errstate(over="ignore"):
        cs = np.concatenate([[0], np.cumsum(np.where(isn, 0, v), dtype=np.int64)])
        cn = np.concatenate([[0], np.cumsum(isn)])
        a, b = np.maximum(li, 0), np.maximum(ri + 1, 0)
        return np.where((li < 0) | (cn[b] - cn[a] > 0), NULL, cs[b] - cs[a])


def fold_direct(v, li, ri):
    """every aggregate of every row from the slice v[li : ri + 1] alone, by the reference's rules stated per window (no code shared with
    window_fold): count is the window's length; sum is null when a cell is; min over null cells only is INF_I64 / +inf; max and first of an F64
    window of NaN cells only are the LAST cell's own NaN, last of it the canonical null.  I64 sums wrap; F64 sums, and the f64 sum behind avg, are
    math.fsum: the exactly rounded sum, which every order of addition gives where the additions are exact.  -> {agg: cells}, as window_fold"""
    import math
    f64 = v.dtype == np.float64
    n = len(li)
    nullb = NAN_BITS if f64 else NULL & (2**64 - 1)
    bits = v.view(np.uint64)
    out = {a: np.full(n, nullb, np.uint64) for a in AGGS if a not in ("count", "avg")}
    cnt, avg = np.zeros(n, np.int64), np.full(n, np.nan)
    for i in range(n):
        if li[i] < 0:
            continue
        w, wb = v[li[i]:ri[i] + 1], bits[li[i]:ri[i] + 1]
        cnt[i] = len(w)
        ok = ~np.isnan(w) if f64 else w != NULL
        cells, cb = w[ok], wb[ok]
        if len(cells) == 0:
            out["min"][i] = np.array([np.inf]).view(np.uint64)[0] if f64 else INF
            if f64:
                out["max"][i] = out["first"][i] = wb[-1]
            continue
        try:
            fs = math.fsum(float(x) for x in cells) + 0.0  # (the reference's chain starts at +0.0: cells of -0.0 only sum to +0.0)
        except (ValueError, OverflowError):  # (+inf and -inf in one window)
            fs = math.nan
        avg[i] = fs / len(cells) if fs == fs else math.nan
        if len(cells) == len(w):
            out["sum"][i] = np.array([fs]).view(np.uint64)[0] if f64 else sum(int(x) for x in cells) & (2**64 - 1)
        out["min"][i], out["max"][i] = cb[np.argmin(cells)], cb[np.argmax(cells)]
        out["first"][i], out["last"][i] = cb[0], cb[-1]
    res = {a: c.view(v.dtype) for a, c in out.items()}
    res["count"], res["avg"] = cnt, avg
    return {a: res[a] for a in AGGS}


def edge_windows(nv, n, rng):
    """(li, ri, info): n windows over a column of nv cells, every position valid (0 <= li <= ri < nv, or (-1, -2)), at most 512 of them longer than
    a lane's 16 cells.  Four blocks of 64 consecutive rows at multiples of 64 -- all long; only the first row long; only the last; all null -- and,
    shuffled over the other rows (info["shuffle"]: the row of each window of the fixed order), every L in 0 .. 3 and every L with R == nv - 1
    crossed with EDGE_LENGTHS and nv - L, then 10 % null rows and windows of 1 .. 16 cells at a random L"""
    assert nv >= 600 and n >= 16 * WAVE
    edge = []
    for length in EDGE_LENGTHS:
        edge += [(L, L + length - 1) for L in (0, 1, 2, 3)] + [(nv - length, nv - 1)]
    edge += [(L, nv - 1) for L in (0, 1, 2, 3)]
    blocks = {"all_long": 2 * WAVE, "lane0_long": 5 * WAVE, "lane63_long": 9 * WAVE, "all_null": 12 * WAVE}
    nrest = n - 4 * WAVE
    assert nrest >= len(edge)

    def short(m):
        length = rng.integers(1, LANE_MAX + 1, m)
        L = rng.integers(0, nv - LANE_MAX, m)
        return L, L + length - 1

    def long_(m):
        length = rng.integers(LANE_MAX + 1, 600, m)
        L = rng.integers(0, nv - 600, m)
        return L, L + length - 1

    fl, fr = short(nrest)
    null = rng.random(nrest) < 0.1
    fl[null], fr[null] = -1, -2
    fl[:len(edge)], fr[:len(edge)] = np.array(edge, np.int64).T
    shuffle = rng.permutation(nrest)
    li, ri = np.empty(n, np.int64), np.empty(n, np.int64)
    free = np.ones(n, bool)
    for at in blocks.values():
        free[at:at + WAVE] = False
    rows = np.flatnonzero(free)[shuffle]
    li[rows], ri[rows] = fl, fr
    at = blocks["all_long"]
    li[at:at + WAVE], ri[at:at + WAVE] = long_(WAVE)
    for name, lane in (("lane0_long", 0), ("lane63_long", WAVE - 1)):
        at = blocks[name]
        li[at:at + WAVE], ri[at:at + WAVE] = short(WAVE)
        li[at + lane], ri[at + lane] = (x[0] for x in long_(1))
    at = blocks["all_null"]
    li[at:at + WAVE], ri[at:at + WAVE] = -1, -2
    length = np.where(li < 0, 0, ri - li + 1)
    assert (((li >= 0) & (li <= ri) & (ri < nv)) | ((li == -1) & (ri == -2))).all() and 0 < int((length > LANE_MAX).sum()) <= 512
    return li, ri, {"shuffle": rows, "blocks": blocks, "edge": edge}
