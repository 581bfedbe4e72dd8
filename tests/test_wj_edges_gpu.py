"""The window join's two kernels (rayforce_amd/csrc/rfx_window.hip) at their wave edges, by equality of bits against the numpy restatement
(tests/wj_ref.py; tests/test_wj_cpu.py pins it to the compiled reference's fixture, and pins rows_per_wave, fold_direct and edge_windows).

What the fixture's 4 097 left rows and the two-million-trade test cannot reach: k_window_fold with 2 .. 32 left rows per wave (16 383 .. 524 224 left
rows with one long window on 256 CUs), the wave loop's second trip at 1 and at 64 rows per wave, F64 cells folded by a wave at 64 rows per wave, the
wave-cooperative loop's odd L, single-cell load at the column's last cell and lengths around its 256-cell step, k_window_ranges' counters across its
second grid-stride trip and at a length of exactly 16, rows the fold never stored, aggregates not asked for, the cells beside a window.

  1. the flat fold rfx_exec_window_fold over caller-owned outputs inside sentinel guards;
  2. joins.window_ranges' counters with (li, ri) known in closed form;
  3. Engine.window_join and the operator door at 20 011 .. 300 007 left rows -- the restatement is the reference.
Every test computes and asserts, from its inputs and the device's CU count, the condition that makes it reach its path."""
import ctypes as C

import numpy as np
import pytest
import torch

import wj_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd import joins
from test_wj_cpu import exact_cells
from test_wj_gpu import AGG_NAMES, T_F64, T_I64, agg_dict, case_tables, host_table, raw_cells, window_join

pytestmark = pytest.mark.gpu

RFX_EINVAL = -2
GUARD = 64                     # sentinel cells on either side of every output
SENTINEL = 0x5A5A5A5A5A5A5A5A  # (positive as an i64; 1.5e127 as an f64)
RS = (1, 2, 4, 8, 16, 32, 64)
PINF, NINF = 0x7FF0000000000000, 0xFFF0000000000000


def cus(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def call_fold(eng, vals, li, ri, nlong, aggs=R.AGGS, perm=None):
    """rfx_exec_window_fold the way joins.window_fold calls it, over caller-owned outputs: every output 64 cells inside a tensor prefilled with the
    sentinel; all seven tensors exist, the pointers of `aggs` alone are passed.  -> (rc, the seven tensors as numpy (7, GUARD + n + GUARD))"""
    n = len(li)
    d_li, d_ri = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).to(eng.device) for x in (li, ri))
    whole = torch.full((len(L.RFX_WAGG), GUARD + n + GUARD), SENTINEL, dtype=torch.int64, device=eng.device)
    ptrs = (C.c_void_p * len(L.RFX_WAGG))()
    for a in aggs:
        ptrs[L.RFX_WAGG[a]] = whole[L.RFX_WAGG[a]].data_ptr() + GUARD * 8
    rc = eng.lib.rfx_exec_window_fold(eng._x, vals.data_ptr(), L.RFX_F64 if vals.dtype == torch.float64 else L.RFX_I64, perm.data_ptr() if perm is not None else None,
                                      d_li.data_ptr(), d_ri.data_ptr(), n, vals.numel(), nlong, ptrs)
    eng.sync()
    return rc, whole.cpu().numpy()


def dev_fold(eng, vals, li, ri, nlong, aggs=R.AGGS, perm=None):
    """-> {agg: the n cells as int64 bits}; the guards of every output unchanged, no cell of [0, n) left as it was, the other tensors untouched"""
    n = len(li)
    rc, whole = call_fold(eng, vals, li, ri, nlong, aggs, perm)
    assert rc == L.RFX_OK, (rc, eng.lib.rfx_exec_last_error(eng._x))
    out = {}
    for a, k in L.RFX_WAGG.items():
        if a in aggs:
            assert (whole[k, :GUARD] == SENTINEL).all() and (whole[k, GUARD + n:] == SENTINEL).all(), ("a guard was written", a)
            left = np.flatnonzero(whole[k, GUARD:GUARD + n] == SENTINEL)
            assert left.size == 0, ("rows never stored", a, int(left.size), left[:5], li[left[:5]], ri[left[:5]])
            out[a] = whole[k, GUARD:GUARD + n].copy()
        else:
            assert (whole[k] == SENTINEL).all(), ("an aggregate not asked for was written", a)
    return out


def no_answer_is_the_sentinel(want):
    for a in R.AGGS:
        assert not (bits(want[a]) == SENTINEL).any(), a


def same(got, want, li, ri, what, aggs=R.AGGS):
    for a in aggs:
        w = bits(want[a])
        bad = np.flatnonzero(got[a] != w)
        assert bad.size == 0, (what, a, int(bad.size), bad[:5], li[bad[:5]], ri[bad[:5]], got[a][bad[:5]], w[bad[:5]])


def nlong_of(li, ri):
    return int((np.where(li < 0, 0, ri - li + 1) > R.LANE_MAX).sum())


# ---------------------------------------------------------------------------------------------------- the flat fold
def sizes_at(r, W):
    """the left-row counts of rows-per-wave r: its smallest n (one trip of the wave loop, the last wave holds one row), then two trips: one row below
    that (r / 2 rows per wave, 2 W - 2 waves), at r = 1 half a trip more, at r = 64 also two waves more than a trip"""
    ns = [W * r - r + 1]
    if r >= 2:
        ns.append(W * r - r)
    if r == 1:
        ns.append(W + W // 2 + 1)  # (256 CUs: W + 4 097)
    if r == 64:
        ns.append(64 * W + 65)
    return ns


@pytest.mark.parametrize("nv", [4099, 4100])  # (the column's last cell at an odd and at an even position: the single-cell load, and not)
@pytest.mark.parametrize("dtype", ["i64", "f64"])
@pytest.mark.parametrize("r", RS)
def test_fold_at_every_rows_per_wave(eng, r, dtype, nv):
    ncus = cus(eng)
    W = ncus * 32  # wave slots of the device; the fold's grid holds W waves (cus * 8 blocks of 4), so more than W waves is a second trip
    assert ncus * 8 * 4 == W
    # every launch form is reached on this device: by this case's own sizes the form r, by the parameter list all seven
    assert {R.rows_per_wave(n, ncus, 1) for x in RS for n in sizes_at(x, W)} == set(RS)
    reached = []
    for n in sizes_at(r, W):
        rng = np.random.default_rng(1000 * r + nv + n % 7)
        li, ri, _ = R.edge_windows(nv, n, rng)
        v = exact_cells(dtype, nv, rng)
        nlong = nlong_of(li, ri)
        assert 0 < nlong <= 512, nlong
        rpw = R.rows_per_wave(n, ncus, nlong)
        waves = -(-n // rpw)
        reached.append((rpw, waves > W))
        want = R.window_fold(v, li, ri)
        no_answer_is_the_sentinel(want)
        summed, long_ = bits(want["sum"]) != (R.NAN_BITS if dtype == "f64" else R.NULL), np.where(li < 0, 0, ri - li + 1) > R.LANE_MAX
        assert (summed & long_).sum() >= 10 and (~summed & long_).sum() >= 10  # a wave's windows with a sum, and with a null cell
        vals = eng.column(v)
        assert vals.data_ptr() % 16 == 0
        got = dev_fold(eng, vals, li, ri, nlong)
        same(got, want, li, ri, (r, dtype, nv, n, rpw))
        if dtype == "i64":
            assert np.array_equal(got["sum"], R.sum_by_cumsum(v, li, ri)), (r, nv, n)
    want_reached = {1: [(1, False), (1, True)], 64: [(64, False), (32, True), (64, True)]}.get(r, [(r, False), (r // 2, True)])
    assert reached == want_reached, (r, reached)


def beside_cases(dtype):
    """disjoint windows, one long per parity of L and of R and one short; the cells at L - 1 and R + 1 belong to no window"""
    wins = [(1010, 1300), (2010, 2301), (3011, 3300), (4011, 4301), (5011, 5018)]
    nv = 6001
    rng = np.random.default_rng(5)
    clean = (rng.integers(-(2**22), 2**22, nv) << 40) if dtype == "i64" else rng.integers(-(2**32) + 1, 2**32, nv) * 0.25
    poisoned = clean.copy()
    for a, b in wins:
        clean[[a - 1, b + 1]] = 0
        poisoned[[a - 1, b + 1]] = R.INF - 1 if dtype == "i64" else 1e300
    li, ri = (np.array(x, np.int64) for x in zip(*wins))
    assert {(a % 2, b % 2) for a, b in wins[:4]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return clean, poisoned, li, ri


@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_the_cells_beside_a_window_stay_out(eng, dtype):
    clean, poisoned, li, ri = beside_cases(dtype)
    want = R.fold_direct(clean, li, ri)
    no_answer_is_the_sentinel(want)
    # either neighbour, folded, would change what it can change
    wider_l, wider_r = R.fold_direct(poisoned, li - 1, ri), R.fold_direct(poisoned, li, ri + 1)
    for wider, aggs in ((wider_l, ("sum", "max", "count", "avg", "first")), (wider_r, ("sum", "max", "count", "avg", "last"))):
        for a in aggs:
            assert (bits(wider[a]) != bits(want[a])).all(), a
    same({a: bits(x) for a, x in R.window_fold(poisoned, li, ri).items()}, want, li, ri, "the restatement")
    for nlong in (nlong_of(li, ri), 0):  # one row per wave; all five rows in one wave
        assert (nlong == 4 and R.rows_per_wave(len(li), cus(eng), nlong) == 1) or (nlong == 0 and R.rows_per_wave(len(li), cus(eng), nlong) == 64)
        for v in (poisoned, clean):
            same(dev_fold(eng, eng.column(v), li, ri, nlong), want, li, ri, (dtype, nlong))


@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_every_aggregate_alone_equals_all_together(eng, dtype):
    rng = np.random.default_rng(6)
    nv, n = 1031, 1500
    li, ri, _ = R.edge_windows(nv, n, rng)
    v = exact_cells(dtype, nv, rng)
    vals, nlong = eng.column(v), nlong_of(li, ri)
    together = dev_fold(eng, vals, li, ri, nlong)
    same(together, R.window_fold(v, li, ri), li, ri, dtype)
    for a in R.AGGS:
        alone = dev_fold(eng, vals, li, ri, nlong, aggs=(a,))  # (asserts that the six other tensors keep the sentinel everywhere)
        assert list(alone) == [a] and np.array_equal(alone[a], together[a]), a


def test_f64_special_cells(eng):
    nv = 700
    rng = np.random.default_rng(8)
    b = (rng.integers(-(2**20), 2**20, nv) * 0.25).view(np.uint64)
    b[0:300] = np.uint64(0x7FF8000000000001) + np.arange(300, dtype=np.uint64)  # NaN cells, every payload its own
    b[[7, 38, 299]] = 0xFFF8000000000123, 0xFFF8000000000124, 0xFFF8000000000125   # ... negative ones where windows end
    b[[310, 350]] = PINF, NINF  # 304 .. 399: one of each
    b[[410, 412]] = PINF, NINF  # 404 .. 420: both inside a lane's window
    b[440] = PINF
    b[500:560] = 0x8000000000000000  # -0.0 only
    b[560:620] = 0                   # +0.0 only
    b[620:680:2] = 0x8000000000000000  # both zeros
    b[621:680:2] = 0
    v = b.view(np.float64)
    rows = {"nan_long": (0, 299), "nan_long_odd": (1, 38), "nan_short": (3, 7), "nan_one": (5, 5), "nan_short_neg_first": (7, 12),
            "inf_both_long": (304, 399), "inf_plus_long": (304, 340), "inf_minus_long": (330, 399), "inf_both_short": (408, 414), "inf_plus_short": (436, 442),
            "negzero_long": (500, 559), "negzero_short": (501, 510), "poszero_long": (560, 619), "poszero_short": (561, 570), "zeros_long": (620, 679),
            "zeros_long_odd": (621, 678), "zeros_short": (630, 639), "zeros_short_odd": (631, 640)}
    li, ri = (np.array(x, np.int64) for x in zip(*rows.values()))
    at = {k: i for i, k in enumerate(rows)}
    want = R.fold_direct(v, li, ri)
    no_answer_is_the_sentinel(want)
    mixed = np.array([k.startswith("zeros") for k in rows])
    both_inf = np.array([k.startswith("inf_both") for k in rows])
    # the two restatements agree wherever the answer does not hang on the order: not on which zero a mixed window's min / max is, nor on the sign of
    # the NaN that +inf + -inf gives
    chain = R.window_fold(v, li, ri)
    for a in R.AGGS:
        skip = (mixed if a in ("min", "max") else both_inf if a in ("sum", "avg") else np.zeros(len(li), bool))
        assert np.array_equal(bits(chain[a])[~skip], bits(want[a])[~skip]), a
    for nlong in (nlong_of(li, ri), 0):
        got = dev_fold(eng, eng.column(v), li, ri, nlong)
        u = {a: got[a].view(np.uint64) for a in R.AGGS}
        for k in ("nan_long", "nan_long_odd", "nan_short", "nan_one", "nan_short_neg_first"):
            i, last = at[k], b[rows[k][1]]
            assert u["max"][i] == last and u["first"][i] == last, (k, hex(u["max"][i]), hex(u["first"][i]), hex(last))
            assert u["last"][i] == R.NAN_BITS and u["sum"][i] == R.NAN_BITS and u["avg"][i] == R.NAN_BITS and u["min"][i] == PINF, k
            assert got["count"][i] == rows[k][1] - rows[k][0] + 1
        assert all(got["max"][at[k]] < 0 for k in ("nan_long", "nan_long_odd", "nan_short")) and got["max"][at["nan_one"]] > 0  # negative NaNs, and not
        for k in ("inf_both_long", "inf_both_short"):
            i = at[k]
            assert np.isnan(got["sum"].view(np.float64)[i]) and np.isnan(got["avg"].view(np.float64)[i]), k
            assert u["min"][i] == NINF and u["max"][i] == PINF, k
        for k, inf in (("inf_plus_long", PINF), ("inf_plus_short", PINF), ("inf_minus_long", NINF)):
            assert u["sum"][at[k]] == inf and u["avg"][at[k]] == inf and u["max" if inf == PINF else "min"][at[k]] == inf, k
        for a in R.AGGS:
            skip = (mixed if a in ("min", "max") else both_inf if a in ("sum", "avg") else np.zeros(len(li), bool))
            w = bits(want[a])
            assert np.array_equal(got[a][~skip], w[~skip]), (a, nlong, np.flatnonzero((got[a] != w) & ~skip))
        for k in ("negzero_long", "negzero_short"):
            assert u["min"][at[k]] == 1 << 63 and u["max"][at[k]] == 1 << 63 and u["first"][at[k]] == 1 << 63 and u["sum"][at[k]] == 0, k
        for k in ("poszero_long", "poszero_short"):
            assert u["min"][at[k]] == 0 and u["max"][at[k]] == 0 and u["sum"][at[k]] == 0, k
        # a zero of either sign (the one divergence the kernel's header documents)
        assert ((got["min"][mixed] & R.INF) == 0).all() and ((got["max"][mixed] & R.INF) == 0).all()
        assert u["first"][at["zeros_long"]] == 1 << 63 and u["last"][at["zeros_long"]] == 0 and u["first"][at["zeros_long_odd"]] == 0


def test_inexact_f64_sums_stay_within_the_summation_bound(eng):
    """sum and avg against math.fsum (fold_direct), not against the code under test.  Any order of n - 1 floating-point additions is within
    gamma(n - 1) * sum|x| of the exact sum, gamma(k) = k u / (1 - k u), u = 2^-53: (n - 1) * 2^-53 * sum|x| to first order; the bound here is twice
    that, which also covers the rounding of the reference's own answer (half an ulp, at most 2^-53 * sum|x|).  avg is one more division: the bound
    over n, plus one ulp of the quotient for the two roundings (half an ulp each)."""
    rng = np.random.default_rng(9)
    nv, n = 4100, 1500
    v = (1.0 + rng.random(nv)) * 2.0 ** rng.integers(0, 13, nv)
    li, ri, _ = R.edge_windows(nv, n, rng)
    length = np.where(li < 0, 0, ri - li + 1)
    assert length.max() == nv and (v >= 1).all() and (v < 2**13).all()
    want = R.fold_direct(v, li, ri)
    no_answer_is_the_sentinel(want)
    cs = np.concatenate([[0.0], np.cumsum(v)])
    bound = np.maximum(length - 1, 0) * 2.0**-52 * (cs[np.maximum(ri + 1, 0)] - cs[np.maximum(li, 0)]) * (1 + 2.0**-40)  # (sum|x| itself rounded up)
    assert bound.max() < 1e-4 and (nv - 1) * 2.0**-52 * nv * 2.0**13 < 1e-4  # every cell is >= 1: one dropped or doubled cell lies far outside
    chain = R.window_fold(v, li, ri)
    assert (bits(chain["sum"]) != bits(want["sum"])).any()  # the additions do round: the reference's chain and the exact sum differ somewhere
    for nlong in (nlong_of(li, ri), 0):
        got = dev_fold(eng, eng.column(v), li, ri, nlong)
        same(got, want, li, ri, "inexact", aggs=("count", "min", "max", "first", "last"))
        live = li >= 0
        gs, ga = got["sum"].view(np.float64), got["avg"].view(np.float64)
        assert (bits(want["sum"])[~live] == R.NAN_BITS).all() and (got["sum"][~live] == R.NAN_BITS).all() and (got["avg"][~live] == R.NAN_BITS).all()
        es = np.abs(gs[live] - want["sum"][live])
        assert (es <= bound[live]).all(), (nlong, es.max(), np.flatnonzero(es > bound[live])[:5])
        ea = np.abs(ga[live] - want["avg"][live])
        ba = bound[live] / length[live] + np.spacing(np.maximum(ga[live], want["avg"][live]))
        assert (ea <= ba).all(), (nlong, ea.max(), np.flatnonzero(ea > ba)[:5])
        assert (es[length[live] == 1] == 0).all()


def test_a_value_column_that_is_not_16_byte_aligned(eng):
    rng = np.random.default_rng(10)
    nv, n = 1031, 1500
    li, ri, _ = R.edge_windows(nv, n, rng)
    v = exact_cells("f64", nv, rng)
    nlong = nlong_of(li, ri)
    held = eng.column(np.concatenate([[0.0], v]))
    view = held[1:]
    assert held.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
    rc, whole = call_fold(eng, view, li, ri, nlong)
    assert rc == RFX_EINVAL and (whole == SENTINEL).all()
    assert b"not 16-byte aligned" in eng.lib.rfx_exec_last_error(eng._x)
    want = R.window_fold(v, li, ri)
    ident = torch.arange(nv, dtype=torch.int64, device=eng.device)
    got = dev_fold(eng, view, li, ri, nlong, perm=ident)  # (gathered into a block of the library's own first)
    same(got, want, li, ri, "gathered")
    same(dev_fold(eng, eng.column(v), li, ri, nlong), want, li, ri, "aligned")


# ---------------------------------------------------------------------------------------------------- the ranges kernel's counters
def one_group_ranges(eng, lo, hi, nr, closed, key=0):
    """one key group, rt = arange(nr): with 0 <= lo <= hi < nr both verbs answer (li, ri) = (lo, hi).  -> (li, ri, nlong, longest) after comparing
    li and ri with the restatement's"""
    n = len(lo)
    lk, rk, rt = np.full(n, key, np.int64), np.zeros(nr, np.int64), np.arange(nr, dtype=np.int64)
    left, right = {"k": eng.column(lk)}, {"k": eng.column(rk), "t": eng.column(rt)}
    perm, li, ri, nlong, longest = joins.window_ranges(eng, ["k"], "t", (eng.column(lo), eng.column(hi)), left, right, closed=bool(closed))
    li, ri = li.cpu().numpy(), ri.cpu().numpy()
    wperm, wli, wri = R.window_ranges([lk], [rk], lo, hi, rt, closed)
    assert np.array_equal(perm.cpu().numpy(), wperm) and np.array_equal(li, wli) and np.array_equal(ri, wri), closed
    return li, ri, nlong, longest


def test_ranges_stats_across_trips(eng):
    n = cus(eng) * 8 * 256 + 65  # k_window_ranges' grid is cus * 8 blocks of 256 lanes: a second trip of one whole wave and one lane
    nr = 4100
    rng = np.random.default_rng(12)
    lo = rng.integers(0, nr - 300, n)
    length = rng.integers(1, 17, n)
    length[[0, n - 1, n // 2]] = 16, 16, 16
    for closed in (0, 1):
        for row, want in ((n - 1, (1, 300)), (0, (1, 300)), (None, (0, 16))):
            ln = length.copy()
            if row is not None:
                ln[row] = 300
            li, ri, nlong, longest = one_group_ranges(eng, lo, lo + ln - 1, nr, closed)
            assert np.array_equal(li, lo) and np.array_equal(ri, lo + ln - 1)
            assert (nlong, longest) == want and longest == ln.max(), (closed, row, nlong, longest)


def test_ranges_stats_at_the_lane_limit(eng):
    n, nr = 4097, 4100
    rng = np.random.default_rng(13)
    lo = rng.integers(0, nr - 17, n)
    length = np.where(np.arange(n) % 3 == 0, 17, 16)
    assert (length == 17).sum() == 1366 and length[n - 1] == 16 and length[4095] == 17  # (row 4 096 alone in the last wave)
    for closed in (0, 1):
        li, ri, nlong, longest = one_group_ranges(eng, lo, lo + length - 1, nr, closed)
        assert np.array_equal(ri - li + 1, length)
        assert (nlong, longest) == (1366, 17), (closed, nlong, longest)
        li, ri, nlong, longest = one_group_ranges(eng, lo, lo + 15, nr, closed)  # sixteen cells everywhere: no window is a wave's
        assert (nlong, longest) == (0, 16), (closed, nlong, longest)


def test_all_null_rows(eng):
    n, nr = 65, 4100
    lo = np.arange(n, dtype=np.int64)
    for closed in (0, 1):
        li, ri, nlong, longest = one_group_ranges(eng, lo, lo + 40, nr, closed, key=7)  # (the right table has key 0 only)
        assert (li == -1).all() and (ri == -2).all() and (nlong, longest) == (0, 0), (closed, nlong, longest)


# ---------------------------------------------------------------------------------------------------- Engine and door at the untested sizes
def mid_case(nl):
    """nl trades against 2 nl quotes of 500 symbols (30 more that the quotes lack); 2 500 quotes moved to symbol 0, so that a widened window of it
    holds more than 1 000 cells at every nl; mostly a lane's windows, 3 % ten times as wide, 200 over most of a group; 0.1 % null times and bounds"""
    rng = np.random.default_rng(nl)
    nr, nsym, T = 2 * nl, 500, 10_000_000
    lk, rk = rng.integers(0, nsym + 30, nl), rng.integers(0, nsym, nr)
    rk[rng.choice(nr, 2500, replace=False)] = 0
    lt, rt = rng.integers(0, T, nl), rng.integers(0, T, nr)
    half = int(4 * T * nsym / nr)  # (a window of `half` ticks holds four quotes of a symbol, on average)
    width = np.where(rng.random(nl) < 0.03, 10, 1)
    lo, hi = lt - rng.integers(0, half, nl) * width, lt + rng.integers(0, half, nl) * width
    wide = rng.choice(nl, 200, replace=False)
    lk[wide[:40]] = 0
    lo[wide], hi[wide] = rng.integers(-5, T // 5, 200), rng.integers(4 * T // 5, T + 5, 200)
    vi = rng.integers(-(2**40), 2**40, nr)  # (a group's f64 sum stays below 2^53: avg's chain is exact)
    vi[rng.random(nr) < 0.02] = R.NULL
    vf = rng.integers(-(2**32) + 1, 2**32, nr) * 0.25
    vf[rng.random(nr) < 0.02] = np.nan
    for a in (lo, hi, rt):
        a[rng.random(len(a)) < 0.001] = R.NULL32
    return dict(name=f"mid_{nl}", nk=1, kinds=["i64"], lk=[lk], rk=[rk], lt=lt, lo=lo, hi=hi, rt=rt, vi=vi, vf=vf)


def mid_reach(c, closed, ncus, want):
    _, li, ri = R.window_ranges(c["lk"], c["rk"], c["lo"], c["hi"], c["rt"], closed)
    nlong = nlong_of(li, ri)
    rpw = R.rows_per_wave(len(li), ncus, nlong)
    assert nlong > 0 and rpw not in (1, 64), (c["name"], rpw)
    if ncus == 256:
        assert rpw == {20_011: 2, 40_009: 4, 100_003: 8, 300_007: 32}[len(li)]
    counts = bits(want[("count", "vi")])
    assert (counts == 0).any() and (counts > 1000).any() and ((counts > 0) & (counts <= 16)).any() and ((counts > 16) & (counts < 200)).any()
    assert np.array_equal(counts, np.where(li < 0, 0, ri - li + 1))


@pytest.mark.parametrize("nl", [20_011, 100_003, 300_007])
def test_window_join_at_mid_sizes(eng, nl):
    c = mid_case(nl)
    left = {"k0": eng.column(c["lk"][0]), "t": eng.column(c["lt"])}
    right = {"k0": eng.column(c["rk"][0]), "t": eng.column(R.widen(c["rt"])), "vi": eng.column(c["vi"]), "vf": eng.column(c["vf"])}
    windows = (eng.column(R.widen(c["lo"])), eng.column(R.widen(c["hi"])))
    for closed in (0, 1):
        want = R.window_join(c["lk"], c["rk"], c["lo"], c["hi"], c["rt"], closed, {"vi": c["vi"], "vf": c["vf"]})
        mid_reach(c, closed, cus(eng), want)
        got = eng.window_join(["k0", "t"], windows, left, right, AGG_NAMES, closed=bool(closed))
        assert list(got) == ["k0", "t"] + list(AGG_NAMES)
        for name, (a, col) in AGG_NAMES.items():
            g = got[name].cpu().numpy()
            assert g.dtype == (np.int64 if a == "count" or (col == "vi" and a != "avg") else np.float64), name
            bad = np.flatnonzero(bits(g) != want[(a, col)])
            assert bad.size == 0, (nl, closed, name, int(bad.size), bad[:5], bits(g)[bad[:5]], want[(a, col)][bad[:5]])


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0
    return o


def test_a_mid_size_join_through_the_door(ops):
    nl = 40_009
    c = mid_case(nl)
    ncus = torch.cuda.get_device_properties(0).multi_processor_count
    for closed in (0, 1):
        want = R.window_join(c["lk"], c["rk"], c["lo"], c["hi"], c["rt"], closed, {"vi": c["vi"], "vf": c["vf"]})
        mid_reach(c, closed, ncus, want)
        names, left, right, wins = case_tables(ops, c, None)
        lt, rt = host_table(ops, left), host_table(ops, right)
        d = agg_dict(ops, AGG_NAMES, by_name=bool(closed))
        st0 = H.to_numpy(ops.rfx_stats(None))
        r, ks = window_join(ops, closed, names + ["t"], wins, lt, rt, d)
        st1 = H.to_numpy(ops.rfx_stats(None))
        try:
            assert not H.is_error(r), H.error_text(r)
            assert H.header(r).type == H.T_TABLE and ops.rfx_last_window_on_gpu() == 1
            assert st1[2] - st0[2] == 1 and st1[3] - st0[3] == 0  # ST_JOIN_GPU / ST_JOIN_DELEGATED
            rk, rv = H.list_items(r)
            assert [ops.rfx_host_symbol_name(int(s)).decode() for s in raw_cells(rk)] == list(left) + list(AGG_NAMES)
            cols = H.list_items(rv)
            for (n, (cells, t)), o in zip(left.items(), cols):
                assert H.header(o).type == t and np.array_equal(raw_cells(o), cells), n
            for (name, (a, col)), o in zip(AGG_NAMES.items(), cols[len(left):]):
                assert H.header(o).type == (T_I64 if a == "count" or (col == "vi" and a != "avg") else T_F64) and H.header(o).len == nl, name
                got = raw_cells(o)
                bad = np.flatnonzero(got != want[(a, col)])
                assert bad.size == 0, (closed, name, int(bad.size), bad[:5], got[bad[:5]], want[(a, col)][bad[:5]])
        finally:
            for o in (r, ks, wins, lt, rt, d):
                ops.rfx_host_drop(o)
