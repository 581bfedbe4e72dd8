"""The plane group-by kernels (rayforce_amd/csrc/rfx_group_plane.hip: k_plane_scatter, k_plane_aggregate, k_plane_hash_aggregate) at their block,
region and LDS edges, every answer against the oracle.

What the small tests of test_gpu_parity.py cannot reach: their 3e5..9e5 rows are 2..4 row blocks of 2^18 rows, so a wave of the aggregate owns at most one
region -- the walk `b = q + r * Q`, the refill of the 64-entry count window at `(r & 63) == 0`, empty regions in mid-walk and first rows rebuilt as
`block * block_rows + delta` run at about 1e9 rows only.  RFX_PLANE_BLOCK_ROWS (host code, read once per process) makes the blocks small: a few million rows
then have the block structure of the headline benchmark.  Settings that are read once per process run in a child process per setting (`_child`).

Every query goes through Engine.select.  A table comes in two kinds: "real" (f64 cells in [0, 1)), compared by check_select of test_gpu_parity.py -- integers,
keys, group order and first rows bit for bit, f64 sums and averages within 1e-9 of the group's sum of magnitudes -- and "exact": integer-valued f64 cells with
|x| < 2^20, whose sums are exact in any order (4.5e6 rows x 2^20 < 2^53), so the f64 results are compared bit for bit as well: a dropped or doubled record fails
whatever its value.  Every case asserts the path counters: RFX_STAT_PLANE_SCATTER (0) and _AGGREGATE (2) moved, _FALLBACK (1) and the chunk kernels (3, 4) did
not -- a case that expects something else says so."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import rfo
from test_gpu_parity import CHUNK_SMALL, NULL, check_select, dev

pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = 2**63 - 1, -(2**63)
BLOCK = 1 << 18            # PL_BLOCK_ROWS
LDS_MAX = 150 * 1024       # PL_AGG_LDS_MAX
WINDOWS = 16 * 64 * 4 + 64  # the waves' count windows behind the tables (plane_agg_lds)


# ---------------------------------------------------------------- the host code's arithmetic, restated
def agg_lds(local, n8, n4):
    """plane_agg_lds: `local` table cells per partition, n8 accumulators of 8 bytes, n4 arrays of 4 bytes (the first rows + one per avg / i64 sum)."""
    return local * (8 * n8 + 4 * n4) + WINDOWS


def region_records(block_rows, pbits, frac=None):
    """c0 of rfx_plane_scope: the expected share of a partition, a quarter more, 160 for its spread, rounded up to whole 128 records."""
    share = block_rows / (1 << pbits)
    if frac is not None:
        share *= min(frac * 1.3 + 0.01, 1.0)
    return (int(share * 1.25 + 160.0) + 127) & ~127


def wave_strides(threads, cus, split_env=0):
    """Q of k_plane_aggregate = split x waves per workgroup, as rfx_plane_accumulate sets the split at 128 partitions and at most 4e7 selected rows: the
    1024-lane form one workgroup a partition (or RFX_PLANE_AGG_SPLIT); the 512-lane form 1..4 workgroups a CU by the size of its tables -- every Q it can take."""
    if threads == 1024:
        return [16 * (split_env if split_env >= 1 else 1)]
    return sorted({8 * max((per_cu * cus + 127) // 128, 1) for per_cu in (1, 2, 3, 4)})


# ---------------------------------------------------------------- tables and checks
def f64_col(n, seed, kind):
    if kind == "exact":  # integers in (-2^20, 2^20): every partial sum of 4.5e6 of them is exact
        return (rfo.gen_i64(n, seed, 2**21 - 1) - (2**20 - 1)).astype(np.float64)
    return rfo.gen_f64(n, seed)


def cut(frac, kind):
    """the value below which `frac` of an f64 column lies"""
    return float(int((2 * frac - 1) * 2**20)) if kind == "exact" else frac


def mk(n, keys, kind, seed=0):
    return {"k": keys, "a": rfo.gen_i64(n, 2 + seed, 1_000_000), "r": np.arange(n, dtype=np.int64), "v": f64_col(n, 5 + seed, kind), "w": f64_col(n, 6 + seed, kind),
            "u": f64_col(n, 7 + seed, kind)}


def stats(eng):
    return [eng.stat(i) for i in range(5)]


def check_exact(eng, host, q, devt=None):
    """check_select with no tolerance: the f64 outputs bit for bit too (for the "exact" tables)."""
    got = eng.select({"from": dev(eng, host) if devt is None else devt, **q})
    want = rfo.select({"from": host, **q})
    assert list(got.keys()) == list(want.keys())
    for name in want:
        g, w = got[name].cpu().numpy(), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
        assert bad.size == 0, (name, int(bad.size), int(bad[0]), g[bad[0]], w[bad[0]])
    return got


def run(eng, host, q, kind, expect="planes", passes=None, devt=None):
    """One query, checked; the path counters moved as `expect` says: "planes" (one scatter, `passes` aggregate launches -- None: at least one -- nothing else),
    "overflow" (the scatter gave up: counter 1 moved by one, no aggregate launch), "handed_back" (the scatter ran, no aggregate launch, no overflow),
    "declined" (no plane aggregate)."""
    s0 = stats(eng)
    (check_exact if kind == "exact" else check_select)(eng, host, q, devt)
    s1 = stats(eng)
    d = [b - a for a, b in zip(s0, s1)]
    if expect == "planes":
        assert d[0] == 1 and (d[2] >= 1 if passes is None else d[2] == passes) and d[1] == 0 and d[3] == 0 and d[4] == 0, (q, d)
    elif expect == "overflow":
        assert d[0] == 1 and d[1] == 1 and d[2] == 0, (q, d)
    elif expect == "handed_back":
        assert d[0] == 1 and d[1] == 0 and d[2] == 0, (q, d)
    else:
        assert expect == "declined" and d[2] == 0, (q, d)


@pytest.fixture()
def small(eng):
    eng.tune(flags=CHUNK_SMALL)
    yield eng
    eng.tune(flags=0)


# ---------------------------------------------------------------- 1. instantiation matrix, default block size
N50, N600 = 700_001, 900_001  # 2 blocks + 175 713 rows (a ragged step of 97), 3 blocks + 113 569 rows (a ragged step of 417)


@pytest.fixture(scope="module")
def t50():
    """50 000 keys: 391 cells per partition, every table set far below 52 KB -- the 512-lane aggregate"""
    return {kind: mk(N50, rfo.gen_i64(N50, 4, 50_000) + 77, kind) for kind in ("real", "exact")}


@pytest.fixture(scope="module")
def t600():
    """600 000 keys: local = ceil(600 000 / 128) = 4 688 cells per partition -- beyond 52 KB from 12 bytes a cell on: the 1024-lane aggregate"""
    return {kind: mk(N600, rfo.gen_i64(N600, 4, 600_000) + 77, kind) for kind in ("real", "exact")}


SCATTER_ARMS = [  # (k_plane_scatter<NC, NP, NV, 7, VGL>, where, aggregates)
    ("2,0,1,7,5", None, {"s": ("sum", "v")}),
    ("2,1,1,7,5", lambda c: ("<", "v", c(0.8)), {"s": ("sum", "v")}),
    ("2,3,1,7,5", lambda c: ("and", ("<", "v", c(0.9)), (">", "v", c(0.05)), ("!=", "k", 1077)), {"s": ("sum", "v")}),
    ("2,8,1,7,5", lambda c: ("and", ("<", "v", c(0.95)), (">", "v", c(0.02)), ("!=", "k", 1077), ("!=", "k", 1078), (">=", "k", 80)), {"s": ("sum", "v")}),
    ("3,1,1,7,5", lambda c: ("<", "a", 800_000), {"s": ("sum", "v")}),
    ("4,3,1,7,5", lambda c: ("and", ("<", "a", 900_000), ("<", "w", c(0.9))), {"s": ("sum", "v")}),
    ("3,0,2,7,4", None, {"s1": ("sum", "v"), "s2": ("sum", "w")}),
    ("4,1,2,7,4", lambda c: ("<", "a", 800_000), {"s1": ("sum", "v"), "s2": ("sum", "w")}),
    ("4,0,3,7,4", None, {"s1": ("sum", "v"), "s2": ("sum", "w"), "s3": ("sum", "u")}),
    ("5,1,3,7,4", lambda c: ("<", "a", 800_000), {"s1": ("sum", "v"), "s2": ("sum", "w"), "s3": ("sum", "u")}),
]


@pytest.mark.parametrize("arm,where,aggs", SCATTER_ARMS, ids=[a[0] for a in SCATTER_ARMS])
def test_scatter_arms(small, t50, arm, where, aggs):
    """One case per reachable <NC, NP, NV, 7, VGL>: 0 / 1 / 3 / 5 predicates on key and value only (no extra column), predicates on one and on two other
    columns, one to three value planes.  (Every selection keeps far more rows than the 50 000 keys span: dense.)"""
    for kind in ("real", "exact"):
        q = dict(by="k", **aggs)
        if where is not None:
            q["where"] = where(lambda f: cut(f, kind))
        run(small, t50[kind], q, kind, passes=1)


AGG_ARMS = [  # (k_plane_aggregate<T, NVL, FAST>, table, aggregates, passes, the LDS arithmetic)
    ("512,1,true", "t50", {"s": ("sum", "v")}, 1),                                          # 391 x (8 + 4) + 4160 = 8 852
    ("1024,1,true", "t600", {"s": ("sum", "v")}, 1),                                        # 4688 x 12 + 4160 = 60 416 > 53 248
    ("512,1,false", "t50", {"av": ("avg", "v"), "f": ("first", "r")}, 1),                   # 391 x (16 + 8) + 4160 = 13 544
    ("1024,1,false", "t600", {"av": ("avg", "v")}, 1),                                      # 4688 x (8 + 8) + 4160 = 79 168
    ("512,2,false", "t50", {"s1": ("sum", "v"), "mx": ("max", "w")}, 1),                    # 391 x (16 + 4) + 4160 = 11 980
    ("1024,2,false", "t600", {"s1": ("sum", "v"), "s2": ("sum", "w")}, 1),                  # 4688 x 20 + 4160 = 97 920
    ("512,3,false", "t50", {"s1": ("sum", "v"), "mn": ("min", "w"), "a3": ("avg", "u")}, 1),  # 391 x (24 + 8) + 4160 = 16 672
    ("1024,3,false", "t600", {"s1": ("sum", "v"), "s2": ("sum", "w"), "s3": ("sum", "u")}, 1),  # 4688 x 28 + 4160 = 135 424 <= 153 600
    # two passes, the second one COUNT / FIRST only (it loads plane 0 to keep its loads uniform): avg v + avg w = 4688 x (16 + 12) + 4160 = 135 424 fits,
    # + count = 4688 x 36 + 4160 = 172 928 does not; count + first = 4688 x (16 + 4) + 4160 = 97 920: <1024, 2, false> then <1024, 1, false>.
    # (A plan of COUNT / FIRST alone has no value plane: rfx_plane_scope declines it -- see test_count_first_only_plan.)
    ("1024,2,false+1024,1,false", "t600", {"a1": ("avg", "v"), "a2": ("avg", "w"), "c": ("count", "a"), "f": ("first", "r")}, 2),
]


@pytest.mark.parametrize("arm,table,aggs,passes", AGG_ARMS, ids=[a[0] for a in AGG_ARMS])
def test_aggregate_arms(small, t50, t600, arm, table, aggs, passes):
    """One case per k_plane_aggregate<512 | 1024, NVL, FAST>; which side of 52 KB a case falls on is plane_agg_lds, restated and asserted."""
    host = {"t50": t50, "t600": t600}[table]
    local = (int(host["real"]["k"].max() - host["real"]["k"].min()) + 1 + 127) >> 7
    assert (agg_lds(local, 1, 1) > 52 * 1024) == arm.startswith("1024") and local + local // 16 <= 1 << 14
    for kind in ("real", "exact"):
        run(small, host[kind], dict(by="k", **aggs), kind, passes=passes)


def test_count_first_only_plan(small, t50):
    """COUNT / FIRST alone read no value column: the planes have nothing to carry and decline before the scatter (nv < 1 in rfx_plane_scope); the chunk
    kernels answer.  Stated expectation: no plane launch at all."""
    s0 = stats(small)
    check_select(small, t50["real"], {"by": "k", "c": ("count", "a"), "f": ("first", "r")})
    s1 = stats(small)
    assert s1[0] == s0[0] and s1[2] == s0[2], (s0, s1)


N256 = 2_400_011


@pytest.fixture(scope="module")
def t256():
    """Key ranges whose tables at 128 partitions no longer fit: l7 = range / 128, and l7 + l7 / 16 cells must fit PL_AGG_LDS_MAX.
    avg over 1.3e6 keys: l7 = 10 157, (10 157 + 634) x 16 + 4160 = 176 816 > 153 600 -> 256 partitions, 5 079 cells x 16 + 4160 = 85 424.
    sum f64 over 1.7e6 keys: l7 = 13 282, (13 282 + 830) x 12 + 4160 = 173 504 > 153 600 -> 256 partitions, 6 641 x 12 + 4160 = 83 852.
    The planner calls a key dense when its range is at most the SELECTED rows: 2.4e6 rows, of which the filter below keeps 80 % = 1.92e6 >= 1.7e6."""
    out = {}
    for kind in ("real", "exact"):
        t = mk(N256, rfo.gen_i64(N256, 4, 1_300_000) - 333, kind)
        t["k17"] = rfo.gen_i64(N256, 14, 1_700_000) + 12_345
        out[kind] = t
    return out


@pytest.mark.parametrize("key,aggs", [("k", {"av": ("avg", "v")}), ("k17", {"s": ("sum", "v")})], ids=["avg_1.3e6", "sum_1.7e6"])
@pytest.mark.parametrize("filtered", [False, True])
def test_256_partition_dense_form(small, t256, key, aggs, filtered):
    """k_plane_scatter<*, *, 1, 8, 4>: 16-record groups, 256 partitions; without a filter and with one that keeps 80 % (a selective one would make the
    range look sparse)."""
    rng = int(t256["real"][key].max() - t256["real"][key].min()) + 1
    n8, n4 = 1, (2 if "av" in aggs else 1)
    l7 = (rng + 127) >> 7
    assert agg_lds(l7 + l7 // 16, n8, n4) > LDS_MAX and agg_lds((rng + 255) >> 8, n8, n4) <= LDS_MAX
    for kind in ("real", "exact"):
        q = dict(by=key, **aggs)
        if filtered:
            q["where"] = ("<", "a", 800_000)
        run(small, t256[kind], q, kind, passes=1)


# ---------------------------------------------------------------- 2. region limits
def region_table(n, in5, kind):
    """Block 0 (the first 2^18 rows): exactly `in5` rows in partition 5 (key & 127), the other 127 partitions share the rest evenly; rows in a fixed
    shuffled order.  1 500 cells per partition: the 512-lane aggregate.  Behind block 0: uniform keys."""
    part = np.empty(BLOCK, np.int64)
    part[:in5] = 5
    others = np.array([p for p in range(128) if p != 5], np.int64)
    part[in5:] = others[np.arange(BLOCK - in5) % 127]
    part = part[np.random.default_rng(20).permutation(BLOCK)]
    k = np.concatenate([part + 128 * rfo.gen_i64(BLOCK, 21, 1500), rfo.gen_i64(n - BLOCK, 22, 128 * 1500)])
    assert int((k[:BLOCK] & 127 == 5).sum()) == in5
    return mk(n, k, kind)


@pytest.mark.parametrize("in5,expect", [(2816, "planes"), (2817, "overflow"), (2784, "planes"), (2783, "planes")])
def test_region_filled_to_its_last_record(small, in5, expect):
    """Unfiltered, 128 partitions, blocks of 2^18 rows: a region holds c0 = 2816 records (2048 x 1.25 + 160 = 2720, rounded up to 128).  A region filled
    to exactly c0 is answered by the planes (`seq >= c0` in the scatter, the `c0 - 2` clamp of the aggregate's loads); one record more and the scatter says
    so -- counter 1 moves by one, no aggregate launch, the chunk kernels answer the same.  2784 = 87 x 32 and 2783: the last group's flush with and without
    a partly filled group."""
    c0 = region_records(BLOCK, 7)
    assert c0 == 2816 and (2816 if expect == "planes" else 2817) >= in5 > c0 - 64
    n = 300_007
    for kind in ("exact", "real"):
        host = region_table(n, in5, kind)
        run(small, host, {"by": "k", "s": ("sum", "v")}, kind, expect=expect, passes=1)
        run(small, host, {"by": "k", "av": ("avg", "v"), "c": ("count", "v"), "f": ("first", "r")}, kind, expect=expect, passes=1)


# ---------------------------------------------------------------- 3. LDS limit
def test_largest_range_whose_tables_fit(small):
    """sum f64 on 256 partitions: 12 bytes a cell, (153 600 - 4 160) // 12 = 12 453 cells, x 256 = 3 187 968 keys.  That range: the planes answer; 256 keys
    more: 12 454 cells do not fit, the planes decline (before the scatter when the sample saw the whole range, after it otherwise), same answer.
    3.5e6 rows: 1.1 x the range -- dense for the planner (range <= rows) and for the sample."""
    cells = (LDS_MAX - WINDOWS) // 12
    rng = cells * 256
    assert agg_lds(cells, 1, 1) <= LDS_MAX < agg_lds(cells + 1, 1, 1) and cells <= 1 << 14 and rng == 3_187_968
    n = 3_500_003
    for extra, expect in ((0, "planes"), (256, "declined")):
        k = rfo.gen_i64(n, 4, rng + extra) - 1_000_001
        k[1], k[2] = -1_000_001, -1_000_001 + rng + extra - 1  # the range, exactly
        for kind in ("exact", "real"):
            run(small, mk(n, k, kind), {"by": "k", "s": ("sum", "v")}, kind, expect=expect, passes=1)


# ---------------------------------------------------------------- 4. key edges
KEY_EDGES = {"kmin_odd": 77, "kmin_negative": -70_001, "at_int64_max": I64_MAX - 199_999, "at_int64_min": I64_MIN + 1}


@pytest.mark.parametrize("edge", list(KEY_EDGES))
def test_key_edges(small, edge):
    """kmin that is no multiple of 128 / 256, a negative kmin, keys that end at INT64_MAX and keys that start at INT64_MIN + 1 (the null is INT64_MIN):
    the `shift` arithmetic of the aggregate's apply() and the scope's order-preserving images."""
    n = 500_009
    k = rfo.gen_i64(n, 4, 200_000) + KEY_EDGES[edge]
    k[3], k[4] = KEY_EDGES[edge], KEY_EDGES[edge] + 199_999
    for kind in ("real", "exact"):
        host = mk(n, k, kind)
        run(small, host, {"by": "k", "s": ("sum", "v")}, kind, passes=1)
        run(small, host, {"where": ("<", "a", 700_000), "by": "k", "mn": ("min", "v"), "av": ("avg", "v"), "f": ("first", "r")}, kind, passes=1)


def test_only_null_key_in_the_last_row(small):
    """The sample cannot see it; the scatter's scope does (its minimum is the null) and hands the query back: a scatter, no overflow, no plane aggregate
    (two value columns: nothing else counts into counter 2).  Stated expectation for ONE value column: the dense planes hand back as before, the planner
    then groups on the hashed tables (a null key is not dense), and THAT route's planes -- k_plane_scatter<.., HK> + k_plane_hash_aggregate, which count
    into the same two counters -- answer with the null in the device-wide table: two scatters, one aggregate launch, no overflow."""
    n = 500_009
    k = rfo.gen_i64(n, 4, 200_000) + 77
    k[n - 1] = NULL
    for kind in ("real", "exact"):
        host = mk(n, k, kind)
        run(small, host, {"by": "k", "s1": ("sum", "v"), "s2": ("sum", "w")}, kind, expect="handed_back")
        s0 = stats(small)
        (check_exact if kind == "exact" else check_select)(small, host, {"by": "k", "s": ("sum", "v")})
        d = [y - x for x, y in zip(s0, stats(small))]
        assert d[0] == 2 and d[1] == 0 and d[2] == 1, d


# ---------------------------------------------------------------- 5. / 6. block structure: one child process per setting
def block_keys(n, card, layout, seed=4):
    r = np.arange(n, dtype=np.int64)
    if layout == "random":
        return rfo.gen_i64(n, seed, card) + 77
    if layout == "sorted":  # every key a run of n / card rows: first rows climb through the blocks
        return r * card // n + 77
    assert layout == "cyclic"
    return r % card + 77


def child_dense(eng, threads, block_rows, split_env):
    """The block structure of the headline at a size the oracle checks in seconds.  `threads` picks the aggregate: 1024 lanes (every pass's tables beyond
    52 KB; Q = 16 x split) or 512 lanes (Q = 8 x workgroups per partition, 64 at most on 256 CUs).  Row counts: more than 128 x Q blocks, so a wave owns more than 128
    regions (its count window is filled three times), and no multiple of Q (the waves' region counts differ: `nreg`).  FAST: `sum v`; general: `avg v` + `first r`
    (r = the row number: first rows bit for bit; beyond 150 KB together they run as two passes, the second one FIRST only)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Qs = wave_strides(threads, cus, split_env)
    nblk0 = 128 * Qs[-1] + 37
    while any(nblk0 % Q == 0 or (nblk0 + 1) % Q == 0 for Q in Qs):
        nblk0 += 1
    # key ranges: the row count follows from the blocks, the range must stay below the rows a filter keeps (the planner's "dense")
    card = min(1_000_000, int(nblk0 * block_rows / 3.2) // 128 * 128) if threads == 1024 else 243_200
    local = (card + 127) >> 7
    if threads == 1024:
        assert agg_lds(local, 1, 1) > 52 * 1024  # the smallest pass there is (first rows + one accumulator)
    else:
        assert agg_lds(local, 2, 2) <= 52 * 1024  # avg + first together: 1 900 cells x 24 + 4160 = 49 760
    done = []
    for name, layout, tail, fast, filt in (("random_fast", "random", 513, True, None), ("sorted_general", "sorted", 1, False, None),
                                           ("cyclic_gap_fast", "cyclic", 511, True, "gap"), ("random_tail_off_general", "random", 513, False, "tail_off"),
                                           ("last_row_only", "random", 511, True, "last_row"), ("tail_rows_only", "cyclic", 513, True, "tail_only")):
        n = (nblk0 - 1) * block_rows + tail
        nblk = (n + block_rows - 1) // block_rows
        assert all(nblk > 128 * Q and nblk % Q != 0 for Q in Qs) and n <= 4_600_000, (name, Qs, nblk, n)
        aggs = {"s": ("sum", "v")} if fast else {"av": ("avg", "v"), "f": ("first", "r")}
        expect, where = "planes", None
        if filt == "gap":  # the first rows (1.3 x the key range: still dense) and the last three blocks: regions of count 0 all through the middle of every wave's walk
            lo, hi = int(1.3 * card), n - tail - 3 * block_rows
            assert lo + 64 * Qs[-1] * block_rows < hi
            where = ("or", ("<", "r", lo), (">=", "r", hi))
        elif filt == "tail_off":  # everything but the ragged tail
            where = ("<", "r", n - tail)
        elif filt == "last_row":  # one selected row: the sample sees none of it, the planes are not tried -- stated expectation: no plane aggregate, same answer
            where, expect = ("==", "r", n - 1), "declined"
        elif filt == "tail_only":
            where, expect = (">=", "r", n - tail), "declined"
        for kind in (("exact",) if expect == "declined" else ("exact", "real")):
            host = mk(n, block_keys(n, card, layout), kind)
            q = dict(by="k", **aggs)
            if where is not None:
                q["where"] = where
            run(eng, host, q, kind, expect=expect)
        done.append(name)
    return done


def child_sparse(eng, block_rows, parts_env):
    """Sparse keys (`k * 1_000_003 - 77`) over 2048-row blocks: k_plane_scatter<.., HK> + k_plane_hash_aggregate, whose 16 waves walk blocks q, q + 16, ...
    -- more than 128 x 16 blocks.  LDS entries: sum f64 20 bytes -> 7 424 a table; the estimate x 1.3 / partitions decides: up to 731 000 keys 128 x 1,
    up to 1 462 000 256 x 1 (the interleaved form), and with RFX_PLANE_HASH_PARTS=128 two workgroups a partition there, four up to 2 924 000."""
    nblk = 128 * 16 + 13
    n = (nblk - 1) * block_rows + 513
    assert n <= 4_600_000
    forms = {0: (("128x1", 300_000), ("256x1_interleaved", 1_000_000)), 128: (("128x2", 1_000_000), ("128x4", 2_400_000))}[parts_env]
    done = []
    for name, distinct in forms:
        for kind in ("exact", "real"):
            host = mk(n, rfo.gen_i64(n, 4, distinct) * 1_000_003 - 77, kind)
            run(eng, host, {"by": "k", "s": ("sum", "v")}, kind, passes=1)
            run(eng, host, {"where": ("<", "a", 500_000), "by": "k", "s": ("sum", "v")}, kind, passes=1)
        done.append(name)
    # COUNT / FIRST only -- this route takes it (no value plane: the key rides as the value), and a general plan
    host = mk(n, rfo.gen_i64(n, 4, 300_000) * 1_000_003 - 77, "exact")
    if parts_env == 0:
        run(eng, host, {"by": "k", "c": ("count", "a"), "f": ("first", "r")}, "exact", passes=1)
        run(eng, host, {"where": ("<", "a", 500_000), "by": "k", "av": ("avg", "v"), "c": ("count", "v")}, "exact", passes=1)
        done.append("count_first_only")
    return done


CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_plane_edges_gpu as T
from rayforce_amd.engine import Engine
eng = Engine(0)
eng.tune(flags=T.CHUNK_SMALL)
print("cases:", {call})
eng.close()
print("child ok")
"""


def _child(env, call):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    p = subprocess.run([sys.executable, "-c", CHILD.format(root=root, tests=here, call=call)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900, cwd=root)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]


@pytest.mark.parametrize("threads,block_rows,split", [(1024, 2048, 0), (1024, 1024, 0), (512, 512, 0), (1024, 1024, 2), (1024, 512, 3)])
def test_block_structure(built, threads, block_rows, split):
    """RFX_PLANE_BLOCK_ROWS of 2048 and 1024 on the 1024-lane aggregate; 512 on the 512-lane one (Q up to 64 there: 8 192 blocks of 1024 rows would be 8.4e6
    rows); RFX_PLANE_AGG_SPLIT=2 / 3 (the non-exclusive write-out, Q = 32 / 48) at the block size that keeps the table below 4.6e6 rows."""
    env = {"RFX_PLANE_BLOCK_ROWS": str(block_rows)}
    if split:
        env["RFX_PLANE_AGG_SPLIT"] = str(split)
    _child(env, f"T.child_dense(eng, {threads}, {block_rows}, {split})")


@pytest.mark.parametrize("parts", [0, 128])
def test_sparse_keys_over_small_blocks(built, parts):
    """child_sparse over 2 061 blocks of 2 048 rows with a ragged tail: the default policy (128 x 1 and the interleaved 256 x 1) and, under
    RFX_PLANE_HASH_PARTS=128, two and four workgroups per partition; each with and without a filter."""
    env = {"RFX_PLANE_BLOCK_ROWS": "2048"}
    if parts:
        env["RFX_PLANE_HASH_PARTS"] = str(parts)
    _child(env, f"T.child_sparse(eng, 2048, {parts})")
