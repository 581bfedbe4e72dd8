"""The window join's contract without a GPU: the numpy restatement (tests/wj_ref.py) equals the fixture written from the compiled reference
(tests/golden/wj_golden.npz, tests/golden/make_wj_golden.py) in every case, for both verbs and all seven aggregates over an I64 and an F64 column, bit
for bit; the fixture covers what it is meant to cover; the library as built exports the operators, the planner and the kernel entry points, and the
standalone host binds both verbs' names."""
import ctypes as C
import os

import numpy as np
import pytest

import wj_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "wj_golden.npz")


@pytest.fixture(scope="module")
def cases():
    gold = np.load(GOLD)
    return [R.load_case(gold, ci) for ci in range(len(gold["cases"]))]


def test_fixture_is_small_and_data_only():
    assert os.path.getsize(GOLD) < 1_000_000
    gold = np.load(GOLD)  # (allow_pickle is off: arrays of numbers and of strings only)
    assert all(gold[k].dtype.kind in "uU" for k in gold.files)


def test_restatement_equals_the_reference_in_every_case(cases):
    for c in cases:
        for closed in (0, 1):
            got = R.window_join(c["lk"], c["rk"], c["lo"], c["hi"], c["rt"], closed, {"vi": c["vi"], "vf": c["vf"]})
            for col in ("vi", "vf"):
                for a in R.AGGS:
                    want = c["out"][closed][col][a]
                    assert got[(a, col)].dtype == np.int64 and np.array_equal(got[(a, col)], want), (c["name"], closed, a, col, int((got[(a, col)] != want).sum()))


def test_the_lang_examples_are_what_the_reference_answers(cases):
    c = cases[0]
    assert c["name"] == "lang_examples" and c["kinds"] == ["sym"]
    assert list(c["out"][0]["vi"]["min"]) == [99, 100]   # tests/lang.c:4289-4295
    assert list(c["out"][1]["vi"]["min"]) == [99, 101]   # tests/lang.c:4297-4303
    assert list(c["out"][0]["vi"]["count"]) == [2, 2] and list(c["out"][1]["vi"]["count"]) == [2, 1]  # (the prevailing quote is inside window-join's window only)


def windows_of(c, closed):
    _, li, ri = R.window_ranges(c["lk"], c["rk"], c["lo"], c["hi"], c["rt"], closed)
    return li, ri, np.where(li < 0, 0, ri - li + 1)


def test_fixture_covers_the_listed_cases(cases):
    by = {c["name"]: c for c in cases}
    assert {c["nk"] for c in cases} == {1, 2, 3}
    assert any(c["kinds"] == ["sym"] for c in cases) and any(c["kinds"] == ["sym", "i64"] for c in cases) and any(c["kinds"] == ["i64"] for c in cases)
    sizes = {0, 1, 63, 64, 65, 4097, 20011}
    assert sizes - {0} <= {len(c["lt"]) for c in cases if len(c["rt"])} and sizes <= {len(c["rt"]) for c in cases if len(c["lt"])}
    # every case ran with one thread and with eight, except the empty left table
    assert [c["name"] for c in cases if c["threads"] != "1,8"] == ["empty_left"] and len(by["empty_left"]["lt"]) == 0 and by["empty_left"]["threads"] == "1"
    # right tables in no order: rows whose (key, time) go down
    shuffled = 0
    for c in cases:
        if c["nk"] == 1 and len(c["rt"]) > 1:
            k, t = c["rk"][0], R.narrow(c["rt"])
            shuffled += bool(((k[1:] < k[:-1]) | ((k[1:] == k[:-1]) & (t[1:] < t[:-1]))).any() and (t[1:] < t[:-1]).any())
    assert shuffled >= 6
    for want in ("sym_keys_sorted", "sym_keys_shuffled", "two_keys", "three_keys", "null_keys", "null_times", "ties", "all_equal_times", "mostly_null_cells",
                 "all_null_cells", "before_after_spanning_reversed_zero_width", "group_lengths_sorted", "group_lengths_shuffled", "one_group_sorted",
                 "one_group_shuffled", "window_lengths", "sorted_20011x1000", "sorted_1000x20011"):
        assert want in by, want
    c = by["null_keys"]
    assert all((k == R.NULL).any() for k in c["lk"] + c["rk"])
    both_null = (c["lk"][0] == R.NULL) & (c["lk"][1] == R.NULL)
    assert (c["out"][0]["vi"]["count"][both_null] > 0).any()  # a NULL key equals a NULL key
    c = by["null_times"]
    assert all((c[n] == R.NULL32).any() for n in ("lo", "hi", "rt"))
    c = by["sym_keys_sorted"]
    absent = ~np.isin(c["lk"][0], c["rk"][0])
    assert absent.any() and (c["out"][0]["vi"]["count"][absent] == 0).all() and (c["out"][0]["vi"]["sum"][absent] == R.NULL).all()
    assert set(np.bincount(by["group_lengths_shuffled"]["rk"][0])) == {1, 2, 3, 64, 65}
    assert len(set(by["one_group_sorted"]["rk"][0])) == 1 and len(by["one_group_sorted"]["rk"][0]) == 4097
    t = R.narrow(by["ties"]["rt"])
    assert len(np.unique(t)) < len(t) // 10
    c = by["before_after_spanning_reversed_zero_width"]
    assert (c["lo"] > c["hi"]).any() and (c["lo"] == c["hi"]).any() and (c["hi"] < 400).any() and (c["lo"] >= 500).any() and ((c["lo"] < 400) & (c["hi"] >= 500)).any()
    # windows whose every cell is null, and windows with some: min over I64 answers INT64_MAX there, max answers null
    c = by["mostly_null_cells"]
    allnull = (c["out"][0]["vi"]["count"] > 0) & (c["out"][0]["vi"]["min"] == R.INF)
    assert allnull.any() and (c["out"][0]["vi"]["max"][allnull] == R.NULL).all()
    partly = (c["out"][0]["vi"]["sum"] == R.NULL) & (c["out"][0]["vi"]["min"] != R.INF) & (c["out"][0]["vi"]["count"] > 0)
    assert partly.any()
    f = c["out"][0]["vf"]
    nanwin = (f["count"] > 0) & (f["min"] == np.array([np.inf]).view(np.int64)[0])
    assert nanwin.any() and (f["max"][nanwin] == R.NAN_BITS).all() and (f["avg"][nanwin] == R.NAN_BITS).all()
    assert np.isnan(by["all_null_cells"]["vf"]).all() and (by["all_null_cells"]["vi"] == R.NULL).all()
    # window lengths on both sides of the fold's boundaries: a lane's at most 16 rows, a wave's 128 rows per step
    for closed in (0, 1):
        lens = set(windows_of(by["window_lengths"], closed)[2])
        assert set(range(0, 41)) | {127, 128, 129, 255, 256, 257, 511, 512, 513, 1000} <= lens, closed
    li = windows_of(by["window_lengths"], 1)[0]
    assert {0, 1} <= set(li[li >= 0] % 2)
    # null rows exist and differ between the verbs somewhere
    assert any((c["out"][0]["vi"]["count"] == 0).any() for c in cases) and any((c["out"][0]["vi"]["count"] != c["out"][1]["vi"]["count"]).any() for c in cases)
    # F64 cells are multiples of 1/8 of small magnitude: exact sums in any order
    for c in cases:
        v = c["vf"][~np.isnan(c["vf"])]
        assert np.array_equal(v * 8, np.round(v * 8)) and (np.abs(v) <= 16).all(), c["name"]


SYMBOLS = ["rfx_window_join", "rfx_window_join1", "rfx_last_window_on_gpu", "rfx_exec_window_ranges", "rfx_exec_window_fold", "rfx_hip_window_ranges", "rfx_hip_window_fold"]


def test_library_exports_the_window_entry_points():
    lib = C.CDLL(os.path.join(ROOT, "rayforce_amd", "librfx.so"))
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_python_bindings_declare_them_and_the_host_binds_the_names():
    from rayforce_amd import _lib as L, hostobj as H
    from rayforce_amd.engine import Engine
    for s in SYMBOLS[3:]:
        assert s in L.PROTOTYPES or s in L.EXEC_PROTOTYPES, s
    for s in SYMBOLS[:3]:
        assert s in H.OPS_PROTOTYPES, s
    assert hasattr(Engine, "window_join")
    lib = H.lib()
    for name, sym in (("window-join", "rfx_window_join"), ("window-join1", "rfx_window_join1")):
        fn = lib.rfx_host_fn(name.encode())
        assert fn, name
        assert H.header(fn).type == 103 and H.header(fn).attrs == 0, name
        assert C.c_int64.from_address(fn + 8).value == C.cast(getattr(lib, sym), C.c_void_p).value, name
    assert lib.rfx_host_fn(b"last")  # (last column) among the aggregates


# ---------------------------------------------------------------------------------------------------- what tests/test_wj_edges_gpu.py stands on
def test_rows_per_wave_at_its_thresholds():
    for cus in (256, 64, 32):
        W = cus * 32
        for r in (1, 2, 4, 8, 16, 32, 64):
            lo = R.n_lo(r, cus)
            assert lo == W * r - r + 1 and R.rows_per_wave(lo, cus, 1) == r, (cus, r)
            assert -(-lo // r) == W and lo % r == 1 % r  # every wave slot once; the last wave holds one row
            if r >= 2:
                assert R.rows_per_wave(W * r - r, cus, 1) == r // 2, (cus, r)
            if r < 64:
                assert R.rows_per_wave(R.n_lo(2 * r, cus) - 1, cus, 400) == r, (cus, r)
            for n in (1, lo - 1, lo, 3 * lo, 64 * W + 65):
                assert R.rows_per_wave(n, cus, 0) == 64, (cus, n)
        # the second trips of the wave loop (cus * 32 waves a trip) at 1 and at 64 rows per wave
        assert R.rows_per_wave(1, cus, 1) == 1 and R.rows_per_wave(W + W // 2 + 1, cus, 1) == 1 and R.rows_per_wave(64 * W + 65, cus, 1) == 64
    assert 8192 + 8192 // 2 + 1 == 8192 + 4097


def exact_cells(dtype, nv, rng):
    """cells whose f64 sums are exact in every order: I64 multiples of 2^40 within +-2^62 (the I64 sums wrap), F64 multiples of 0.25 below 2^30.
    5 % nulls, all of them in the column's first half (10 % there) so that long windows of the second half keep a sum, and a run of 40"""
    null = (rng.random(nv) < 0.1) & (np.arange(nv) < nv // 2)
    null[100:140] = True
    if dtype == "i64":
        v = rng.integers(-(2**22), 2**22, nv) << 40
        v[null] = R.NULL
    else:
        v = rng.integers(-(2**32) + 1, 2**32, nv) * 0.25
        v[null] = np.nan
    return v


@pytest.mark.parametrize("dtype", ["i64", "f64"])
def test_fold_direct_equals_the_replay_on_the_edge_windows(dtype):
    rng = np.random.default_rng(3)
    nv, n = 1031, 3001
    li, ri, info = R.edge_windows(nv, n, rng)
    length = np.where(li < 0, 0, ri - li + 1)
    # what the set is there for
    assert set(R.EDGE_LENGTHS) | {nv, nv - 1, nv - 2, nv - 3} <= set(length) and 0 < (length > 16).sum() <= 512
    for L, Rr in info["edge"]:
        assert ((li == L) & (ri == Rr)).any(), (L, Rr)
    assert sorted(info["shuffle"]) != list(info["shuffle"]) and len(set(info["shuffle"])) == n - 256
    b = info["blocks"]
    assert all(at % 64 == 0 for at in b.values())
    assert (length[b["all_long"]:b["all_long"] + 64] > 16).all() and (li[b["all_null"]:b["all_null"] + 64] == -1).all()
    assert list(np.flatnonzero(length[b["lane0_long"]:b["lane0_long"] + 64] > 16)) == [0]
    assert list(np.flatnonzero(length[b["lane63_long"]:b["lane63_long"] + 64] > 16)) == [63]
    assert {0, 1} <= set(li[length > 16] % 2) and {0, 1} <= set(ri[length > 16] % 2) and (ri[length > 16] == nv - 1).any()
    v = exact_cells(dtype, nv, rng)
    want, got = R.window_fold(v, li, ri), R.fold_direct(v, li, ri)
    for a in R.AGGS:
        assert got[a].dtype == want[a].dtype, a
        bad = np.flatnonzero(np.ascontiguousarray(got[a]).view(np.int64) != np.ascontiguousarray(want[a]).view(np.int64))
        assert bad.size == 0, (a, bad[:5], li[bad[:5]], ri[bad[:5]], got[a][bad[:5]], want[a][bad[:5]])
    summed = ~np.isnan(want["sum"]) if dtype == "f64" else want["sum"] != R.NULL
    assert (summed & (length > 16)).sum() >= 10 and (~summed & (length > 16)).sum() >= 10 and (summed & (length > 500)).any()
    if dtype == "i64":
        assert np.array_equal(R.sum_by_cumsum(v, li, ri), want["sum"])
        full = want["sum"] != R.NULL
        assert (np.abs(want["avg"][full & (length > 2)] * length[full & (length > 2)]) > 2.0**63).any()  # some sums wrapped
        covered = (li >= 100) & (ri < 140)
        assert covered.any() and (want["min"][covered] == R.INF).all() and (want["max"][covered] == R.NULL).all()
    else:
        covered = (li >= 100) & (ri < 140)
        assert covered.any() and np.isinf(want["min"][covered]).all() and np.isnan(want["max"][covered]).all()
