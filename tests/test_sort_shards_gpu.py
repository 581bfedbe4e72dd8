"""The sort over shards on the GPU, all by equality of bits: the flat merge kernel against the numpy restatement (tests/merge_ref.py), the planner
through Engine(..., shards=k) against tests/sort_ref.py and against the unsharded engine, the door under RFX_SHARDS=k in a process of its own
against the reference's fixture (tests/golden/sort_golden.npz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import merge_ref as M
import sort_ref as R
from rayforce_amd import _lib as L
from rayforce_amd.engine import Engine
from test_sort_gpu import cells_of, check_sorted

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the flat kernel
def upload_runs(eng, runs):
    return [([eng.column(k) for k in keys], eng.column(rows), row0) for keys, rows, row0 in runs]


def test_the_shipped_tile(eng):
    assert eng.lib.rfx_hip_merge_tile() == 1024  # (what tests/test_merge_cpu.py restates the splitters with)


@pytest.mark.parametrize("kind", M.KINDS)
def test_flat_merge_equals_the_restatement(eng, kind):
    tile = eng.lib.rfx_hip_merge_tile()
    rng = np.random.default_rng(len(kind))
    for lens in M.run_shapes(tile):
        cols, f64s = M.cells(kind, lens, rng)
        types = [L.RFX_F64 if f else L.RFX_I64 for f in f64s]
        for desc in (False, True):
            runs = M.make_runs(cols, f64s, lens, desc)
            want_perm, want_vals = M.merge(runs, f64s, desc)
            dev = upload_runs(eng, runs)
            outputs = [(True, False)] + ([(False, True), (True, True)] if len(cols) == 1 else [])
            for want_p, want_v in outputs:
                perm, vals = eng.merge_runs(dev, types, desc, want_perm=want_p, want_values=want_v)
                if want_p:
                    assert np.array_equal(perm.cpu().numpy(), want_perm), (kind, lens, desc, want_p, want_v)
                if want_v:
                    assert np.array_equal(vals.cpu().numpy(), want_vals), (kind, lens, desc, want_p, want_v)


@pytest.mark.parametrize("tile", [512, 2048])
def test_flat_merge_with_another_tile(eng, tile):
    rng = np.random.default_rng(tile)
    for kind in ("interleaved", "f64_special", "two_columns"):
        for lens in ([tile - 1, tile, tile + 1], [0, 3 * tile + 7, 1, 40_000]):
            cols, f64s = M.cells(kind, lens, rng)
            runs = M.make_runs(cols, f64s, lens, True)
            perm, _ = eng.merge_runs(upload_runs(eng, runs), [L.RFX_F64 if f else L.RFX_I64 for f in f64s], True, tile=tile)
            assert np.array_equal(perm.cpu().numpy(), M.merge(runs, f64s, True)[0]), (kind, lens, tile)


def test_flat_merge_of_a_gap_wider_than_one_staging_window(eng):
    """16 runs whose keys interleave one to one: every gap between splitters holds close to a tile of EVERY run (8 staging windows)"""
    k, n = 16, 3000
    cols = [np.tile(np.arange(n, dtype=np.int64), k)]  # run r = 0 .. n-1: equal keys across all runs, ordered by run
    runs = M.make_runs(cols, [False], [n] * k)
    for want_v in (False, True):
        perm, vals = eng.merge_runs(upload_runs(eng, runs), [L.RFX_I64], False, want_values=want_v)
        want = M.merge(runs, [False])
        assert np.array_equal(perm.cpu().numpy(), want[0])
        assert not want_v or np.array_equal(vals.cpu().numpy(), want[1])


def test_flat_merge_refuses_what_it_does_not_take(eng):
    a = eng.column(np.arange(10, dtype=np.int64))
    with pytest.raises(L.RfxError):
        eng.merge_runs([([a], a, 0)], [L.RFX_I64], tile=100)
    with pytest.raises(L.RfxError):
        eng.merge_runs([([a, a], a, 0)], [L.RFX_I64, L.RFX_I64], want_values=True)
    with pytest.raises(L.RfxError):
        eng.merge_runs([([a], a, 0)] * 17, [L.RFX_I64])


# ---------------------------------------------------------------------------------------------------- the planner
@pytest.fixture(scope="module")
def sharded(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    engines = {}

    def get(k):
        if k not in engines:
            engines[k] = Engine(0, shards=k)
        return engines[k]

    yield get
    for e in engines.values():
        e.close()


def check_case(eng, es, kind, n):
    rng = np.random.default_rng(n * 31 + len(kind))
    bits, f64 = cells_of(rng, kind, n)
    bits = np.ascontiguousarray(bits, dtype=np.int64)
    col = eng.column(bits.view(np.float64) if f64 else bits)
    for desc in (False, True):
        got = es.sort_index(col, descending=desc, over_shards=True)
        assert np.array_equal(got.cpu().numpy(), R.order(bits, f64, desc)[0]), (kind, n, desc)
        assert torch.equal(got, eng.sort_index(col, descending=desc)), (kind, n, desc)
        vals = es.sort_values(col, descending=desc, over_shards=True)
        assert np.array_equal(vals.cpu().numpy().view(np.int64), R.values(bits, f64, desc)[0]), (kind, n, desc, "values")
        assert torch.equal(vals.view(torch.int64), eng.sort_values(col, descending=desc).view(torch.int64)), (kind, n, desc, "values")


@pytest.mark.parametrize("kind", ["narrow", "full", "one_digit", "extremes", "f64"])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_planner_over_shards_equals_the_restatement_and_one_shard(eng, sharded, k, kind):
    for n in (1, 2, 63, 64, 65, 4097, 100_003):
        check_case(eng, sharded(k), kind, n)


@pytest.mark.parametrize("kind", ["narrow", "full", "one_digit", "extremes", "f64"])
@pytest.mark.parametrize("k", [2, 8])
def test_planner_over_shards_3e6_rows(eng, sharded, k, kind):
    check_case(eng, sharded(k), kind, 3_000_001)


def test_two_and_three_columns_over_shards(eng, sharded):
    rng = np.random.default_rng(5)
    n = 200_003
    a, b, c = rng.integers(0, 50, n), (rng.integers(-3, 3, n) * 0.5).view(np.int64), rng.integers(0, 4, n)
    cols = [eng.column(a), eng.column(b.view(np.float64)), eng.column(c)]
    for k in (3, 5):
        es = sharded(k)
        for desc in (False, True):
            for m in (2, 3):
                got = es.sort_index(cols[:m], descending=desc, over_shards=True)
                assert np.array_equal(got.cpu().numpy(), R.lex_order([a, b, c][:m], [False, True, False][:m], desc)), (k, desc, m)
                assert torch.equal(got, eng.sort_index(cols[:m], descending=desc))


def test_counters_and_the_one_shard_path(eng, sharded):
    bits = np.random.default_rng(9).integers(0, 1_000_000, 50_000)
    col = eng.column(bits)
    before = [eng.xstat(s) for s in (L.RFX_XSTAT_SORTS, L.RFX_XSTAT_SORT_PASSES, L.RFX_XSTAT_SORT_MERGES)]
    plain = eng.sort_index(col)
    mid = [eng.xstat(s) for s in (L.RFX_XSTAT_SORTS, L.RFX_XSTAT_SORT_PASSES, L.RFX_XSTAT_SORT_MERGES)]
    same = eng.sort_index(col, over_shards=True)  # one shard: the existing path, no merge
    after = [eng.xstat(s) for s in (L.RFX_XSTAT_SORTS, L.RFX_XSTAT_SORT_PASSES, L.RFX_XSTAT_SORT_MERGES)]
    assert torch.equal(plain, same)
    assert [m - b for m, b in zip(mid, before)] == [a - m for a, m in zip(after, mid)] == [1, 3, 0]
    es = sharded(3)
    b3 = [es.xstat(s) for s in (L.RFX_XSTAT_SORTS, L.RFX_XSTAT_SORT_MERGES)]
    es.sort_index(col, over_shards=True)
    assert [es.xstat(s) - b for s, b in zip((L.RFX_XSTAT_SORTS, L.RFX_XSTAT_SORT_MERGES), b3)] == [3, 1]
    with pytest.raises(L.RfxError, match="sort over a sharded table"):  # the default stays the refusal
        es.sort_index(col)
    with pytest.raises(L.RfxError, match="sort over a sharded table"):
        es.sort_values(col)


def test_a_merge_tile_the_kernel_does_not_take_is_ignored(eng):
    """RFX_MERGE_TILE is a measurement knob read when a planner is made: a value outside 512 .. 2048 must not fail the sort"""
    bits = np.random.default_rng(10).integers(0, 1000, 20_011)
    col = eng.column(bits)
    for tile in ("7", "2048"):
        os.environ["RFX_MERGE_TILE"] = tile
        try:
            es = Engine(0, shards=3)
        finally:
            del os.environ["RFX_MERGE_TILE"]
        try:
            assert np.array_equal(es.sort_index(col, over_shards=True).cpu().numpy(), R.order(bits, False)[0]), tile
        finally:
            es.close()


def test_2_pow_24_plus_5_rows_over_five_shards_by_properties(eng, sharded):
    n = 2**24 + 5
    g = torch.Generator(device="cuda:0").manual_seed(6)
    col = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=g)
    col[::1000] = float("nan")
    col[1::1000] = -0.0
    col[2::1000] = 0.0
    for desc in (False, True):
        perm = sharded(5).sort_index(col, descending=desc, over_shards=True)
        check_sorted(eng, col, True, perm, desc)


# ---------------------------------------------------------------------------------------------------- the door
_SHARDED_DOOR = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import numpy as np
import sort_ref as R
import test_sort_gpu as T
from rayforce_amd import hostobj as H
ops = H.lib()
assert ops.rfx_host_bind() == 0
# the asserts of the one-shard tests, as they are: cells, type codes, attribute bytes, rfx_last_sort_on_gpu() -- lengths 0, 1, 2 leave shards without rows,
# 20011 rows of ties are the stability case
T.test_fixture_vectors_through_the_operators(ops)
assert ops.rfx_ops_shards() == SHARDS, ops.rfx_ops_shards()
T.test_fixture_tables_through_xasc_and_xdesc(ops)
# more columns than one gather launch takes: the batched concatenate-and-gather runs twice
rng = np.random.default_rng(12)
n, ncol = 20011, 11
host = {f"c{i}": (rng.integers(0, 7, n) if i < 2 else rng.integers(-2**62, 2**62, n)) for i in range(ncol)}
host["c1"] = (rng.integers(-3, 3, n) * 0.5)
tab = H.table(host)
for verb, desc in (("rfx_xasc", False), ("rfx_xdesc", True)):
    y = H.symbols(["c0", "c1"])
    r = getattr(ops, verb)(tab, y)
    assert not H.is_error(r), H.error_text(r)
    assert ops.rfx_last_sort_on_gpu() == 1
    got = H.table_to_numpy(r)
    perm = R.lex_order([host["c0"], host["c1"].view(np.int64)], [False, True], desc)
    assert list(got) == list(host)
    for name in host:
        assert np.array_equal(np.asarray(got[name]).view(np.int64), np.asarray(host[name][perm]).view(np.int64)), (verb, name)
    ops.rfx_host_drop(r)
    ops.rfx_host_drop(y)
assert ops.rfx_ops_shards() == SHARDS
print("SORT-DOOR-OK", SHARDS)
'''


def run_door(built, shards, extra_env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    code = f"ROOT = {ROOT!r}\nSHARDS = {shards}\n" + _SHARDED_DOOR
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "SORT-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


@pytest.mark.parametrize("shards", [2, 3, 8])
def test_sort_over_shards_through_the_door(built, shards):
    """RFX_SHARDS=k in a process of its own (the operator layer's shards are fixed at its first call): stand-alone, no host verbs bound"""
    run_door(built, shards, {"RFX_SHARDS": str(shards)})


def test_sort_over_every_device_through_the_door(built):
    """RFX_DEVICES=all: one shard per device, the runs of the other devices copied to shard 0's before the merge"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    run_door(built, min(torch.cuda.device_count(), L.RFX_MAX_SHARDS), {"RFX_DEVICES": "all"})
