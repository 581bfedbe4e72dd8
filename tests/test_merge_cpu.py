"""The merge of sorted runs without a GPU: the numpy restatement (tests/merge_ref.py) equals np.lexsort of the whole table on every run shape and
key content the GPU tests walk, the splitter rule places every splitter where the merged order has it, and the library as built exports and
declares the new entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import merge_ref as M
import sort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024  # (the shipped one is asserted equal on the GPU box: rfx_hip_merge_tile())


@pytest.mark.parametrize("kind", M.KINDS)
def test_merged_runs_equal_the_sort_of_the_whole(kind):
    rng = np.random.default_rng(len(kind))
    for lens in M.run_shapes(TILE):
        cols, f64s = M.cells(kind, lens, rng)
        for desc in (False, True):
            runs = M.make_runs(cols, f64s, lens, desc)
            perm, vals = M.merge(runs, f64s, desc)
            want = R.lex_order(cols, f64s, desc) if sum(lens) else np.empty(0, np.int64)
            assert np.array_equal(perm, want), (kind, lens, desc)
            assert np.array_equal(vals, cols[0][want]), (kind, lens, desc)
            if len(cols) == 1 and sum(lens):
                assert np.array_equal(vals, R.values(cols[0], f64s[0], desc)[0]), (kind, lens, desc)


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("tile", [512, 1024])
def test_a_splitters_co_ranks_sum_to_its_place(kind, tile):
    rng = np.random.default_rng(tile + len(kind))
    for lens in ([tile - 1, tile, tile + 1], [0, 3 * tile + 7, 0, 2 * tile], [40] * 15 + [40_000], [tile + 1] * 16):
        cols, f64s = M.cells(kind, lens, rng)
        for desc in (False, True):
            runs = M.make_runs(cols, f64s, lens, desc)
            perm, _ = M.merge(runs, f64s, desc)
            sp = M.splitters(runs, f64s, tile, desc)
            assert len(sp) == sum((n - 1) // tile for n in lens if n)
            places = [s[3] for s in sp]
            assert len(set(places)) == len(places)
            for a, p, co, place in sp:
                assert perm[place] == runs[a][2] + runs[a][1][p], (kind, lens, desc, a, p)
                assert all(0 <= c <= n for c, n in zip(co, lens))
            # between two consecutive splitters no run contributes more than `tile` records
            by_place = sorted(sp, key=lambda s: s[3])
            los = [[0] * len(lens)] + [s[2] for s in by_place]
            his = [s[2] for s in by_place] + [list(lens)]
            for lo, hi in zip(los, his):
                assert all(0 <= h - l <= tile for l, h in zip(lo, hi)), (kind, lens, desc)


def test_library_exports_and_bindings_declare_the_merge():
    lib = C.CDLL(os.path.join(ROOT, "rayforce_amd", "librfx.so"))
    from rayforce_amd import _lib as L
    from rayforce_amd.engine import Engine
    for s in ("rfx_hip_merge_runs", "rfx_hip_merge_tile", "rfx_exec_sort_shards"):
        assert hasattr(lib, s), s
        assert s in L.PROTOTYPES, s
    assert C.sizeof(L.MergeRun) == 8 * L.RFX_MAX_KEYS + 24
    assert L.RFX_MERGE_MAX_RUNS == L.RFX_MAX_SHARDS
    assert hasattr(Engine, "merge_runs")
    import inspect
    assert "over_shards" in inspect.signature(Engine.sort_index).parameters and "over_shards" in inspect.signature(Engine.sort_values).parameters
