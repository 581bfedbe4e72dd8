"""The partition and collect kernels (rayforce_amd/csrc/rfx_collect.hip) beyond what a query-sized fixture reaches, by equality of bits against the numpy
restatement (tests/collect_ref.py: a stable argsort of the ids plus a bincount), through Engine.partition / partition_collect / group_collect / group_rows.

  1. the partition at 2^20 + 5 elements (several trips of every capped grid, 513 tiles of the gather) with 1, 255, 256, 257, 65 536, 65 537 and 2^20 + 5
     groups: no, one, two and three radix passes -- the pass count is asserted, it is what "a digit every id agrees on costs nothing" means;
  2. one group of m - 1 elements beside a singleton; ids descending so that every element moves; a group without elements between two that have some;
  3. nine columns (two launches over one permutation) mixing the four cell widths, under a filter with gaps, into outputs whose base is only cell-aligned,
     between guard cells: every cell is written, nothing beyond the extents is (outputs and the context's scratch pool poisoned with 0xA5 first);
  4. every (width, misalignment) of the 16-byte store groups around the tile edges 2 047 / 2 048 / 2 049;
  5. what the check refuses: an id outside [0, groups), a row id outside the columns -- refused BEFORE anything is placed (the outputs keep their poison);
  6. Engine.group_collect / group_rows over keys on the dense, the wide dense and the hashed grouping routes, with and without where:."""
import ctypes as C

import numpy as np
import pytest
import torch

import collect_ref as R
from rayforce_amd import _lib as L
from rayforce_amd._lib import RfxError

pytestmark = pytest.mark.gpu

M_BIG = (1 << 20) + 5
TILE = 2048   # COL_TILE
GUARD = 64    # sentinel cells on either side of every output
POISON = 0xA5


def dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def poison_pool(eng, nbytes):
    """leave 0xA5 in a block of the context's pool, so that scratch taken next does not start out as zeros"""
    p = C.c_void_p()
    L.check(eng.lib.rfx_hip_malloc(eng._ctx, C.byref(p), nbytes), "malloc")
    L.check(eng.lib.rfx_hip_memset(eng._ctx, p, POISON, nbytes), "memset")
    eng.sync()
    L.check(eng.lib.rfx_hip_free(eng._ctx, p), "free")


def check_partition(eng, gid, groups, passes=None):
    p0 = eng.xstat(L.RFX_XSTAT_COLLECT_PASSES)
    offsets, perm = eng.partition(dev(eng, gid), groups)
    ran = eng.xstat(L.RFX_XSTAT_COLLECT_PASSES) - p0
    want_off, want_perm = R.partition(gid, groups)
    assert np.array_equal(offsets.cpu().numpy(), want_off)
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    if passes is not None:
        assert ran == passes, (groups, ran)


@pytest.mark.parametrize("groups,passes", [(1, 0), (255, 1), (256, 1), (257, 2), (65536, 2), (65537, 3), (M_BIG, 3)])
def test_partition_group_counts(eng, groups, passes):
    i = np.arange(M_BIG, dtype=np.int64)
    gid = (i * 7919 + 13) % groups  # (7919 is prime to every count here: all groups occur when groups <= m)
    assert len(np.unique(gid)) == groups
    poison_pool(eng, M_BIG * 24)
    check_partition(eng, gid, groups, passes)


def test_partition_heavy_group_and_singleton(eng):
    for at in (0, M_BIG // 2, M_BIG - 1):  # where the singleton sits
        gid = np.zeros(M_BIG, dtype=np.int64)
        gid[at] = 1
        check_partition(eng, gid, 2, 1)


def test_partition_descending_ids_move_every_element(eng):
    gid = np.arange(M_BIG - 1, -1, -1, dtype=np.int64)
    assert (R.partition(gid, M_BIG)[1] != np.arange(M_BIG)).sum() == M_BIG - 1  # (all but the middle one of an odd count)
    check_partition(eng, gid, M_BIG, 3)


def test_partition_groups_without_elements(eng):
    gid = np.array([5, 0, 5, 9, 0, 5], dtype=np.int64)
    check_partition(eng, gid, 12)  # groups 1-4, 6-8, 10-11 are empty ranges
    i = np.arange(70001, dtype=np.int64)
    check_partition(eng, (i % 3) * 1000, 100000)  # long runs of empty groups
    offsets, perm = eng.partition(eng.empty(0), 5)
    assert offsets.cpu().tolist() == [0] * 6 and perm.numel() == 0
    offsets, perm = eng.partition(eng.empty(0), 0)
    assert offsets.cpu().tolist() == [0] and perm.numel() == 0


def guarded(eng, m, dtype, shift):
    """a poisoned buffer and the view of m cells that starts `shift` cells past a 16-byte boundary, GUARD cells inside"""
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    buf = torch.empty(m + 2 * GUARD + per16, dtype=dtype, device=eng.device)
    buf.view(torch.uint8).fill_(POISON)
    at = GUARD + shift
    assert (buf.data_ptr() % 16) == 0
    return buf, buf[at:at + m], at


def assert_guards(buf, at, m):
    raw = buf.view(torch.uint8).cpu().numpy()
    w = buf.element_size()
    assert (raw[:at * w] == POISON).all() and (raw[(at + m) * w:] == POISON).all(), "a write outside the output's extent"


NINE = ["i64", "u8", "i32", "f64", "i16", "b8", "timestamp", "date", "u8"]


def test_nine_columns_filter_with_gaps_cell_aligned_outputs(eng):
    m = M_BIG
    n = 3 * m + 2
    rows = np.arange(m, dtype=np.int64) * 3 + 1  # every third row: a filter with gaps
    rows[-1] = n - 1
    gid = (np.arange(m, dtype=np.int64) * 31) % 1000
    cols = [R.value_column(k, n, seed) for seed, k in enumerate(NINE)]
    bufs = [guarded(eng, m, torch.from_numpy(c[:1]).dtype, 1 + k % 3) for k, c in enumerate(cols)]
    poison_pool(eng, m * 24)
    l0 = eng.xstat(L.RFX_XSTAT_COLLECT_LAUNCHES)
    offsets, outs, rows_out = eng.partition_collect(dev(eng, gid), 1000, [dev(eng, c) for c in cols], rows=dev(eng, rows), outs=[b[1] for b in bufs], want_rows=True)
    assert eng.xstat(L.RFX_XSTAT_COLLECT_LAUNCHES) - l0 == 2  # ten outputs: eight, then two, over the same permutation
    want_off, want_cells, want_rows = R.collect(gid, 1000, cols, rows)
    assert np.array_equal(offsets.cpu().numpy(), want_off)
    assert np.array_equal(rows_out.cpu().numpy(), want_rows)
    for (buf, view, at), got, want in zip(bufs, outs, want_cells):
        assert got.data_ptr() == view.data_ptr() and got.data_ptr() % 16 != 0
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))  # bits, not values: -0.0 and NaN payloads alike
        assert_guards(buf, at, m)


@pytest.mark.parametrize("kind", ["u8", "i16", "i32", "f64"])
def test_store_groups_at_tile_edges(eng, kind):
    """every misalignment of the output against the 16-byte store groups, at sizes around the tile"""
    width = np.dtype(R.DTYPES[kind]).itemsize
    for m in (1, 15, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        col = R.value_column(kind, m, 3)
        gid = (np.arange(m, dtype=np.int64) * 5) % 7
        want_off, (want,), _ = R.collect(gid, 7, [col])
        for shift in sorted({0, 1, 16 // width - 1}):
            buf, view, at = guarded(eng, m, torch.from_numpy(col[:1]).dtype, shift)
            offsets, (got,), _ = eng.partition_collect(dev(eng, gid), 7, [dev(eng, col)], outs=[view])
            assert np.array_equal(offsets.cpu().numpy(), want_off)
            assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), (m, shift)
            assert_guards(buf, at, m)


@pytest.mark.parametrize("bad", [7, -1, R.NULL_I64, 1 << 40])
def test_bad_group_id_is_refused_before_anything_is_placed(eng, bad):
    m = 5000
    gid = (np.arange(m, dtype=np.int64) * 5) % 7
    gid[m - 3] = bad
    col = R.value_column("i64", m)
    buf, view, at = guarded(eng, m, torch.int64, 0)
    with pytest.raises(RfxError, match="a group id outside"):
        eng.partition_collect(dev(eng, gid), 7, [dev(eng, col)], outs=[view])
    eng.sync()
    assert (buf.view(torch.uint8).cpu().numpy() == POISON).all()
    with pytest.raises(RfxError, match="a group id outside"):
        eng.partition(dev(eng, gid), 7)


@pytest.mark.parametrize("bad", [20000, -1, R.NULL_I64])
def test_bad_row_id_is_refused_before_anything_is_gathered(eng, bad):
    m, n = 5000, 20000
    gid = (np.arange(m, dtype=np.int64) * 5) % 7
    rows = np.arange(m, dtype=np.int64) * 4
    rows[17] = bad
    buf, view, at = guarded(eng, m, torch.int64, 0)
    with pytest.raises(RfxError, match="a row id outside the columns"):
        eng.partition_collect(dev(eng, gid), 7, [dev(eng, R.value_column("i64", n))], rows=dev(eng, rows), outs=[view])
    eng.sync()
    assert (buf.view(torch.uint8).cpu().numpy() == POISON).all()


def test_two_shards_refuse(built):
    from rayforce_amd.engine import Engine
    e = Engine(0, shards=2)
    try:
        k = torch.arange(4096, dtype=torch.int64, device=e.device) % 5
        with pytest.raises(RfxError, match="collect over a sharded table"):
            e.partition(k, 5)
        with pytest.raises(RfxError, match="collect over a sharded table"):
            e.group_rows(k)
        with pytest.raises(RfxError, match="collect over a sharded table"):
            e.group_collect(k, {"v": k})
    finally:
        e.close()


# ---- Engine.group_collect / group_rows: the groups in first-occurrence order, from the grouping routes the planner takes ----
ROUTES = {"dense": dict(base=-40, stride=1), "wide": dict(base=10, stride=1000), "sparse": dict(base=-(1 << 50), stride=(1 << 40) + 12345)}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n,groups,shape", [(1, 1, "cycle"), (65, 2, "heavy"), (4097, 257, "cycle"), (70001, 65537, "cycle"), (4097, 4097, "own")])
def test_group_collect_and_rows(eng, route, n, groups, shape):
    key = R.key_column(n, groups, shape, **ROUTES[route])
    kinds = ["i64", "f64", "i32", "i16", "u8", "b8"]
    cols = {k: R.value_column(k, n, s) for s, k in enumerate(kinds)}
    table = {"k": dev(eng, key), **{k: dev(eng, c) for k, c in cols.items()}}
    a = R.value_column("i64", n, 9) % 100
    table["a"] = dev(eng, a)
    for where, mask in ((None, None), (("<", "a", 37), a < 37), (("<", "a", -1), a < -1), ((">=", "a", -(1 << 62)), a >= -(1 << 62))):
        want_keys, want_off, want_cells, want_rows = R.group_collect(key, [cols[k] for k in kinds], mask)
        keys, offsets, cells = eng.group_collect("k", kinds, where, table)
        assert np.array_equal(keys.cpu().numpy(), want_keys), "groups are not in first-occurrence order"
        assert np.array_equal(offsets.cpu().numpy(), want_off)
        for k, want in zip(kinds, want_cells):
            got = cells[k].cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (k, where)
        keys, offsets, rows = eng.group_rows("k", where, table)
        assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(offsets.cpu().numpy(), want_off)
        assert np.array_equal(rows.cpu().numpy(), want_rows)
