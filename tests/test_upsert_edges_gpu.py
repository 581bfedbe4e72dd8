"""upsert's plan, place and fill kernels (rayforce_amd/csrc/rfx_upsert.hip) beyond their first tiles, by equality of bits against the numpy restatement of
their contracts (tests/upsert_ref.py plan / place / fill; tests/test_upsert_cpu.py pins it to the per-cell replay and to the compiled reference's fixture).

What the fixture's 6 000 batch rows cannot reach: k_up_scan with more than one tile per thread (more than 256 tiles of 2 048 rows), k_up_clear's second and
third trip (more rows than its capped grid has threads), a scratch W that an earlier call left full of larger winners, hundreds of thousands of atomicMax on
one address, k_up_dest's carry over hundreds of tiles, the matched stores of 1-, 2- and 4-byte cells (the planner refuses such calls: the flat entry point
takes them), k_up_fill at every (width, address & 15, cells), and the one-key find and the multi-key join index inside upsert over 3e5 .. 1e6 table rows.

  1. the flat entry points rfx_hip_upsert_plan / _place / _fill on the Engine's context over torch tensors;
  2. Engine.upsert / Engine.insert and the operator door on cases of the fixture's vocabulary with m > 524 288 -- the restatement is the reference.
Every test computes and asserts, from its inputs alone, the condition that makes it reach its path."""
import ctypes as C

import numpy as np
import pytest
import torch

import upsert_door as D
import upsert_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H

pytestmark = pytest.mark.gpu

TILE, BLOCK, WAVE = 2048, 256, 64  # UP_TILE, RFX_BLOCK, RFX_WAVE
BLOCKS_PER_CU = 2                  # the context's default (rfx_ctx.hip); no test of the suite tunes it
RFX_EINVAL = -2
GUARD = 64                         # sentinel cells on either side of every output
SENTINEL = 0xA5
NULL = R.NULL_I64


def tiles(m):
    return (m + TILE - 1) // TILE


def scan_chunk(m, thread):
    """k_up_scan: the tiles [b0, b1) thread `thread` sums, and `per`"""
    nblk = tiles(m)
    per = (nblk + BLOCK - 1) // BLOCK
    b0 = thread * per
    return b0, min(b0 + per, nblk), per


def clear_threads(eng):
    """the threads of k_up_clear's capped grid (rfx_stream_grid): 4 * CUs * workgroups per CU * 256"""
    return 4 * torch.cuda.get_device_properties(eng.device).multi_processor_count * BLOCKS_PER_CU * BLOCK


def dev_plan(eng, idx, n):
    d_idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(eng.device)
    dest = torch.full((len(idx),), -99, dtype=torch.int64, device=eng.device)
    a = C.c_int64(-1)
    L.check(eng.lib.rfx_hip_upsert_plan(eng._ctx, d_idx.data_ptr(), len(idx), n, dest.data_ptr(), C.byref(a)), "upsert_plan")
    return dest.cpu().numpy(), int(a.value)


def check_plan(eng, idx, n, what):
    dest, a = dev_plan(eng, idx, n)
    want, wa = R.plan(idx, n)
    bad = np.flatnonzero(dest != want)
    assert bad.size == 0, (what, int(bad.size), bad[:5], idx[bad[:5]], dest[bad[:5]], want[bad[:5]])
    assert a == wa, (what, a, wa)
    return dest, a


# ---------------------------------------------------------------- plan: tile and scan edges
N_PLAN = 100_003
MS = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 524_287, 524_288, 524_289, 526_337, 1_572_869)
NONE_VALUES = R.HOSTILE + (N_PLAN, N_PLAN + 5, 2**62)


def idx_none(m, n, rng):
    return np.array(NONE_VALUES, dtype=np.int64)[np.arange(m) % len(NONE_VALUES)]


def idx_all(m, n, rng):
    return np.arange(m, dtype=np.int64) * 7 % n  # (7 and n coprime: distinct rows while m <= n, then every row again)


def idx_half(m, n, rng):
    none = np.array(NONE_VALUES, dtype=np.int64)[rng.integers(0, len(NONE_VALUES), m)]
    return np.where(rng.random(m) < 0.5, rng.integers(0, n, m), none)


def idx_runs(m, n, rng):
    j = np.arange(m, dtype=np.int64)
    return np.where(j // 3000 % 2 == 0, j % n, NULL)  # runs longer than a tile; 3 000 = 46 * 64 + 56: every boundary inside a wavefront


MAKERS = {"none": idx_none, "all": idx_all, "half": idx_half, "runs": idx_runs}


def test_the_sizes_reach_the_scan_and_the_clear(eng):
    assert np.gcd(7, N_PLAN) == 1 and 3000 % WAVE != 0 and 3000 > TILE
    assert [tiles(m) for m in MS[-5:]] == [256, 256, 257, 258, 769]
    assert [scan_chunk(m, 0)[2] for m in MS[-5:]] == [1, 1, 2, 2, 4]
    assert 524_289 - 256 * TILE == 1  # the last tile holds one row
    assert scan_chunk(524_289, 128) == (256, 257, 2) and scan_chunk(524_289, 129)[0] > 257  # a short chunk, then threads that start past nblk
    assert scan_chunk(1_572_869, 192) == (768, 769, 4) and scan_chunk(1_572_869, 193)[0] > 769
    cap = clear_threads(eng)
    assert 1_572_869 > cap, cap  # k_up_clear takes a second trip
    if cap == 524_288:  # 256 CUs: three full trips and a fourth of five rows
        assert -(-1_572_869 // cap) == 4 and 1_572_869 - 3 * cap == 5


@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_plan_at_tile_and_scan_edges(eng, maker):
    rng = np.random.default_rng(11)
    assert max(tiles(m) for m in MS) > BLOCK and MS[-1] > clear_threads(eng)
    for m in MS:
        idx = MAKERS[maker](m, N_PLAN, rng)
        dest, a = check_plan(eng, idx, N_PLAN, (maker, m))
        hit = (idx >= 0) & (idx < N_PLAN)
        if maker == "none":
            assert a == m and not hit.any()
        elif maker == "all":
            assert a == 0 and hit.all() and (int((dest < 0).sum()) > 0) == (m > N_PLAN)
        elif m >= (64 if maker == "half" else 3001):
            assert 0 < a < m
        if maker == "runs" and m > 6000:  # matched and unmatched rows within one wavefront's ballot
            assert hit[2999] and not hit[3000] and 2999 // WAVE == 3000 // WAVE


@pytest.mark.parametrize("m", [1, 2049, 526_337])
def test_plan_over_a_table_of_no_rows(eng, m):
    """n = 0: no scratch W, no clear; whatever idx holds, every row is appended in order"""
    idx = np.array(R.HOSTILE + (0, 5, 2**62), dtype=np.int64)[np.arange(m) % 6]
    dest, a = check_plan(eng, idx, 0, m)
    assert a == m and np.array_equal(dest, np.arange(m))
    assert (m == 526_337) == (tiles(m) > BLOCK)


# ---------------------------------------------------------------- plan: contention
def test_plan_under_contention_on_a_thousand_rows(eng):
    n, m = 1_000_003, 1_572_869
    rng = np.random.default_rng(9)
    rows = rng.integers(0, 1000, m) * (n // 1000)
    idx = np.where(rng.random(m) < 0.01, -1, rows)
    assert tiles(m) > BLOCK and m > clear_threads(eng)
    writers = np.bincount(idx[idx >= 0] // (n // 1000), minlength=1000)
    assert writers.min() > 1400  # about 1 557 writers per row
    dest, a = check_plan(eng, idx, n, "hot")
    assert (a, int((dest == -1).sum()), int(((dest >= 0) & (dest < n)).sum())) == (15_617, 1_556_252, 1_000)  # (what this seed gives)
    assert a == int((idx < 0).sum())
    again, _ = dev_plan(eng, idx, n)
    assert dest.tobytes() == again.tobytes()


def test_plan_under_contention_on_one_row(eng):
    """one address, half a million atomics, one survivor: the last matched batch row"""
    n, m = 4_097, 526_337
    rng = np.random.default_rng(10)
    idx = np.where(rng.random(m) < 0.01, -1, 5)
    assert tiles(m) > BLOCK and int((idx == 5).sum()) > 500_000
    dest, a = check_plan(eng, idx, n, "one")
    last = int(np.flatnonzero(idx == 5)[-1])
    assert np.flatnonzero(dest == 5).tolist() == [last] and int((dest == -1).sum()) == m - a - 1
    again, _ = dev_plan(eng, idx, n)
    assert dest.tobytes() == again.tobytes()


# ---------------------------------------------------------------- plan: a scratch that an earlier call left full of winners
@pytest.mark.parametrize("second", ["short", "permuted"])
def test_plan_over_a_poisoned_scratch(eng, second):
    """Call A leaves in W, for every table row, a winner above 1 272 000.  Call B, same n (the pool's same size class), names rows whose true winners are
    smaller: a row B did not clear keeps A's winner, atomicMax cannot lower it, and the row's write is lost (dest -1 where plan says the row).  `short`: B has
    600 011 rows, every winner below that; `permuted`: B has A's 1 572 869 rows in a random order, so matched rows lie in the clear's second and third trip
    and about half of the table rows have a smaller winner than A left.
    What this cannot observe: whether the pool really handed A's block back to B -- if it did not, the test passes for another reason."""
    n, ma = 300_007, 1_572_869
    ja = np.arange(ma, dtype=np.int64)
    idx_a = ja % n
    wa = R.winners(idx_a, n)
    assert wa.min() > 1_272_000 and ma > clear_threads(eng)
    if second == "short":
        mb = 600_011
        jb = np.arange(mb, dtype=np.int64)
        idx_b = np.where(jb % 2 == 0, jb * 7 % n, NULL)
    else:
        mb = ma
        idx_b = np.random.default_rng(12).permutation(np.where(ja % 2 == 0, ja * 7 % n, NULL))
    wb = R.winners(idx_b, n)
    stale = (wb >= 0) & (wb < wa)  # the rows whose write a missed clear would lose
    assert tiles(mb) > BLOCK
    if second == "short":
        assert wb.max() < mb < wa.min() and stale.sum() == (wb >= 0).sum() > 290_000
    else:
        cap = clear_threads(eng)
        beyond = stale[idx_b[(np.arange(mb) >= cap) & (idx_b >= 0)]]  # matched rows of a later trip that a missed clear would lose
        assert mb > cap and beyond.sum() > 1000 and stale.sum() > 100_000
    check_plan(eng, idx_a, n, "A")
    check_plan(eng, idx_b, n, "B")


# ---------------------------------------------------------------- place: every width
N_PLACE = 1_001
PLACE_MS = (1, 2, 15, 16, 17, 2047, 2048, 2049, 4097, 6143)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def cells(rng, count, width):
    return rng.integers(0, 256, count * width, dtype=np.uint8).view(UINT[width])


def place_dest(kind, m, n, rng):
    """-> (dest or None, total, appends_only)"""
    if kind == "insert":
        return None, n + m, 0
    idx = np.where(rng.random(m) < 0.6, rng.integers(0, n, m) // 3, NULL)  # matched rows with repeats
    if m <= 2:
        idx[0] = 7  # (a matched row in the smallest batches too)
    dest, a = R.plan(idx, n)
    total = n + a
    if kind == "extras":  # destinations the place must ignore
        dest = dest.copy()
        for k, v in enumerate((-1, total, total + 5)):
            dest[k * m // 3] = v
    return dest, total, int(kind == "appends_only")


def run_place(eng, cols, dest, m, n, total, rng, what):
    """cols: [(width, appends_only, offset cells)].  Every output lies inside a larger tensor, GUARD sentinel cells on either side, the result pointer at
    GUARD + offset cells: cell-aligned only.  The whole tensor is compared."""
    pc = (L.UpsertCol * len(cols))()
    keep, wants = [], []
    d_dest = torch.from_numpy(dest).to(eng.device) if dest is not None else None
    assert d_dest is None or d_dest.data_ptr() % 16 == 0
    for k, (width, ao, off) in enumerate(cols):
        batch = cells(rng, m, width)
        whole = np.full(GUARD + off + total + GUARD, SENTINEL * 0x0101010101010101 & (2**(8 * width) - 1), dtype=UINT[width])
        whole[GUARD + off:GUARD + off + total] = cells(rng, total, width)
        d_batch, d_whole = torch.from_numpy(batch.view(np.uint8)).to(eng.device), torch.from_numpy(whole.view(np.uint8)).to(eng.device)
        assert d_batch.data_ptr() % 16 == 0 and d_whole.data_ptr() % 16 == 0
        pc[k].d_batch, pc[k].d_out, pc[k].width, pc[k].appends_only = d_batch.data_ptr(), d_whole.data_ptr() + (GUARD + off) * width, width, ao
        R.place([whole[GUARD + off:GUARD + off + total]], [batch], dest, n, total, [ao])
        keep.append((d_batch, d_whole))  # (both stay allocated until the launch has run)
        wants.append(whole)
    L.check(eng.lib.rfx_hip_upsert_place(eng._ctx, pc, len(cols), d_dest.data_ptr() if d_dest is not None else None, m, n, total), "upsert_place")
    eng.sync()
    for k, ((_d_batch, d_whole), want) in enumerate(zip(keep, wants)):
        got = d_whole.cpu().numpy().view(want.dtype)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, k, cols[k], int(bad.size), bad[:5] - GUARD - cols[k][2], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_place_every_width(eng, width):
    rng = np.random.default_rng(13 + width)
    narrow_matched = 0
    for m in PLACE_MS:
        for kind in ("insert", "plan", "appends_only", "extras"):
            dest, total, ao = place_dest(kind, m, N_PLACE, rng)
            if dest is not None:
                matched = int(((dest >= 0) & (dest < N_PLACE)).sum())
                assert matched >= 1 or (kind == "extras" and m < 15), (m, kind)  # matched stores present (appends_only: present and to be left alone)
                narrow_matched += matched if kind != "appends_only" else 0
                if kind == "extras":
                    assert (dest == total).any() or (dest == total + 5).any() or m == 1
            for off in (0, 1, 3):
                run_place(eng, [(width, ao, off)], dest, m, N_PLACE, total, rng, (width, m, kind, off))
    assert narrow_matched > 1000 and tiles(max(PLACE_MS)) == 3


def test_place_eight_columns_of_mixed_widths_in_one_launch(eng):
    rng = np.random.default_rng(17)
    m = 6143
    dest, total, _ = place_dest("plan", m, N_PLACE, rng)
    cols = [(8, 0, 1), (1, 0, 3), (4, 1, 0), (2, 0, 1), (8, 1, 0), (2, 1, 3), (1, 1, 0), (4, 0, 3)]
    assert len(cols) == L.RFX_MAX_COLS and {w for w, _a, _o in cols} == {1, 2, 4, 8}
    run_place(eng, cols, dest, m, N_PLACE, total, rng, "mixed")


def test_place_refuses_what_its_contract_excludes(eng):
    """rfx_hip.h: 1 .. RFX_MAX_COLS columns per launch; batch columns 16-byte aligned; total = n + at most m appended rows; d_dest NULL means total = n + m"""
    n, m = 100, 64
    batch, out = torch.zeros(m + 2, dtype=torch.int64, device=eng.device), torch.full((n + m,), 3, dtype=torch.int64, device=eng.device)
    dest = torch.arange(n, n + m, dtype=torch.int64, device=eng.device)

    def call(ncols, batch_ptr, d_dest, total):
        pc = (L.UpsertCol * 9)()
        for k in range(9):
            pc[k].d_batch, pc[k].d_out, pc[k].width, pc[k].appends_only = batch_ptr, out.data_ptr(), 8, 0
        return eng.lib.rfx_hip_upsert_place(eng._ctx, pc, ncols, d_dest, m, n, total)

    assert L.RFX_MAX_COLS == 8 and batch.data_ptr() % 16 == 0
    assert call(9, batch.data_ptr(), dest.data_ptr(), n + m) == RFX_EINVAL
    assert call(1, batch.data_ptr() + 8, dest.data_ptr(), n + m) == RFX_EINVAL
    assert call(1, batch.data_ptr(), dest.data_ptr(), n - 1) == RFX_EINVAL
    assert call(1, batch.data_ptr(), None, n + m - 1) == RFX_EINVAL
    eng.sync()
    assert bool((out == 3).all())  # nothing was launched
    assert call(1, batch.data_ptr(), None, n + m) == L.RFX_OK
    eng.sync()
    assert bool((out[:n] == 3).all()) and bool((out[n:] == 0).all())


# ---------------------------------------------------------------- fill: the alignment matrix
def test_fill_at_every_alignment(eng):
    """(width, address & 15, cells): the head to the first 16-byte boundary, the 16-byte stores, the tail -- bits whose every byte differs, so a slipped
    phase changes bytes"""
    bits, pad = 0x0807060504030201, 256
    launches, shapes = 0, set()
    for width in (1, 2, 4, 8):
        for off in range(16 // width + 1):
            for count in (0, 1, 2, 3, 15, 16, 17, 31, 33, 4097):
                whole = torch.full((pad + off * width + count * width + pad,), SENTINEL, dtype=torch.uint8, device=eng.device)
                assert whole.data_ptr() % 256 == 0
                L.check(eng.lib.rfx_hip_upsert_fill(eng._ctx, whole.data_ptr() + pad + off * width, width, bits, count), "upsert_fill")
                eng.sync()
                want = np.full(whole.numel(), SENTINEL, dtype=np.uint8)
                want[pad + off * width:pad + (off + count) * width] = R.fill(width, bits, count).view(np.uint8)
                got = whole.cpu().numpy()
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (width, off, count, bad[:8] - pad, got[bad[:8]], want[bad[:8]])
                launches += 1
                nbytes = count * width
                head = min(-(off * width) % 16, nbytes)
                shapes.add((head > 0, (nbytes - head) // 16 > 0, (nbytes - head) % 16 > 0, head % 8 != 0))
    assert launches == (17 + 9 + 5 + 3) * 10
    assert {(True, True, True, True), (True, True, True, False), (False, True, False, False), (True, False, False, True), (False, False, True, False)} <= shapes


# ---------------------------------------------------------------- the planner and the door at scale
T4 = [R.I64, R.F64, R.I64, R.TS]
SCALE = [
    dict(name="dense_all", keys=1, types=T4, n=300_007, m=1_572_869, pattern="all", route="dense", counts=(1_572_869, 0)),
    dict(name="hash_alt", keys=1, types=T4, n=2**20 + 5, m=1_572_869, pattern="alt", route="hash"),
    dict(name="small_table_dups", keys=1, types=T4, n=4_097, m=526_337, pattern="dups", route="dense", counts=(263_170, 263_167), door=True),
    dict(name="hot", keys=1, types=T4, n=1_000_003, m=1_572_869, pattern="hot", route="hash"),
    dict(name="one", keys=1, types=[R.I64, R.F64], n=4_097, m=526_337, pattern="one", route="dense"),
    dict(name="keys3_tdup", keys=3, types=[R.I64, R.TS, R.I64, R.F64, R.TS], n=500_009, m=530_003, pattern="alt", tdup=1, counts=(265_002, 265_001)),
    dict(name="keys2_runs", keys=2, types=[R.I64, R.TS, R.F64, R.I64], n=500_009, m=530_003, pattern="runs", tdup=1),
    dict(name="sparse_dict_missing", keys=1, form="dict", types=T4, n=300_007, m=600_011, pattern="runs", sparse=1, given=[3, 0, 1], route="hash",
         counts=(300_005, 300_006), door=True),
    dict(name="short_list", keys=1, types=[R.I64, R.F64, R.I64, R.F64], n=300_007, m=600_011, pattern="alt", given=[0, 1, 2], route="dense"),
    dict(name="none_every_width", keys=1, types=[R.I64, R.F64, R.I32, R.I16, R.B8], n=4_097, m=526_337, pattern="none", route="disjoint", counts=(0, 526_337)),
    dict(name="insert_every_width", verb="insert", keys=0, types=[R.I64, R.F64, R.I32, R.I16, R.B8, R.U8], n=4_097, m=526_337, pattern="none"),
]
SCALE = [dict(dict(verb="upsert", form="list", given=list(range(len(c["types"])))), **c) for c in SCALE]


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0
    return o


def reach(c, counts):
    """what the case is there for, from its description and the restatement's counts"""
    n, m = c["n"], c["m"]
    assert m > 524_288 and tiles(m) > BLOCK, c["name"]
    if "counts" in c:
        assert (counts["matched"], counts["appended"]) == c["counts"], c["name"]
    if c["verb"] == "insert":
        return
    refs = R.batch_refs(c["pattern"], n, m)
    # (tdup: table row 10 carries row 3's key tuple, so row 10's own tuple is in no table row: a batch row that names it is new)
    assert counts["matched"] == int(((refs < n) & ~((refs == 10) & bool(c.get("tdup")))).sum()), c["name"]
    if c["name"] == "dense_all":
        assert 3 * (n - 1) + 1 <= 2**20 and counts["appended"] == 0  # the table's key range: find's dense route; key columns take no place launch
    if c["name"] == "small_table_dups":
        assert counts["matched"] // n >= 64  # writers per table row
    if c["name"] == "hot":
        assert len(np.unique(refs[refs < n])) == 1000 and counts["matched"] > 1500 * 1000
    if c["name"] == "one":
        assert counts["matched"] == (m + 1) // 2
    if c.get("tdup"):
        assert (refs == 3).any()  # a batch row names the tuple that table rows 3 and 10 both carry: the first of them answers
    if c["name"] == "sparse_dict_missing":
        assert 2 not in c["given"] and c["form"] == "dict" and counts["matched"] > 0  # a null vector of m cells; matched rows take the null
    if c["name"] == "short_list":
        assert 3 not in c["given"] and n % 2 == 1 and counts["appended"] > 16  # the appended nulls start at an odd 8-byte cell: a head before the 16-byte stores
    if c["name"] == "none_every_width":
        assert {np.dtype(R.DTYPE[tp]).itemsize for tp in c["types"]} == {1, 2, 4, 8}


@pytest.mark.parametrize("name", [c["name"] for c in SCALE])
def test_the_planner_at_scale(eng, name):
    c = next(c for c in SCALE if c["name"] == name)
    counts = {}
    c = dict(c, out=R.answer(c, counts))
    reach(c, counts)
    if c["keys"] == 1:  # upsert's index step does not record its route: the same find, asked directly
        table, batch = R.inputs(c)
        tk, bk = table[0], batch[c["given"].index(0)]
        assert R.find_route(tk, bk) == c["route"], (name, R.find_route(tk, bk))
        got = eng.find(torch.from_numpy(tk).to(eng.device), torch.from_numpy(bk).to(eng.device)).cpu().numpy()
        assert eng.last_set_route == c["route"], (name, eng.last_set_route)
        assert np.array_equal(np.where(got == NULL, -1, got), R.index([tk], [bk], 1)), name
    stats = (L.RFX_XSTAT_UPSERTS, L.RFX_XSTAT_UPSERT_MATCHED, L.RFX_XSTAT_UPSERT_APPENDED, L.RFX_XSTAT_INSERTS)
    before = [eng.xstat(s) for s in stats]
    D.check_engine(eng, c)
    want = [0, 0, 0, 1] if c["verb"] == "insert" else [1, counts["matched"], counts["appended"], 0]
    assert [eng.xstat(s) - b for s, b in zip(stats, before)] == want, name


@pytest.mark.parametrize("name", [c["name"] for c in SCALE if c.get("door")])
def test_the_door_at_scale(ops, name):
    c = next(c for c in SCALE if c["name"] == name)
    counts = {}
    c = dict(c, out=R.answer(c, counts))
    reach(c, counts)
    try:
        D.check_door(ops, c)
        assert ops.rfx_last_upsert_on_gpu() == 1, name
    finally:
        ops.rfx_cache_clear()
