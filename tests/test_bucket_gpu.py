"""The bucket verbs on the GPU -- xrank, xbar, within, floor, ceil, round, neg -- by equality of bits: every case of the reference's fixture
(tests/golden/bucket_golden.npz) through the Engine and through the C door, the shapes handed back with their reasons, the attribute short-cut,
the element-wise verbs over 2 and 3 shards, and by: (xbar ...) through rfx_select as it answered before."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bucket_door as D
import bucket_ref as B
from oracle import rfo
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = B.load_cases()
VERBS = ["xrank", "xbar", "within", "floor", "ceil", "round", "neg"]
ELEMENTWISE = VERBS[1:]


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0  # standalone host: nothing behind the door to hand a shape to
    return o


@pytest.mark.parametrize("verb", VERBS)
def test_fixture_through_the_engine(eng, verb):
    maps = eng.xstat(L.RFX_XSTAT_BUCKET_MAPS)
    ran = 0
    for c in CASES:
        if c["verb"] == verb:
            D.check_engine(eng, c)
            ran += len(c["out"]) > 0 or verb != "xrank"
    assert ran
    if verb != "xrank":
        assert eng.xstat(L.RFX_XSTAT_BUCKET_MAPS) - maps == ran


@pytest.mark.parametrize("verb", VERBS)
def test_fixture_through_the_door(ops, verb):
    for c in CASES:
        if c["verb"] == verb:
            D.check_door(ops, c)


def refused(ops, r, reason):
    assert r and H.is_error(r), reason
    assert ops.rfx_last_bucket_on_gpu() == 0, reason
    assert reason in ops.rfx_ops_last_error().decode(), (reason, ops.rfx_ops_last_error().decode())
    assert "no host function" in H.error_text(r)
    ops.rfx_host_drop(r)


def test_shapes_outside_the_device_path_are_handed_back(ops):
    i64v = D.host_vector(ops, np.arange(10, dtype=np.int64), B.I64)
    f64v = D.host_vector(ops, np.arange(10, dtype=np.float64), B.F64)
    ten = D.host_atom(ops, 10, B.I64)
    # xrank
    refused(ops, ops.rfx_xrank(D.host_vector(ops, np.arange(10, dtype=np.int64), 6), ten), "key type")  # SYMBOL keys
    refused(ops, ops.rfx_xrank(D.host_vector(ops, np.arange(10, dtype=np.int32), B.I32), ten), "key type")  # 4-byte keys
    refused(ops, ops.rfx_xrank(i64v, D.host_atom(ops, 0, B.I64)), "domain")
    refused(ops, ops.rfx_xrank(i64v, D.host_atom(ops, -3, B.I32)), "domain")
    refused(ops, ops.rfx_xrank(i64v, D.host_atom(ops, 2.0, B.F64)), "bucket count type")
    refused(ops, ops.rfx_xrank(i64v, D.host_vector(ops, np.array([10], np.int64), B.I64)), "bucket count type")
    refused(ops, ops.rfx_xrank(D.host_vector(ops, np.arange(3, dtype=np.int64), B.I64), D.host_atom(ops, 2**62, B.I64)), "63 bits")
    # xbar
    refused(ops, ops.rfx_xbar(ten, D.host_atom(ops, 3, B.I64)), "atom and atom")
    refused(ops, ops.rfx_xbar(i64v, D.host_vector(ops, np.arange(9, dtype=np.int64), B.I64)), "length")
    refused(ops, ops.rfx_xbar(D.host_vector(ops, np.arange(10, dtype=np.int64), 6), ten), "operand types")
    refused(ops, ops.rfx_xbar(D.host_vector(ops, np.arange(10, dtype=np.int32), B.DATE), D.host_atom(ops, 2.0, B.F64)), "operand types")
    cells = torch.arange(16, dtype=torch.int64, device="cuda")  # behind the device-column handles below (the door refuses them before it reads a cell)

    def handle(tp, n):
        import ctypes as C
        return ops.rfx_host_device_vector(tp, n, (C.c_void_p * 1)(cells.data_ptr()), 1)
    refused(ops, ops.rfx_xbar(handle(B.DATE, 10), ten), "a 4-byte device column")
    refused(ops, ops.rfx_xbar(D.host_vector(ops, np.arange(10, dtype=np.int32), B.I32), handle(B.I32, 10)), "a 4-byte device column")
    # floor / ceil / round: the integer arms are clone_obj, atoms run no kernel
    for verb in ("floor", "ceil", "round"):
        refused(ops, getattr(ops, "rfx_" + verb)(i64v), "not an F64 vector")
        refused(ops, getattr(ops, "rfx_" + verb)(D.host_atom(ops, 1.5, B.F64)), "an atom")
    # neg
    refused(ops, ops.rfx_neg(D.host_vector(ops, np.ones(10, np.int8), 1)), "not an I32 / I64 / F64 vector")
    refused(ops, ops.rfx_neg(D.host_vector(ops, np.arange(10, dtype=np.int64), B.TS)), "not an I32 / I64 / F64 vector")
    refused(ops, ops.rfx_neg(ten), "an atom")
    refused(ops, ops.rfx_neg(handle(B.I32, 10)), "a 4-byte device column")
    # within
    rng2 = D.host_vector(ops, np.array([1, 5], np.int64), B.I64)
    refused(ops, ops.rfx_within(f64v, rng2), "2-cell I64 vector")
    refused(ops, ops.rfx_within(i64v, D.host_vector(ops, np.array([1, 5, 9], np.int64), B.I64)), "2-cell I64 vector")
    refused(ops, ops.rfx_within(D.host_vector(ops, np.arange(10, dtype=np.int64), B.TS), rng2), "2-cell I64 vector")
    refused(ops, ops.rfx_within(i64v, handle(B.I64, 2)), "2-cell I64 vector")  # a range that is a device-column handle
    # ... and a device shape right after answers again
    r = ops.rfx_within(i64v, rng2)
    assert not H.is_error(r) and ops.rfx_last_bucket_on_gpu() == 1 and D.result_cells(r).tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0, 0]


def test_host_functions_are_bound_by_name(ops):
    for name in ("xrank", "xbar", "floor", "ceil", "round", "neg"):
        f = ops.rfx_host_fn(name.encode())
        assert f, name
    import ctypes as C
    xb = ops.rfx_host_fn(b"xbar")
    assert C.c_int64.from_address(H.payload(xb) - 8).value == C.cast(ops.rfx_xbar, C.c_void_p).value  # the verb, not a stub


def test_xrank_equals_rank_times_n_over_len(eng):
    rng = np.random.default_rng(11)
    n = 2**20 + 5
    for keys, nb in ((rng.integers(0, 1_000_000, n), 10), (rng.integers(-(2**63), 2**63 - 1, n), 7), (rng.standard_normal(n), 100)):
        col = eng.column(keys)
        perm = eng.sort_index(col)
        rank = torch.empty_like(perm)
        rank[perm] = torch.arange(n, device=perm.device)
        before = eng.xstat(L.RFX_XSTAT_XRANKS), eng.xstat(L.RFX_XSTAT_XRANK_SORTED)
        got = eng.xrank(col, nb)
        assert torch.equal(got, (rank * nb) // n)
        assert eng.xstat(L.RFX_XSTAT_XRANKS) - before[0] == 1 and eng.xstat(L.RFX_XSTAT_XRANK_SORTED) == before[1]


@pytest.mark.parametrize("n", [1, 65, 4097, 2**20 + 5])
def test_attribute_short_cut_is_taken_and_agrees_with_the_sorted_route(eng, n):
    rng = np.random.default_rng(n)
    up = np.cumsum(rng.integers(1, 1000, n))  # strictly ascending: the sorted route's ranks are the positions
    for cells, attr in ((up, "asc"), (up[::-1].copy(), "desc")):
        col = eng.column(cells)
        for nb in (1, 3, 10, n, 2 * n + 1):
            before = eng.xstat(L.RFX_XSTAT_XRANK_SORTED), eng.xstat(L.RFX_XSTAT_SORTS)
            short = eng.xrank(col, nb, attr)
            assert eng.xstat(L.RFX_XSTAT_XRANK_SORTED) - before[0] == 1 and eng.xstat(L.RFX_XSTAT_SORTS) == before[1]  # counted, and no sort ran
            assert torch.equal(short, eng.xrank(col, nb)), (n, attr, nb)
            assert eng.xstat(L.RFX_XSTAT_SORTS) - before[1] == 1


@pytest.mark.parametrize("shards", [2, 3])
def test_elementwise_verbs_over_shards_through_the_engine(built, shards):
    e = Engine(0, shards=shards)
    try:
        for c in CASES:
            if c["verb"] in ELEMENTWISE and len(c["out"]) in (4097, 20011):
                D.check_engine(e, c)
        with pytest.raises(RfxError, match="xrank over a sharded table"):
            e.xrank(torch.arange(4097, device="cuda:0"), 10)
    finally:
        e.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_verbs_wait_for_the_kernels_that_made_their_operands(built, shards):
    """shards 1.. run on streams of their own, which do not wait for torch's: an operand a torch kernel is still writing when the verb is called
    has to be complete before any shard reads it.  Each operand below ends a chain of torch kernels over 2^23 rows, enqueued right before the
    call with nothing waited for; the expected cells come from the same chains on the host."""
    n = 2**23 + 5
    rng = np.random.default_rng(shards)
    a, b = rng.integers(-(2**20), 2**20, n), rng.integers(1, 2**10, n)
    f = (rng.random(n) - 0.5) * 1e6

    def chain(t):  # (the last shard's rows are the last to be written)
        for _ in range(16):
            t = t * 1
        return t

    e = Engine(0, shards=shards)
    try:
        da, db, df = (torch.from_numpy(v).to(e.device) for v in (a, b, f))
        torch.cuda.synchronize()
        got = e.xbar(chain(da * db), 5)
        assert np.array_equal(got.cpu().numpy(), B.xbar(a * b, B.I64, np.array([5]), B.I64, y_atom=True)[0])
        got = e.floor(chain(df * 0.5))
        assert np.array_equal(B.as_bits(got.cpu().numpy()), B.floor(f * 0.5))
        got = e.neg(chain(da * db))
        assert np.array_equal(got.cpu().numpy(), -(a * b))
        got = e.within(chain(da * db), -1000, 2**24)
        assert np.array_equal(got.cpu().numpy(), B.within(a * b, -1000, 2**24))
    finally:
        e.close()


_SHARDED_DOOR = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import numpy as np
import bucket_door as D
import bucket_ref as B
from rayforce_amd import hostobj as H
ops = H.lib()
assert ops.rfx_host_bind() == 0
ran = 0
for c in B.load_cases():
    if c["verb"] != "xrank" and len(c["out"]) in (4097, 20011):
        D.check_door(ops, c)
        ran += 1
assert ops.rfx_ops_shards() == SHARDS and ran > 20, (ops.rfx_ops_shards(), ran)
r = ops.rfx_xrank(D.host_vector(ops, np.arange(4097, dtype=np.int64), B.I64), D.host_atom(ops, 10, B.I64))
assert H.is_error(r) and ops.rfx_last_bucket_on_gpu() == 0 and "xrank over a sharded table" in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error()
print("BUCKET-DOOR-OK", ran)
'''


@pytest.mark.parametrize("shards", [2, 3])
def test_elementwise_verbs_over_shards_through_the_door(built, shards):
    """RFX_SHARDS=k in a process of its own (the operator layer's shards are fixed at its first call): 4097 and 20011 rows split mid-vector"""
    env = dict(os.environ, RFX_SHARDS=str(shards), HSA_ENABLE_IPC_MODE_LEGACY="0")
    code = f"ROOT = {ROOT!r}\nSHARDS = {shards}\n" + _SHARDED_DOOR
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "BUCKET-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_select_by_xbar_answers_as_before(ops):
    """the by: path buckets its keys with the formula the xbar verb shares (rfx_common.hpp): negative keys, one and two key columns (a null group key
    is the host's, as it was)"""
    n = 300_007
    host = {"k": rfo.gen_i64(n, 4, 4000) - 2000, "a": rfo.gen_i64(n, 2, 1_000_000), "v": rfo.gen_f64(n, 5)}
    q = {"s": ("sum", "a"), "c": ("count", "a"), "m": ("max", "a")}
    for by in ({"b": ("xbar", "k", 10)}, {"b": ("xbar", "a", 1000)}, {"k": "k", "b": ("xbar", "a", 250_000)}):
        tab = H.table(host)
        d = H.select_dict({**q, "by": by}, tab)
        r = ops.rfx_select(d)
        assert r and not H.is_error(r), H.error_text(r)
        assert ops.rfx_last_select_on_gpu() == 1
        got, want = H.table_to_numpy(r), rfo.select({"from": host, **q, "by": by})
        assert list(got) == list(want)
        for name in want:
            assert np.array_equal(got[name], want[name]), (by, name)
        for o in (r, d, tab):
            ops.rfx_host_drop(o)
    # and the verb itself answers the very buckets the keys were grouped by, nulls among them
    host["k"][::997] = -(2**63)
    x = D.host_vector(ops, host["k"], B.I64)
    w = D.host_atom(ops, 10, B.I64)
    r = ops.rfx_xbar(x, w)
    assert not H.is_error(r) and np.array_equal(D.result_cells(r), rfo.xbar(host["k"], 10))
