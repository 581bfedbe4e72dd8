"""The row verbs on the GPU -- filter, take, reverse -- by equality of bits: every case of the reference's fixture (tests/golden/rows_golden.npz) through
the C door over standalone host objects (cells, type code, attributes) and through the Engine, under both write-out forms of the compaction; the shapes
handed back with their reasons; filter over 2 and 3 shards; a predicate tree against a mask against where + at_ids; a mask that is a device handle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rows_door as D
import rows_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_cases()
VERBS = ["filter", "take", "reverse"]
BIG = 2**20 + 5


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0  # standalone host: nothing behind the door to hand a shape to
    return o


@pytest.mark.parametrize("verb", VERBS)
def test_fixture_through_the_door(ops, verb):
    ran = 0
    for c in CASES:
        if c["verb"] == verb and c["host"] is None:
            D.check_door(ops, c)
            ran += 1
            if any(tp == R.I64 for tp, _a, _c in c["cols"]) and len(c["cols"][0][2]) <= 1025:  # (atoms among them)
                D.check_door(ops, c, retype=(R.I64, R.SYMBOL))  # SYMBOL cells are copied as I64 cells are: the same answer under the other type code
    assert ran > 50


@pytest.mark.parametrize("form", [None, "direct", "ring"])
def test_filter_fixture_through_the_engine(eng, form):
    before = eng.xstat(L.RFX_XSTAT_ROWS_FILTERS), eng.xstat(L.RFX_XSTAT_ROWS_IN), eng.xstat(L.RFX_XSTAT_ROWS_OUT)
    ran = rows_in = rows_out = 0
    for c in CASES:
        if c["verb"] == "filter" and c["host"] is None:
            D.check_engine(eng, c, form)
            ran += 1
            rows_in += len(c["mask"])
            rows_out += len(c["out"][0][2])
    assert eng.xstat(L.RFX_XSTAT_ROWS_FILTERS) - before[0] == ran
    assert eng.xstat(L.RFX_XSTAT_ROWS_IN) - before[1] == rows_in and eng.xstat(L.RFX_XSTAT_ROWS_OUT) - before[2] == rows_out


@pytest.mark.parametrize("verb", ["take", "reverse"])
def test_fixture_through_the_engine(eng, verb):
    stat = L.RFX_XSTAT_ROWS_TAKES if verb == "take" else L.RFX_XSTAT_ROWS_REVERSES
    before, ran = eng.xstat(stat), 0
    for c in CASES:
        if c["verb"] == verb and c["host"] is None:
            D.check_engine(eng, c)
            ran += len(c["out"][0][2]) > 0  # (an empty answer launches nothing and is not counted)
    assert eng.xstat(stat) - before == ran


def test_shapes_outside_the_device_path_are_handed_back(ops):
    hosts = [c for c in CASES if c["host"]]
    assert len(hosts) > 30
    for c in hosts:
        D.check_refused(ops, c)
    cells = torch.arange(16, dtype=torch.int64, device="cuda")
    h32 = ops.rfx_host_device_vector(R.DATE, 10, (C.c_void_p * 1)(cells.data_ptr()), 1)
    for r in (ops.rfx_reverse(h32), ops.rfx_take(h32, D.host_atom(ops, 3, R.I64)), ops.rfx_filter(h32, D.host_vector(ops, np.ones(10, np.int8), R.B8))):
        assert H.is_error(r) and ops.rfx_last_rows_on_gpu() == 0 and "a 4-byte device column" in ops.rfx_ops_last_error().decode()
    # ... and a device shape right after answers again
    r = ops.rfx_reverse(D.host_vector(ops, np.arange(5, dtype=np.int64), R.I64, R.ATTR_ASC))
    assert not H.is_error(r) and ops.rfx_last_rows_on_gpu() == 1 and D.cells_of(r).tolist() == [4, 3, 2, 1, 0] and H.header(r).attrs == R.ATTR_DESC


def _case(name, verb, cols, **kw):
    """a case the reference's column files cannot carry, answered by the restatement (which the CPU tests hold to the fixture)"""
    c = dict(name=name, verb=verb, cols=cols, alias=[-1] * len(cols), table=False, atom=False, names=[], mask=None, count=None, host=None)
    c.update(kw)
    c["out"] = R.answer(c)
    return c


def _cells(tp, n, seed):
    rng = np.random.default_rng(seed)
    if tp == R.F64:
        return rng.standard_normal(n)
    if tp == R.B8:
        return rng.integers(0, 2, n).astype(np.int8)
    a = rng.integers(-2**30, 2**30, n).astype(R.DTYPE[tp])
    a[::7] = R.NULL64 if a.dtype == np.int64 else R.NULL32
    return a


@pytest.mark.parametrize("tp", R.ROW_TYPES)
def test_reverse_of_every_type_under_every_attribute(ops, tp):
    """attrs 0, ASC, DESC, DISTINCT | ASC (and DISTINCT alone, DISTINCT | DESC) set on standalone host vectors: the reference's files carry only what its
    own verbs set (ASC / DESC on the sortable types, DISTINCT | ASC on I64)"""
    for attrs in (0, R.ATTR_ASC, R.ATTR_DESC, R.ATTR_DISTINCT | R.ATTR_ASC, R.ATTR_DISTINCT | R.ATTR_DESC, R.ATTR_DISTINCT):
        for n in (0, 1, 65, 129, 4097):
            c = _case(f"reverse_type{tp}_attrs{attrs}_len{n}", "reverse", [(tp, attrs, _cells(tp, n, n + attrs))])
            assert c["out"][0][1] == R.reverse_attrs(attrs) and ((c["out"][0][1] & R.ATTR_DISTINCT) != 0) == ((attrs & R.ATTR_DISTINCT) != 0)
            D.check_door(ops, c)


def test_symbol_atoms_and_vectors(ops):
    sym = [ops.rfx_host_intern(w.encode(), len(w)) for w in ("aa", "bb", "cc", "dd", "ee")]
    atom = [(R.SYMBOL, 0, np.array(sym[2:3], np.int64))]
    for count in (("atom", R.I64, 67), ("atom", R.I32, -5), ("atom", R.I16, 1), ("atom", R.I64, 0), ("range", 0, 9), ("range", -3, 4097)):
        D.check_door(ops, _case(f"take_symbol_atom_{R.count_text(count)}", "take", atom, atom=True, count=count))
    for n in (5, 65, 4097):
        vec = [(R.SYMBOL, 0, np.resize(np.array(sym, np.int64), n))]
        for count in (("atom", R.I64, 3), ("atom", R.I64, -3), ("atom", R.I32, 2 * n + 3), ("atom", R.I16, -(n + 1)), ("range", 1, n), ("range", -2, 7)):
            D.check_door(ops, _case(f"take_symbol_len{n}_{R.count_text(count)}", "take", vec, count=count))
        mask = (np.random.default_rng(n).random(n) < 0.5).astype(np.uint8)
        D.check_door(ops, _case(f"filter_symbol_len{n}", "filter", vec, mask=mask))
        tab = vec + [(R.F64, 0, _cells(R.F64, n, n)), (R.SYMBOL, 0, vec[0][2][::-1].copy())]
        D.check_door(ops, _case(f"filter_symbol_table_len{n}", "filter", tab, mask=mask, table=True, names=["s", "f", "s2"], alias=[-1, -1, -1]))
        D.check_door(ops, _case(f"take_symbol_table_len{n}", "take", tab, count=("atom", R.I64, -(n + 2)), table=True, names=["s", "f", "s2"], alias=[-1, -1, -1]))


def test_engine_take_refuses_a_malformed_range(eng):
    col = torch.arange(10, device=eng.device)
    for count in ((3,), (1, 2, 3), (1, -2)):
        with pytest.raises(RfxError, match="a range is"):
            eng.take(col, count)
    with pytest.raises(RfxError, match="a range is"):
        eng.take(7, (3,))


def test_host_functions_are_bound_by_name(ops):
    for name, fn in (("filter", ops.rfx_filter), ("take", ops.rfx_take), ("reverse", ops.rfx_reverse)):
        f = ops.rfx_host_fn(name.encode())
        assert f and C.c_int64.from_address(H.payload(f) - 8).value == C.cast(fn, C.c_void_p).value, name
        assert H.header(f).type == (101 if name == "reverse" else 102) and H.header(f).attrs == 0


def _table(n, seed):
    rng = np.random.default_rng(seed)
    return {"a": rng.integers(-2**40, 2**40, n), "f": rng.standard_normal(n), "i": rng.integers(-2**31 + 1, 2**31, n).astype(np.int32),
            "b": rng.integers(0, 2, n).astype(np.int8), "k": rng.integers(0, 1000, n)}


@pytest.mark.parametrize("pct", [50, 99])
def test_big_random_masks_equal_the_restatement(eng, pct):
    """2^20 + 5 rows under i.i.d. masks (the fixture holds such masks up to 20011 rows and 1 % at this length), both write-out forms"""
    host = _table(BIG, pct)
    host["i"][::17] = R.NULL32
    mask = (np.random.default_rng(pct + 1).random(BIG) * 100 < pct).astype(np.int8)
    dev = {k: eng.column(v) if v.dtype != np.int32 else torch.from_numpy(v).to(eng.device) for k, v in host.items()}
    for form in ("direct", "ring"):
        got = eng.filter(dev, eng.column(mask), form=form)
        for k, v in host.items():
            assert np.array_equal(R.as_bits(got[k].cpu().numpy()), R.as_bits(R.filter_cells(v, mask))), (form, k)


@pytest.mark.parametrize("shards", [2, 3])
def test_filter_over_shards_equals_one_shard(built, eng, shards):
    e = Engine(0, shards=shards)
    try:
        for c in CASES:
            if c["verb"] == "filter" and c["host"] is None and len(c["mask"]) in (513, 1025, 4097, 20011, BIG):
                for form in ("direct", "ring"):
                    D.check_engine(e, c, form)
        host = _table(20011, shards)
        dev = {k: torch.from_numpy(v).to(e.device) for k, v in host.items()}
        one = {k: torch.from_numpy(v).to(eng.device) for k, v in host.items()}
        tree = ("and", ("<", "k", 700), (">", "f", -0.5))
        got, want = e.filter(dev, tree, dev), eng.filter(one, tree, one)
        for k in host:
            assert torch.equal(got[k].cpu(), want[k].cpu()), k
        with pytest.raises(RfxError, match="take over a sharded table"):
            e.take(dev["a"], 10)
        with pytest.raises(RfxError, match="reverse over a sharded table"):
            e.reverse(dev["a"])
    finally:
        e.close()


@pytest.mark.parametrize("n", [1025, 20011, BIG])
def test_predicate_tree_equals_mask_equals_where_and_at(eng, n):
    host = _table(n, n)
    dev = {k: torch.from_numpy(v).to(eng.device) for k, v in host.items()}
    tree = ("or", ("and", ("<", "k", 300), (">", "f", 0.0)), ("==", "k", 999))
    keep = ((host["k"] < 300) & (host["f"] > 0.0)) | (host["k"] == 999)
    by_tree = eng.filter(dev, tree, dev)
    by_mask = eng.filter(dev, eng.mask_of(tree, dev))
    ids = eng.where(tree, dev)
    for k, v in host.items():
        assert np.array_equal(R.as_bits(by_tree[k].cpu().numpy()), R.as_bits(v[keep])), k
        assert torch.equal(by_tree[k], by_mask[k]), k
        if v.dtype in (np.int64, np.float64):
            assert torch.equal(by_tree[k], eng.at_ids(dev[k], ids)), k


def test_filter_with_a_device_handle_mask(ops):
    n = 20011
    host = _table(n, 7)
    mask = (np.random.default_rng(8).random(n) < 0.3).astype(np.int8)
    dmask = torch.from_numpy(mask).cuda()
    dcol = torch.from_numpy(host["a"]).cuda()
    hm = ops.rfx_host_device_vector(R.B8, n, (C.c_void_p * 1)(dmask.data_ptr()), 1)
    for x, want in ((D.host_vector(ops, host["i"], R.TIME), host["i"]), (ops.rfx_host_device_vector(R.TS, n, (C.c_void_p * 1)(dcol.data_ptr()), 1), host["a"])):
        r = ops.rfx_filter(x, hm)
        assert r and not H.is_error(r) and ops.rfx_last_rows_on_gpu() == 1, H.error_text(r)
        assert H.header(r).type == H.header(x).type and np.array_equal(D.cells_of(r), want[mask != 0])
        ops.rfx_host_drop(r)


_SHARDED_DOOR = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import rows_door as D
import rows_ref as R
from rayforce_amd import hostobj as H
ops = H.lib()
assert ops.rfx_host_bind() == 0
ran = 0
for c in R.load_cases():
    if c["host"] is None and c["verb"] == "filter" and len(c["mask"]) in (513, 1025, 4097, 20011):
        D.check_door(ops, c)
        ran += 1
assert ops.rfx_ops_shards() == SHARDS and ran > 20, (ops.rfx_ops_shards(), ran)
for c in R.load_cases():
    if c["name"] in ("take_len4097_m1_pos_t5", "reverse_i64_len4097"):
        r, _ = D.call(ops, c)
        assert H.is_error(r) and ops.rfx_last_rows_on_gpu() == 0 and c["verb"] + " over a sharded table" in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error()
        ran += 100
assert ran > 200
print("ROWS-DOOR-OK", ran)
'''


@pytest.mark.parametrize("shards", [2, 3])
def test_filter_over_shards_through_the_door(built, shards):
    """RFX_SHARDS=k in a process of its own (the operator layer's shards are fixed at its first call)"""
    env = dict(os.environ, RFX_SHARDS=str(shards), HSA_ENABLE_IPC_MODE_LEGACY="0")
    code = f"ROOT = {ROOT!r}\nSHARDS = {shards}\n" + _SHARDED_DOOR
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ROWS-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
