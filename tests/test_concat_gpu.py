"""concat and raze on the GPU by equality of bits: every case of the reference's fixture (tests/golden/concat_golden.npz) through the C door over
standalone host objects (cells, type code, attributes) and through the Engine; the shapes handed back with their reasons; tensor views and device
handles as operands; the planner's counters; a sharded Engine and a sharded door refuse with their reason; and what the feature is for -- the answer of
(concat t batch) is resident: a select over it uploads nothing."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import concat_door as D
import concat_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [c for c in R.load_cases() if not c.get("host")]
HOSTS = [c for c in R.load_cases() if c.get("host")]
ST_UPLOADS = 4


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0  # standalone host: nothing behind the door to hand a shape to
    return o


@pytest.mark.parametrize("verb", ["concat", "table", "raze"])
def test_fixture_through_the_door(ops, verb):
    ran = 0
    for c in CASES:
        if c["verb"] == verb:
            D.check_door(ops, c)
            ran += 1
            if any(tp == R.I64 for tp, _p in c["cols"]) and sum(len(cells) for _t, _a, cells in c["out"]) <= 5000:
                D.check_door(ops, R.retyped(c, R.I64, R.SYMBOL))  # SYMBOL cells are copied as I64 cells are: the same answer under the other type code
    assert ran >= {"concat": 250, "table": 6, "raze": 24}[verb]
    ops.rfx_cache_clear()


def test_u8_atoms_through_the_door(ops):
    """(the recorder cannot make a U8 atom inside the reference: (first v) of a U8 vector is not one -- held to the restatement)"""
    v = np.arange(37, dtype=np.uint8)
    for parts in ([v, {"atom": 200}], [{"atom": 255}, v], [v[:0], {"atom": 7}]):
        c = dict(name="u8_atom", verb="concat", cols=[(R.U8, parts)])
        D.check_door(ops, dict(c, out=R.answer(c)))


@pytest.mark.parametrize("verb", ["concat", "table", "raze"])
def test_fixture_through_the_engine_and_the_counters(eng, verb):
    before = [eng.xstat(s) for s in (L.RFX_XSTAT_CONCATS, L.RFX_XSTAT_CONCAT_SPANS, L.RFX_XSTAT_CONCAT_CELLS)]
    calls = spans = cells = 0
    for c in CASES:
        if c["verb"] == verb:
            D.check_engine(eng, c)
            n = sum(len(o[2]) for o in c["out"])
            if n:  # (an empty answer launches nothing and is not counted)
                calls += 1
                spans += sum(len(parts) for _tp, parts in c["cols"])
                cells += n
    after = [eng.xstat(s) for s in (L.RFX_XSTAT_CONCATS, L.RFX_XSTAT_CONCAT_SPANS, L.RFX_XSTAT_CONCAT_CELLS)]
    assert [a - b for a, b in zip(after, before)] == [calls, spans, cells]


def test_shapes_outside_the_device_path_are_handed_back(ops):
    assert len(HOSTS) == len(R.HOST_SHAPES)
    for c in HOSTS:
        D.check_refused(ops, c)


@pytest.mark.parametrize("dtype", [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float64])
def test_tensor_views_as_operands(eng, dtype):
    """t[1:], t[3:]: source addresses that are cell-aligned and nothing more, on both sides and inside a raze"""
    n = 20011
    t = (torch.arange(n, device=eng.device) * 7 - 300).to(dtype)
    u = (torch.arange(n, device=eng.device) * 3 + 11).to(dtype)
    for a, b in ((t[1:], u[3:]), (t[3:], u[1:]), (t[1:18], u[3:]), (t[3:], u[5:6]), (t[2:], u)):
        assert torch.equal(eng.concat(a, b), torch.cat([a, b]))
    parts = [t[1:], u[3:40], t[:0], u[7:], t[5:6], t[n - 3:]]
    assert torch.equal(eng.raze(parts), torch.cat(parts))
    got = eng.concat({"a": t[1:], "b": u[3:]}, {"b": u[5:9], "a": t[3:7]})
    assert list(got) == ["a", "b"] and torch.equal(got["a"], torch.cat([t[1:], t[3:7]])) and torch.equal(got["b"], torch.cat([u[3:], u[5:9]]))


def test_engine_refuses_what_the_reference_does_not_concatenate(eng):
    t = torch.arange(5, device=eng.device)
    for bad in (lambda: eng.concat(1, 2), lambda: eng.concat(t, t.double()), lambda: eng.concat({"a": t}, {"b": t}), lambda: eng.raze([]),
                lambda: eng.concat({"a": t}, t)):
        with pytest.raises(RfxError):
            bad()


def test_device_handles_as_operands(ops):
    x = torch.arange(1000, dtype=torch.int64, device="cuda") * 5
    y = torch.arange(77, dtype=torch.float64, device="cuda")
    m = (torch.arange(333, device="cuda") % 3 == 0).to(torch.int8)
    for t, tp in ((x, R.I64), (y, R.F64), (m, R.B8), (x, R.TS)):
        h = ops.rfx_host_device_vector(tp, t.numel() - 1, (C.c_void_p * 1)(t.data_ptr() + t.element_size()), 1)  # (from the second cell: cell-aligned only)
        v = D.host_vector(ops, t[:5].cpu().numpy(), tp)
        r = ops.rfx_concat(v, h)
        assert not H.is_error(r) and ops.rfx_last_concat_on_gpu() == 1 and H.header(r).type == tp and H.header(r).attrs == 0
        assert np.array_equal(D.cells_of(r), torch.cat([t[:5], t[1:]]).cpu().numpy())
        for o in (r, v, h):
            ops.rfx_host_drop(o)


def test_a_sharded_engine_refuses(built):
    e = Engine(0, shards=2)
    try:
        t = torch.arange(100, device=e.device)
        with pytest.raises(RfxError, match="concat over a sharded column"):
            e.concat(t, t)
        with pytest.raises(RfxError, match="concat over a sharded column"):
            e.raze([t, t])
    finally:
        e.close()


_CHILD = """
import os, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np
import concat_door as D, concat_ref as R
from rayforce_amd import hostobj as H
ops = H.lib(); ops.rfx_host_bind()
{body}
"""


def _child(body, **env):
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT, body=body)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_a_sharded_door_hands_back(built):
    """RFX_SHARDS=2 in a process of its own (the operator layer's shards are fixed at its first call)"""
    out = _child("""
x = D.host_vector(ops, np.arange(100, dtype=np.int64), R.I64)
r = ops.rfx_concat(x, x)
assert H.is_error(r) and ops.rfx_last_concat_on_gpu() == 0 and ops.rfx_ops_shards() == 2
print(ops.rfx_ops_last_error().decode())
""", RFX_SHARDS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    assert "concat over a sharded column" in out


# ---- the residency of the answer ----
ROWS, BATCH = 200_003, 1_003
_RESIDENCY = """
rng = np.random.default_rng(7)
def tab(n):
    return dict(k=rng.integers(0, 1000, n), v=rng.integers(-1000, 1000, n).astype(np.float64), w=rng.integers(0, 1 << 40, n))
ht, hb = tab({rows}), tab({batch})
ops.rfx_cache_clear()
bytes0 = ops.rfx_cache_bytes()
t, b = H.table(ht), H.table(hb)
r = ops.rfx_concat(t, b)
assert not H.is_error(r) and ops.rfx_last_concat_on_gpu() == 1
d = H.select_dict(dict(s=("sum", "v"), u=("sum", "w"), by="k"), r)
s0 = H.to_numpy(ops.rfx_stats(0))
a = ops.rfx_select(d)
s1 = H.to_numpy(ops.rfx_stats(0))
assert not H.is_error(a) and ops.rfx_last_select_on_gpu() == 1
got = H.table_to_numpy(a)
print("UPLOADS", int(s1[{up}] - s0[{up}]))
hr = dict((n, np.concatenate([ht[n], hb[n]])) for n in ht)
keys = np.array(sorted(set(hr["k"].tolist())))
order = np.argsort(got["k"])
assert np.array_equal(got["k"][order], keys)
assert np.array_equal(got["s"][order], np.array([hr["v"][hr["k"] == k].sum() for k in keys]))   # (integer-valued f64 cells: exact in any order)
assert np.array_equal(got["u"][order], np.array([hr["w"][hr["k"] == k].sum() for k in keys]))
print("ANSWER ok")
"""


def test_the_answer_is_resident(ops):
    """(concat t batch), then a grouped select over the answer: not one upload; an update of the answer by the host's own rule (copy unless the only
    owner) is seen; dropping the answer gives every byte back"""
    rng = np.random.default_rng(7)

    def tab(n):
        return dict(k=rng.integers(0, 1000, n), v=rng.integers(-1000, 1000, n).astype(np.float64), w=rng.integers(0, 1 << 40, n))

    ht, hb = tab(ROWS), tab(BATCH)
    ops.rfx_cache_clear()
    bytes0 = ops.rfx_cache_bytes()
    t, b = H.table(ht), H.table(hb)
    r = ops.rfx_concat(t, b)
    assert not H.is_error(r) and ops.rfx_last_concat_on_gpu() == 1
    assert ops.rfx_cache_bytes() - bytes0 == 3 * 8 * (ROWS + BATCH + ROWS + BATCH)  # the operands' copies and the answer's
    hr = {n: np.concatenate([ht[n], hb[n]]) for n in ht}
    assert all(np.array_equal(v, hr[n]) for n, v in H.table_to_numpy(r).items())
    cols = H.list_items(H.list_items(r)[1])
    assert [H.header(c).rc for c in cols] == [2, 2, 2]  # the cache's reference to every column of the answer
    d = H.select_dict(dict(s=("sum", "v"), u=("sum", "w"), by="k"), r)

    def select():
        s0 = H.to_numpy(ops.rfx_stats(0))
        a = ops.rfx_select(d)
        s1 = H.to_numpy(ops.rfx_stats(0))
        assert not H.is_error(a) and ops.rfx_last_select_on_gpu() == 1, H.error_text(a)
        got = H.table_to_numpy(a)
        ops.rfx_host_drop(a)
        keys = np.array(sorted(set(hr["k"].tolist())))
        order = np.argsort(got["k"])
        assert np.array_equal(got["k"][order], keys)
        assert np.array_equal(got["s"][order], np.array([hr["v"][hr["k"] == k].sum() for k in keys]))  # (integer-valued f64 cells: exact in any order)
        assert np.array_equal(got["u"][order], np.array([hr["w"][hr["k"] == k].sum() for k in keys]))
        return int(s1[ST_UPLOADS] - s0[ST_UPLOADS]), int(s1[13] - s0[13])

    uploads, own_hits = select()
    print("uploads of the select after the append:", uploads, "-- uses proven current by ownership:", own_hits)
    assert uploads == 0 and own_hits >= 3
    # the host updates the answer's column v by its own rule: the cache's reference makes it copy, the copy is a new vector -> one upload, the new cells
    collist = H.list_items(r)[1]
    slots = (C.c_void_p * 3).from_address(H.payload(collist))
    vi = list(ht).index("v")
    assert H.header(slots[vi]).rc == 2
    hr["v"] = hr["v"].copy()
    hr["v"][[0, ROWS - 1, ROWS, ROWS + BATCH - 1]] += 12345.0
    old = slots[vi]
    slots[vi] = H.vector(hr["v"])
    ops.rfx_host_drop(old)
    uploads, _ = select()
    assert uploads == 1
    for o in (d, r, t, b):
        ops.rfx_host_drop(o)
    ops.rfx_cache_clear()
    assert ops.rfx_cache_bytes() == bytes0


def test_without_adoption_the_select_uploads_the_answers_columns(built):
    body = _RESIDENCY.format(rows=ROWS, batch=BATCH, up=ST_UPLOADS)
    assert "UPLOADS 0" in _child(body) and "UPLOADS 3" in _child(body, RFX_CONCAT_ADOPT="0")


def test_adoption_under_checksum_validation(ops):
    """(rfx_ops_set_validation(1): the adopted copy is vouched for by the checksum of the payload it was read back into; a raw write is seen)"""
    assert ops.rfx_ops_set_validation(1) == 0
    try:
        x = D.host_vector(ops, np.arange(5000, dtype=np.int64), R.I64)
        r = ops.rfx_concat(x, x)
        s0 = H.to_numpy(ops.rfx_stats(0))
        a = ops.rfx_sum(r)
        s1 = H.to_numpy(ops.rfx_stats(0))
        assert C.c_int64.from_address(a + 8).value == 2 * sum(range(5000)) and s1[ST_UPLOADS] == s0[ST_UPLOADS]
        np.frombuffer((C.c_char * (10000 * 8)).from_address(H.payload(r)), dtype=np.int64)[9999] += 1000
        b = ops.rfx_sum(r)
        s2 = H.to_numpy(ops.rfx_stats(0))
        assert C.c_int64.from_address(b + 8).value == 2 * sum(range(5000)) + 1000 and s2[ST_UPLOADS] - s1[ST_UPLOADS] == 1 and s2[6] - s1[6] == 1
        for o in (a, b, r, x):
            ops.rfx_host_drop(o)
    finally:
        assert ops.rfx_ops_set_validation(0) == 0
