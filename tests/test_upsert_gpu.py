"""upsert and insert on the GPU by equality of bits: every case of the reference's fixture (tests/golden/upsert_golden.npz) through the C door over
standalone host objects (cells, type code, attribute byte) and through the Engine; the shapes handed back with their reasons; the planner's counters; a
sharded Engine and a sharded door refuse with their reason; the same call twice gives the same bytes; and what the feature is for -- the answer of
(upsert t 1 batch) is resident: a select over it uploads nothing."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import upsert_door as D
import upsert_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = R.load_cases()
CASES = [c for c in ALL if not c.get("host")]
HOSTS = [c for c in ALL if c.get("host")]
GROUPS = ("grid_n0", "grid_n1_", "grid_n64", "grid_n4097", f"grid_n{R.BIG}", "pattern", "keys", "nine", "short", "dict", "table", "record", "insert", "other")
ST_UPLOADS = 4


def group_of(c):
    return next((g for g in GROUPS[:-1] if c["name"].startswith(g)), "other")


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0  # standalone host: nothing behind the door to hand a shape to
    return o


def test_every_case_has_a_group():
    assert {group_of(c) for c in CASES} == set(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_fixture_through_the_door(ops, group):
    ran = 0
    for c in CASES:
        if group_of(c) == group:
            D.check_door(ops, c)
            ran += 1
            if c["n"] <= 5000 and group in ("pattern", "keys", "short", "record", "insert"):
                D.check_door(ops, R.retyped(c, R.I64, R.SYMBOL))  # SYMBOL cells are looked up and copied as I64 cells are: the same answer under the other code
    assert ran >= 1
    ops.rfx_cache_clear()


@pytest.mark.parametrize("group", GROUPS)
def test_fixture_through_the_engine_and_the_counters(eng, group):
    stats = (L.RFX_XSTAT_UPSERTS, L.RFX_XSTAT_UPSERT_MATCHED, L.RFX_XSTAT_UPSERT_APPENDED, L.RFX_XSTAT_INSERTS)
    before = [eng.xstat(s) for s in stats]
    want = [0, 0, 0, 0]
    for c in CASES:
        if group_of(c) == group:
            D.check_engine(eng, c)
            counts = {}
            R.answer(c, counts)
            if c["verb"] == "insert":
                want[3] += 1
            else:
                want = [want[0] + 1, want[1] + counts["matched"], want[2] + counts["appended"], want[3]]
    assert [a - b for a, b in zip([eng.xstat(s) for s in stats], before)] == want


def test_the_phase_timers_advance(eng):
    stats = (L.RFX_XSTAT_NS_UPSERT_INDEX, L.RFX_XSTAT_NS_UPSERT_PLAN, L.RFX_XSTAT_NS_UPSERT_PLACE)
    before = [eng.xstat(s) for s in stats]
    D.check_engine(eng, next(c for c in CASES if c["name"] == "pattern_dups"))
    assert all(eng.xstat(s) > b for s, b in zip(stats, before))


def test_shapes_outside_the_device_path_are_handed_back(ops):
    assert len(HOSTS) == len(R.HOST_SHAPES)
    for c in HOSTS:
        D.check_refused(ops, c)


def test_the_same_call_twice_gives_the_same_bytes(ops):
    for name in ("pattern_dups", "keys3", "sparse_keys_dups"):
        c = next(c for c in CASES if c["name"] == name)
        one, two = D.check_door(ops, c), D.check_door(ops, c)
        assert all(a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes() for a, b in zip(one, two)), name
    ops.rfx_cache_clear()


def test_device_handles_as_operands(ops):
    """the table's columns as device handles from their tensors' second cell (cell-aligned only), the batch's as handles at their tensors' start"""
    n, m = 5001, 301
    k = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 3
    v = torch.arange(n + 1, dtype=torch.float64, device="cuda") * 0.5
    bk = torch.arange(m, dtype=torch.int64, device="cuda") * 9 + 3 * n - 900  # the first hundred match rows of the table
    bv = -torch.arange(m, dtype=torch.float64, device="cuda")
    handle = lambda t, tp, skip: ops.rfx_host_device_vector(tp, t.numel() - skip, (C.c_void_p * 1)(t.data_ptr() + skip * t.element_size()), 1)  # noqa: E731
    tab = ops.rfx_host_table(H.symbols(["k", "v"]), H.list_of([handle(k, R.I64, 1), handle(v, R.F64, 1)]))
    batch = H.list_of([handle(bk, R.I64, 0), handle(bv, R.F64, 0)])
    one = ops.rfx_host_i64(1)
    r = D.vary(ops, "upsert", [tab, one, batch])
    assert not H.is_error(r) and ops.rfx_last_upsert_on_gpu() == 1, ops.rfx_ops_last_error().decode()
    hk, hv, hbk, hbv = k[1:].cpu().numpy(), v[1:].cpu().numpy(), bk.cpu().numpy(), bv.cpu().numpy()
    row = {int(x): i for i, x in enumerate(hk)}
    new = [j for j in range(m) if int(hbk[j]) not in row]
    for j in range(m):
        if int(hbk[j]) in row:
            hv[row[int(hbk[j])]] = hbv[j]
    assert 0 < len(new) < m
    got = [D.cells_of(o) for o in H.list_items(H.list_items(r)[1])]
    assert np.array_equal(got[0], np.concatenate([hk, hbk[new]])) and np.array_equal(got[1], np.concatenate([hv, hbv[new]]))
    for o in (r, tab, one, batch):
        ops.rfx_host_drop(o)


def test_engine_refuses_what_the_reference_does_not_answer_with_vectors(eng):
    k = torch.arange(5, device=eng.device) * 3 + 7
    v = torch.arange(5, device=eng.device).double()
    w = torch.arange(5, device=eng.device).to(torch.int32)
    for bad in (lambda: eng.upsert({"k": k, "v": v}, 1, {"z": k}), lambda: eng.upsert({"k": k, "v": v}, 3, [k, v]), lambda: eng.upsert({"k": k, "v": v}, 1, [k, w]),
                lambda: eng.upsert({"k": k, "w": w}, 1, [k, w]), lambda: eng.upsert({"k": k, "w": w}, 1, [k + 100]), lambda: eng.upsert({"k": v, "v": v}, 1, [v, v]),
                lambda: eng.insert({"k": k, "v": v}, [k]), lambda: eng.upsert({"k": k, "v": v}, 1, [k[:0], v[:0]]), lambda: eng.upsert({"k": k, "v": v}, 1, [k, v[:3]])):
        with pytest.raises(RfxError):
            bad()


def test_a_sharded_engine_refuses(built):
    e = Engine(0, shards=2)
    try:
        k = torch.arange(100, device=e.device)
        with pytest.raises(RfxError, match="upsert over a sharded table"):
            e.upsert({"k": k, "v": k.double()}, 1, [k, k.double()])
        with pytest.raises(RfxError, match="insert over a sharded table"):
            e.insert({"k": k, "v": k.double()}, [k, k.double()])
    finally:
        e.close()


_CHILD = """
import os, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np
import upsert_door as D, upsert_ref as R
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
c = dict(name="x", verb="upsert", keys=1, form="list", types=[R.I64, R.F64], n=100, m=10, pattern="alt", given=[0, 1])
for verb in ("upsert", "insert"):
    r, _ = D.call(ops, dict(c, verb=verb, keys=1 if verb == "upsert" else 0))
    assert H.is_error(r) and ops.rfx_last_upsert_on_gpu() == 0 and ops.rfx_ops_shards() == 2
    print(ops.rfx_ops_last_error().decode())
""", RFX_SHARDS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    assert "upsert over a sharded table" in out and "insert over a sharded table" in out


# ---- the residency of the answer ----
ROWS, BATCH = 200_003, 1_003
_RESIDENCY = """
rng = np.random.default_rng(7)
ht = dict(k=np.arange({rows}, dtype=np.int64) * 3, g=rng.integers(0, 1000, {rows}), v=rng.integers(-1000, 1000, {rows}).astype(np.float64), w=rng.integers(0, 1 << 40, {rows}))
hb = dict(k=rng.integers(0, 6 * {rows}, {batch}), g=rng.integers(0, 1000, {batch}), v=rng.integers(-1000, 1000, {batch}).astype(np.float64), w=rng.integers(0, 1 << 40, {batch}))
ops.rfx_cache_clear()
t, b, one = H.table(ht), H.table(hb), ops.rfx_host_i64(1)
import ctypes as C
r = ops.rfx_upsert((C.c_void_p * 3)(t, one, b), 3)
assert not H.is_error(r) and ops.rfx_last_upsert_on_gpu() == 1
d = H.select_dict(dict(s=("sum", "v"), u=("sum", "w"), by="g"), r)
s0 = H.to_numpy(ops.rfx_stats(0))
a = ops.rfx_select(d)
s1 = H.to_numpy(ops.rfx_stats(0))
assert not H.is_error(a) and ops.rfx_last_select_on_gpu() == 1
got = H.table_to_numpy(a)
print("UPLOADS", int(s1[{up}] - s0[{up}]))
hr = dict((n, v.copy()) for n, v in ht.items())
row = dict((int(k), i) for i, k in enumerate(ht["k"]))
extra = dict((n, []) for n in ht)
for j in range({batch}):
    i = row.get(int(hb["k"][j]))
    for n in ht:
        if i is None:
            extra[n].append(hb[n][j])
        elif n != "k":
            hr[n][i] = hb[n][j]
hr = dict((n, np.concatenate([hr[n], np.array(extra[n], dtype=hr[n].dtype)])) for n in ht)
assert all(np.array_equal(v, hr[n]) for n, v in H.table_to_numpy(r).items())
keys = np.array(sorted(set(hr["g"].tolist())))
order = np.argsort(got["g"])
assert np.array_equal(got["g"][order], keys)
assert np.array_equal(got["s"][order], np.array([hr["v"][hr["g"] == k].sum() for k in keys]))   # (integer-valued f64 cells: exact in any order)
assert np.array_equal(got["u"][order], np.array([hr["w"][hr["g"] == k].sum() for k in keys]))
print("ANSWER ok")
"""


def test_the_answer_is_resident_and_without_adoption_it_is_uploaded(built):
    """(upsert t 1 batch), then a grouped select over the answer: not one upload; with RFX_CONCAT_ADOPT=0 the select uploads the three columns it names"""
    body = _RESIDENCY.format(rows=ROWS, batch=BATCH, up=ST_UPLOADS)
    with_adoption, without = _child(body), _child(body, RFX_CONCAT_ADOPT="0")
    assert "UPLOADS 0" in with_adoption and "ANSWER ok" in with_adoption
    assert "UPLOADS 3" in without and "ANSWER ok" in without
