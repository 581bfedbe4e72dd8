"""The set verbs on the device -- distinct / in / find / sect / except / union (rfx_set.hip, rfx_exec_set.c, rfx_ops_set.c): every case of the
fixture the compiled reference wrote (tests/golden/set_golden.npz) through the planner (Engine), through the C operators over host vectors and
over device-column handles -- bit for bit, order, type code and attributes included, on the reference's own route; the shapes the reference
cannot answer are refused with their reason; larger random columns against the restatement (tests/set_ref.py) and torch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import set_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError
from rayforce_amd.sets import RfxUndefined
from test_set_cpu import DEFINED, HOST

pytestmark = pytest.mark.gpu
ROUTE_CODE = {"none": 0, "dense": 1, "hash": 2, "disjoint": 3, "atom": 4}
COUNTER = {"distinct": L.RFX_XSTAT_SET_DISTINCTS, "union": L.RFX_XSTAT_SET_DISTINCTS, "in": L.RFX_XSTAT_SET_MEMBERS, "find": L.RFX_XSTAT_SET_MEMBERS,
           "sect": L.RFX_XSTAT_SET_FILTERS, "except": L.RFX_XSTAT_SET_FILTERS}


def col(eng, a):
    return eng.column(np.ascontiguousarray(a, dtype=np.int64))


def engine_verb(eng, c):
    x = col(eng, c["x"])
    if c["verb"] == "distinct":
        return eng.distinct(x)
    y = int(c["y"][0]) if c["atom"] else col(eng, c["y"])
    return {"in": eng.isin, "find": eng.find, "sect": eng.sect, "except": eng.except_, "union": eng.union}[c["verb"]](x, y)


# ---------------------------------------------------------------------------------------------------- the fixture through Engine
@pytest.mark.parametrize("c", DEFINED, ids=lambda c: c["name"])
def test_fixture_through_engine(eng, c):
    before = eng.xstat(COUNTER[c["verb"]])
    got = engine_verb(eng, c)
    assert eng.last_set_route == c["route"], (c["name"], eng.last_set_route)
    assert got.dtype == (torch.int8 if c["verb"] == "in" else torch.int64)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), c["out"]), c["name"]
    # a call that had nothing to look up launches nothing and is not counted
    launched = c["route"] != "none"
    assert eng.xstat(COUNTER[c["verb"]]) - before == int(launched), c["name"]


@pytest.mark.parametrize("c", HOST, ids=lambda c: c["name"])
def test_undefined_shapes_are_declined_by_the_planner(eng, c):
    with pytest.raises(RfxUndefined, match="undefined in the reference"):
        engine_verb(eng, c)
    assert eng.last_set_route == "undefined"


# ---------------------------------------------------------------------------------------------------- the door
@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    o.rfx_host_bind()
    return o


def host_vector(ops, cells, t):
    o = ops.rfx_host_vector(t, cells.size)
    data = np.ascontiguousarray(cells, dtype=np.int64)
    if cells.size:
        C.memmove(H.payload(o), data.ctypes.data, data.nbytes)
    return o


def device_handle(cells, t, keep):
    """a device-column handle over a torch tensor (kept alive by `keep`); an empty column is an empty slice of a real allocation"""
    d = torch.from_numpy(np.ascontiguousarray(cells, dtype=np.int64)).to("cuda:0") if cells.size else torch.zeros(1, dtype=torch.int64, device="cuda:0")[:0]
    keep.append(d)
    o = H.device_vector(d)
    H.header(o).type = t
    return o


def cells_of(o):
    h = H.header(o)
    if h.type == 1:
        return np.frombuffer((C.c_char * h.len).from_address(H.payload(o)), dtype=np.int8).astype(np.int64)
    return np.frombuffer((C.c_char * (h.len * 8)).from_address(H.payload(o)), dtype=np.int64).copy()


def door_verb(ops, c, make):
    x = make(c["x"], c["type"])
    if c["verb"] == "distinct":
        return ops.rfx_distinct(x), [x]
    if c["atom"]:
        y = ops.rfx_host_i64(int(c["y"][0]))
        H.header(y).type = -c["type"]
    else:
        y = make(c["y"], c["type"])
    return getattr(ops, "rfx_" + c["verb"])(x, y), [x, y]


@pytest.mark.parametrize("how", ["host_vectors", "device_handles"])
@pytest.mark.parametrize("c", DEFINED, ids=lambda c: c["name"])
def test_fixture_through_the_operators(ops, c, how):
    keep = []
    make = (lambda a, t: host_vector(ops, a, t)) if how == "host_vectors" else (lambda a, t: device_handle(a, t, keep))
    r, args = door_verb(ops, c, make)
    try:
        assert not H.is_error(r), (c["name"], H.error_text(r))
        h = H.header(r)
        assert ops.rfx_last_set_on_gpu() == 1, (c["name"], ops.rfx_ops_last_error())
        assert ops.rfx_last_set_route() == ROUTE_CODE[c["route"]], c["name"]
        assert h.type == c["rtype"], c["name"]
        # (a SYMBOL answer's attributes cannot be read out of the reference binary: -1 in the fixture; index_distinct_i64 sets ATTR_DISTINCT whatever the type)
        assert h.attrs == (c["attrs"] if c["attrs"] >= 0 else int(c["verb"] in ("distinct", "union"))), c["name"]
        assert np.array_equal(cells_of(r), c["out"]), c["name"]
    finally:
        for o in args + [r]:
            ops.rfx_host_drop(o)


@pytest.mark.parametrize("c", HOST, ids=lambda c: c["name"])
def test_undefined_shapes_are_refused_by_the_operators(ops, c):
    r, args = door_verb(ops, c, lambda a, t: host_vector(ops, a, t))
    assert H.is_error(r), c["name"]  # (no host beside the library here: never answered)
    text = H.error_text(r)
    assert "not covered by the MI355X path" in text and "undefined in the reference" in text and "no host function" in text, text
    assert ops.rfx_last_set_on_gpu() == 0
    for o in args + [r]:
        ops.rfx_host_drop(o)


def test_set_stats_tell_who_answered(ops):
    """rfx_set_stats, the verb a host loads beside the six: answered by the device / handed over (here: refused, no host) / the answered ones by route"""
    def stats():
        r = ops.rfx_set_stats(None)
        st = H.to_numpy(r).copy()
        ops.rfx_host_drop(r)
        return st

    s0 = stats()
    assert s0.shape == (7,)
    x, y, neg = host_vector(ops, np.arange(100) % 9, 5), host_vector(ops, np.array([0, 10**12, 5]), 5), host_vector(ops, np.array([-7, 10**12, 5]), 5)
    empty, far, atom = host_vector(ops, np.empty(0, np.int64), 5), host_vector(ops, np.array([500, 501]), 5), ops.rfx_host_i64(3)
    calls = [("distinct", (x,), 1), ("in", (y, y), 2), ("find", (x, far), 3), ("except", (x, atom), 4), ("distinct", (empty,), 0), ("sect", (neg, y), None), ("union", (x, atom), None)]
    for verb, args, route in calls:
        before = stats()
        r = getattr(ops, "rfx_" + verb)(*args)
        d = stats() - before
        want = np.zeros(7, np.int64)
        if route is None:
            assert H.is_error(r)
            want[1] = 1
        else:
            assert not H.is_error(r), H.error_text(r)
            want[0] = want[2 + route] = 1
        assert np.array_equal(d, want), (verb, d)
        ops.rfx_host_drop(r)
    for o in (x, y, neg, empty, far, atom):
        ops.rfx_host_drop(o)


def test_in_over_a_column_that_is_not_16_byte_aligned(eng):
    """the B8 probe's 16-byte loads need x aligned; a slice from an odd cell on takes the 8-byte-load kernel: same bytes, full steps and tail"""
    rng = np.random.default_rng(8)
    for kind, n in (("dense", 5 * 512 + 77), ("hash", 70_001)):
        x, y = big(rng, kind, n + 1), big(rng, kind, n // 3)
        dx = col(eng, x)[1:]
        assert dx.data_ptr() % 16 == 8
        m = eng.isin(dx, col(eng, y))
        assert eng.last_set_route == kind and np.array_equal(m.cpu().numpy().astype(bool), np.isin(x[1:], y))


def test_shapes_outside_the_device_path_are_handed_back(ops):
    i64 = host_vector(ops, np.arange(10), 5)
    ts = host_vector(ops, np.arange(10), 9)
    f64 = ops.rfx_host_vector(10, 4)
    i32 = ops.rfx_host_vector(4, 4)
    atom = ops.rfx_host_i64(3)
    tab = H.table({"a": np.arange(4)})
    lst = ops.rfx_host_list(0)
    shapes = [("distinct", (f64,)), ("distinct", (i32,)), ("distinct", (atom,)), ("distinct", (tab,)), ("distinct", (lst,)),
              ("in", (i64, ts)), ("in", (atom, i64)), ("in", (i64, atom)), ("in", (i32, i32)), ("find", (i64, atom)), ("find", (f64, f64)),
              ("union", (i64, ts)), ("union", (i64, atom)), ("sect", (ts, ts)), ("sect", (i64, atom)), ("except", (ts, ts)), ("except", (i64, f64)),
              ("except", (tab, atom))]
    for verb, args in shapes:
        r = getattr(ops, "rfx_" + verb)(*args)
        assert H.is_error(r), (verb, args)
        assert f"{verb}: not covered by the MI355X path" in H.error_text(r) and "no host function" in H.error_text(r), H.error_text(r)
        assert ops.rfx_last_set_on_gpu() == 0
        ops.rfx_host_drop(r)


_SHARDED_DOOR = r"""
import sys
sys.path.insert(0, ROOT)
import numpy as np
from rayforce_amd import hostobj as H
ops = H.lib()
ops.rfx_host_bind()
x = H.vector(np.arange(5000) % 7)
for verb, args in (("distinct", (x,)), ("in", (x, x)), ("find", (x, x)), ("sect", (x, x)), ("except", (x, x)), ("union", (x, x))):
    r = getattr(ops, "rfx_" + verb)(*args)
    assert H.is_error(r), verb
    assert "over a sharded column" in H.error_text(r), H.error_text(r)
    assert ops.rfx_last_set_on_gpu() == 0
assert ops.rfx_ops_shards() == 2
print("sharded door ok")
"""


def test_the_door_hands_sharded_columns_back(built):
    """RFX_SHARDS=2 in a process of its own (the operator layer's shards are fixed at its first call)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RFX_SHARDS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {root!r}\n" + _SHARDED_DOOR], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "sharded door ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_a_sharded_planner_refuses_with_its_reason():
    e = Engine(0, shards=2)
    try:
        c = torch.arange(1000, device="cuda:0")
        for what, call in (("distinct", lambda: e.distinct(c)), ("union", lambda: e.union(c, c)), ("in", lambda: e.isin(c, c)), ("find", lambda: e.find(c, c)),
                           ("sect", lambda: e.sect(c, c)), ("except", lambda: e.except_(c, c))):
            with pytest.raises(RfxError, match=f"{what} over a sharded column"):
                call()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- larger columns
def big(rng, kind, n):
    if kind == "dense":
        return rng.integers(-5000, 600_000, n)
    a = rng.integers(0, 10**12, max(2, n // 8))[rng.integers(0, max(2, n // 8), n)]  # ~n/8 keys over 1e12: the hash route, duplicates
    a[0], a[1] = 0, 10**12
    return a


@pytest.mark.parametrize("kind,n", [("dense", 1_000_003), ("hash", 1_000_003), ("dense", 6_000_011), ("hash", 2_500_009)])
def test_large_columns_equal_the_restatement_and_torch(eng, kind, n):
    rng = np.random.default_rng(n)
    x, y = big(rng, kind, n), big(rng, kind, n // 3 + 1)
    if kind == "hash":
        y[2 : y.size // 2] = x[rng.integers(0, n, y.size // 2 - 2)]  # (a real intersection)
    dx, dy = col(eng, x), col(eng, y)
    d = eng.distinct(dx)
    assert eng.last_set_route == kind
    want, route = R.distinct(x)
    assert route == kind and np.array_equal(d.cpu().numpy(), want)
    assert torch.equal(torch.sort(d).values, torch.unique(dx))
    u = eng.union(dx, dy)
    assert eng.last_set_route == kind and torch.equal(torch.sort(u).values, torch.unique(torch.cat([dx, dy])))
    if n < 2_000_000:
        assert np.array_equal(u.cpu().numpy(), R.union(x, y)[0])
    m = eng.isin(dx, dy)
    assert eng.last_set_route == kind and torch.equal(m.bool(), torch.isin(dx, dy))
    f = eng.find(dx, dy)
    assert eng.last_set_route == kind and np.array_equal(f.cpu().numpy(), R.find(x, y)[0])
    s, e = eng.sect(dx, dy), eng.except_(dx, dy)
    assert torch.equal(s, dx[m.bool()]) and torch.equal(e, dx[~m.bool()])
    assert torch.equal(eng.except_(dx, int(x[5])), dx[dx != int(x[5])]) and eng.last_set_route == "atom"


def test_timing_counters(eng):
    ns = [eng.xstat(s) for s in (L.RFX_XSTAT_NS_SET_BUILD, L.RFX_XSTAT_NS_SET_PROBE)]
    c = col(eng, np.arange(50_000) % 977)
    eng.distinct(c)
    eng.isin(c, c)
    assert eng.xstat(L.RFX_XSTAT_NS_SET_BUILD) > ns[0] and eng.xstat(L.RFX_XSTAT_NS_SET_PROBE) > ns[1]


# ---------------------------------------------------------------------------------------------------- `in` under where: stays what it was
def test_in_under_where_keeps_its_path(ops):
    """(in column [v1 .. vn]) inside a select's where: is still taken apart into at most RFX_MAX_PREDS comparisons of the ONE fused pass -- no
    mask pass, no set verb -- and a longer list is still not the device's (without a host: an error object), although `in` is a verb now."""
    rng = np.random.default_rng(5)
    a, v = rng.integers(0, 50, 100_000), rng.integers(0, 1000, 100_000)
    tab = H.table({"a": a, "v": v})
    xl = L.load_library()

    def counters():
        st = H.to_numpy(ops.rfx_stats(0))
        x = ops.rfx_ops_exec()
        return [int(st[0]), int(st[1]), int(st[10])] + [int(xl.rfx_exec_stat(x, s)) if x else 0 for s in (L.RFX_XSTAT_SET_MEMBERS, L.RFX_XSTAT_SET_FILTERS)]

    def select(values):
        where = H.list_of([ops.rfx_host_fn(b"in"), H.atom("a"), H.vector(np.array(values, np.int64))])
        q = ops.rfx_host_dict(H.symbols(["s", "where", "from"]), H.list_of([H.expr(("sum", "v")), where, ops.rfx_host_clone(tab)]))
        return ops.rfx_select(q)

    ops.rfx_select(H.select_dict({"s": ("sum", "v")}, tab))  # (the planner exists from here on)
    before = counters()
    r = select([3, 5, 7])
    assert not H.is_error(r), H.error_text(r)
    assert int(H.table_to_numpy(r)["s"][0]) == int(v[np.isin(a, [3, 5, 7])].sum())
    after = counters()
    assert [x - y for x, y in zip(after, before)] == [1, 0, 0, 0, 0]  # on the GPU, not delegated, no mask pass, no set verb
    r = select(list(range(9)))  # one more than RFX_MAX_PREDS
    assert H.is_error(r) and ops.rfx_last_select_on_gpu() == 0
    assert counters()[3:] == after[3:]
