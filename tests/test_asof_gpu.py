"""The asof join, bin and binr on the GPU, all by equality of bits: the flat search kernel and the planner against the numpy restatement
(tests/asof_ref.py) over sizes far beyond the fixture, every case of the reference's fixture (tests/golden/asof_golden.npz) through
rfx_asof_join / rfx_bin / rfx_binr and through Engine, the shapes handed back, the counters."""
import ctypes as C

import numpy as np
import pytest
import torch

import asof_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError
from test_asof_cpu import GOLD, index_case, table_case

pytestmark = pytest.mark.gpu
NULL = -(2**63)


def seg_search(eng, q, t, right, none, group=None, seg=None, rows=None):
    """rfx_hip_seg_search over device copies of numpy arrays -> numpy"""
    dq, dt = eng.column(q), eng.column(t)
    out = torch.empty(len(q), dtype=torch.int64, device=dq.device)
    dg = eng.column(group) if group is not None else None
    ds = eng.column(seg) if seg is not None else None
    dr = eng.column(rows) if rows is not None else None
    L.check(eng.lib.rfx_hip_seg_search(eng._ctx, dq.data_ptr(), len(q), dg.data_ptr() if dg is not None else None, len(seg) // 2 if seg is not None else 0,
                                       ds.data_ptr() if ds is not None else None, len(t), dt.data_ptr(), dr.data_ptr() if dr is not None else None,
                                       int(right), none, out.data_ptr()), "seg_search")
    eng.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("nx", [1, 2, 3, 63, 64, 65, 1000, 1_000_003])
@pytest.mark.parametrize("kind", ["sorted", "unsorted", "ties"])
def test_flat_search_kernel_equals_the_restatement(eng, kind, nx):
    rng = np.random.default_rng(nx * 7 + len(kind))
    x = rng.integers(-50, 50, nx) if kind == "ties" else rng.integers(-(2**62), 2**62, nx)
    if kind != "unsorted":
        x = np.sort(x)
    y = np.concatenate([rng.choice(x, 2000), rng.integers(-(2**62), 2**62, 2000), [NULL, 2**63 - 1, x.min() - 1, x.max() + 1]]).astype(np.int64)
    assert np.array_equal(seg_search(eng, y, x, False, -1), R.bin_(x, y)), (kind, nx, "bin")
    assert np.array_equal(seg_search(eng, y, x, True, nx), R.binr(x, y)), (kind, nx, "binr")
    assert np.array_equal(eng.bin(eng.column(x), eng.column(y)).cpu().numpy(), R.bin_(x, y))
    assert np.array_equal(eng.binr(eng.column(x), eng.column(y)).cpu().numpy(), R.binr(x, y))


def test_segments_runs_and_row_mapping(eng):
    """the two kernels by themselves: runs of a sorted group column addressed by the group's id, then searches inside the runs"""
    rng = np.random.default_rng(11)
    n = 200_000
    lens = np.concatenate([[1, 2, 3, 64, 65, 100_000], rng.integers(1, 40, 4000)])
    lens = lens[np.cumsum(lens) <= n]
    m = m2 = int(lens.sum())
    gs = np.repeat(np.sort(rng.choice(m, len(lens), replace=False)), lens)  # group ids: distinct cells of [0, m), ascending like first rows
    seg = torch.full((2 * m,), -7, dtype=torch.int64, device="cuda:0")
    dgs = eng.column(gs)
    L.check(eng.lib.rfx_hip_asof_runs(eng._ctx, dgs.data_ptr(), m2, seg.data_ptr()), "runs")
    eng.sync()
    seg = seg.cpu().numpy()
    ids, starts, counts = np.unique(gs, return_index=True, return_counts=True)
    assert np.array_equal(seg[2 * ids], starts) and np.array_equal(seg[2 * ids + 1], starts + counts)
    untouched = np.ones(2 * m, bool)
    untouched[2 * ids] = untouched[2 * ids + 1] = False
    assert (seg[untouched] == -7).all()
    t = rng.integers(0, 1000, m2)
    rows = rng.permutation(m2).astype(np.int64)
    nq = 50_000
    pick = rng.integers(0, len(ids), nq)
    group = np.where(rng.random(nq) < 0.1, NULL, ids[pick])
    q = rng.integers(-10, 1010, nq)
    got = seg_search(eng, q, t, False, NULL, group=group, seg=seg[: 2 * m2], rows=rows)
    has = group != NULL
    idx = R.search(t, np.where(has, starts[pick], 0), np.where(has, counts[pick], 0), q)
    want = np.where(idx >= 0, rows[np.where(idx >= 0, np.where(has, starts[pick], 0) + idx, 0)], NULL)
    assert np.array_equal(got, want)


def big_sides(rng, shape, nl, nr):
    if shape == "skewed":  # one group of 1e6 rows beside 1e5 groups of one
        rk = rng.permutation(np.concatenate([np.zeros(nr - 100_000, np.int64), np.arange(1, 100_001)]))
        lk = np.where(rng.random(nl) < 0.5, 0, rng.integers(0, 120_000, nl))
        return [lk], [rk]
    if shape == "wide":  # tuples whose ranges do not multiply into 64 bits: the row-hash route
        wide = [rng.integers(-(2**62), 2**62, 5000) for _ in range(3)]
        pl, pr = rng.integers(0, 5000, nl), rng.integers(0, 4000, nr)
        return [w[pl] for w in wide], [w[pr] for w in wide]
    nk = {"one_key": 1, "two_keys": 2}[shape]
    return [rng.integers(0, 3000, nl) for _ in range(nk)], [rng.integers(0, 3000, nr) for _ in range(nk)]


@pytest.mark.parametrize("sort_right", [True, False])
@pytest.mark.parametrize("shape,nl,nr", [("one_key", 1_000_003, 2_000_001), ("two_keys", 500_000, 700_001), ("wide", 300_000, 300_000),
                                         ("skewed", 800_000, 1_100_000), ("one_key", 70_001, 65), ("one_key", 65, 70_001)])
def test_planner_equals_the_restatement(eng, shape, nl, nr, sort_right):
    rng = np.random.default_rng(nl + nr + sort_right)
    lk, rk = big_sides(rng, shape, nl, nr)
    lt, rt = rng.integers(0, 10_000_000, nl), rng.integers(0, 10_000_000, nr)
    if sort_right:
        rt = np.sort(rt)
    for a in (lk[0], rk[0], lt, rt):
        a[rng.random(len(a)) < 0.001] = NULL
    want = R.asof_index(lk, lt, rk, rt)
    names = [f"k{i}" for i in range(len(lk))]
    left = {**{n: eng.column(c) for n, c in zip(names, lk)}, "t": eng.column(lt)}
    right = {**{n: eng.column(c) for n, c in zip(names, rk)}, "t": eng.column(rt)}
    before = [eng.xstat(s) for s in (L.RFX_XSTAT_ASOF_JOINS, L.RFX_XSTAT_SEARCHES, L.RFX_XSTAT_SORTS, L.RFX_XSTAT_BINS)]
    got = eng.asof_index(names, "t", left, right).cpu().numpy()
    after = [eng.xstat(s) for s in (L.RFX_XSTAT_ASOF_JOINS, L.RFX_XSTAT_SEARCHES, L.RFX_XSTAT_SORTS, L.RFX_XSTAT_BINS)]
    assert np.array_equal(got, want), (shape, nl, nr, sort_right, int((got != want).sum()))
    assert (want != NULL).any() and (nl < 1000 or (want == NULL).any())  # (the inputs exercise both outcomes)
    assert [a - b for a, b in zip(after, before)] == [1, nl, 1, 0]


def test_counters_of_bin_and_empty_sides(eng):
    x, y = eng.column(np.arange(100)), eng.column(np.arange(7))
    before = [eng.xstat(s) for s in (L.RFX_XSTAT_ASOF_JOINS, L.RFX_XSTAT_SEARCHES, L.RFX_XSTAT_BINS)]
    eng.bin(x, y)
    eng.binr(x, y)
    assert eng.bin(x, eng.empty(0)).numel() == 0  # (no launch, not counted)
    assert [eng.xstat(s) - b for s, b in zip((L.RFX_XSTAT_ASOF_JOINS, L.RFX_XSTAT_SEARCHES, L.RFX_XSTAT_BINS), before)] == [0, 14, 2]
    ns = [eng.xstat(s) for s in (L.RFX_XSTAT_NS_ASOF_BUILD, L.RFX_XSTAT_NS_ASOF_PROBE)]
    c = eng.column(np.arange(5000) % 7)
    eng.asof_index(["k"], "t", {"k": c, "t": c}, {"k": c, "t": c})
    assert eng.xstat(L.RFX_XSTAT_NS_ASOF_BUILD) > ns[0] and eng.xstat(L.RFX_XSTAT_NS_ASOF_PROBE) > ns[1]


def test_sharded_asof_join_is_refused_with_its_reason():
    e = Engine(0, shards=2)
    try:
        c = torch.arange(1000, device="cuda:0")
        with pytest.raises(RfxError, match="asof join over a sharded table"):
            e.asof_index(["k"], "t", {"k": c, "t": c}, {"k": c, "t": c})
        with pytest.raises(RfxError, match="bin over a sharded table"):
            e.bin(c, c)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- the fixture through Engine
def test_fixture_index_cases_through_engine(eng):
    gold = np.load(GOLD)
    for ci in range(len(gold["index_cases"])):
        name, lk, lt, rk, rt, ids = index_case(gold, ci)
        names = [f"k{i}" for i in range(len(lk))]
        left = {**{n: eng.column(c) for n, c in zip(names, lk)}, "t": eng.column(lt)}
        right = {**{n: eng.column(c) for n, c in zip(names, rk)}, "t": eng.column(rt)}
        got = eng.asof_index(names, "t", left, right).cpu().numpy()
        assert np.array_equal(got, ids), name


def test_fixture_tables_through_engine(eng):
    gold = np.load(GOLD)
    done = 0
    for ci in range(len(gold["table_cases"])):
        name, keys, left, right, want = table_case(gold, ci)
        if left["t"][1] == R.T_TIME:
            continue  # (Engine takes 8-byte device columns; the 4-byte asof column goes through the door below)
        as_dev = lambda cols: {n: eng.column(v.view(np.float64) if t == R.T_F64 else v) for n, (v, t) in cols.items()}
        got = eng.asof_join(keys, as_dev(left), as_dev(right))
        assert list(got) == list(want), name
        for col, (cells, nul, t) in want.items():
            src_t = (right.get(col) or left[col])[1]
            exp = np.where(nul == 1, R.typed_null(src_t), cells)
            assert np.array_equal(got[col].cpu().numpy().view(np.int64), exp), (name, col)
        done += 1
    assert done >= 8


def test_fixture_bin_cases_through_engine(eng):
    gold = np.load(GOLD)
    for ci, case in enumerate(gold["bin_cases"]):
        x, y = eng.column(gold[f"b{ci}_x"]), eng.column(gold[f"b{ci}_y"])
        assert np.array_equal(eng.bin(x, y).cpu().numpy(), gold[f"b{ci}_bin"]), case
        assert np.array_equal(eng.binr(x, y).cpu().numpy(), gold[f"b{ci}_binr"]), case


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
    data = np.ascontiguousarray(cells.astype(np.int32) if t in (4, 7, 8) else cells)
    if cells.size:
        C.memmove(H.payload(o), data.ctypes.data, data.nbytes)
    return o


def raw_cells(o):
    h = H.header(o)
    if h.type in (4, 7, 8):
        return np.frombuffer((C.c_char * (h.len * 4)).from_address(H.payload(o)), dtype=np.int32).astype(np.int64)
    return np.frombuffer((C.c_char * (h.len * 8)).from_address(H.payload(o)), dtype=np.int64).copy()


def host_table(ops, cols, syms):
    return ops.rfx_host_table(H.symbols(list(cols)), H.list_of([host_vector(ops, syms[v] if t == R.T_SYMBOL and syms is not None else v, t) for v, t in cols.values()]))


def asof_join(ops, keys, lt, rt):
    ks = H.symbols(keys)
    return ops.rfx_asof_join((C.c_void_p * 3)(ks, lt, rt), 3), ks


def test_fixture_tables_through_the_operator(ops):
    gold = np.load(GOLD)
    syms = np.array([ops.rfx_host_intern(str(s).encode(), len(str(s))) for s in gold["symbols"]], np.int64)
    back = {int(s): i for i, s in enumerate(syms)}
    for ci in range(len(gold["table_cases"])):
        name, keys, left, right, want = table_case(gold, ci)
        lt, rt = host_table(ops, left, syms), host_table(ops, right, syms)
        stats0 = H.to_numpy(ops.rfx_stats(None))
        r, ks = asof_join(ops, keys, lt, rt)
        assert not H.is_error(r), (name, H.error_text(r))
        assert H.header(r).type == H.T_TABLE
        nl = len(left["t"][0])
        assert ops.rfx_last_asof_on_gpu() == int(nl > 0), name
        stats1 = H.to_numpy(ops.rfx_stats(None))
        assert len(stats1) == 17 and stats1[2] - stats0[2] == int(nl > 0) and stats1[3] - stats0[3] == 0, name  # ST_JOIN_GPU / ST_JOIN_DELEGATED (an empty left table: neither)
        rk, rv = H.list_items(r)
        assert [ops.rfx_host_symbol_name(int(s)).decode() for s in raw_cells(rk)] == list(want), name
        for (col, (cells, nul, t)), c in zip(want.items(), H.list_items(rv)):
            src_t = (right.get(col) or left[col])[1]
            assert H.header(c).type == src_t and H.header(c).len == nl, (name, col)  # (typed also where the reference returns a LIST)
            got = raw_cells(c)
            exp = np.where(nul == 1, R.typed_null(src_t), cells)
            if src_t == R.T_SYMBOL:
                got = np.array([back[int(s)] for s in got], np.int64)
            assert np.array_equal(got, exp), (name, col)
        for o in (r, lt, rt, ks):
            ops.rfx_host_drop(o)


def test_fixture_bin_cases_through_the_operators(ops):
    gold = np.load(GOLD)
    for ci, case in enumerate(gold["bin_cases"]):
        t = int(str(case).split("|")[1])
        for verb in ("bin", "binr"):
            x, y = host_vector(ops, gold[f"b{ci}_x"], t), host_vector(ops, gold[f"b{ci}_y"], t)
            r = getattr(ops, "rfx_" + verb)(x, y)
            assert not H.is_error(r), (case, H.error_text(r))
            assert H.header(r).type == R.T_I64 and H.header(r).attrs == 0, case
            assert np.array_equal(raw_cells(r), gold[f"b{ci}_{verb}"]), (case, verb)
            assert ops.rfx_last_asof_on_gpu() == int(len(gold[f"b{ci}_y"]) > 0), case
            for o in (r, x, y):
                ops.rfx_host_drop(o)


def test_shapes_outside_the_device_path_are_handed_back(ops):
    # (standalone: no host verb behind the door, so an error object naming the reason -- never an answer of ours)
    n = 10
    i64 = lambda: np.arange(n, dtype=np.int64)

    def refused(keys, left, right, why, nargs=3):
        lt, rt = (host_table(ops, t, None) if isinstance(t, dict) else t for t in (left, right))
        ks = H.symbols(keys) if isinstance(keys, list) else keys
        bx, by = H.vector(i64()), H.vector(i64())
        b = ops.rfx_bin(bx, by)
        assert ops.rfx_last_asof_on_gpu() == 1
        st0 = H.to_numpy(ops.rfx_stats(None))
        r = ops.rfx_asof_join((C.c_void_p * 3)(ks, lt, rt), nargs)
        st1 = H.to_numpy(ops.rfx_stats(None))
        assert H.is_error(r), why
        assert ops.rfx_last_asof_on_gpu() == 0, why
        assert why in ops.rfx_ops_last_error().decode(), (why, ops.rfx_ops_last_error().decode())
        assert st1[2] == st0[2] and st1[3] - st0[3] == 1, why  # (a hand-over counts as a delegated join)
        for o in (r, ks, lt, rt, b, bx, by):
            ops.rfx_host_drop(o)

    base = {"s": (i64(), R.T_I64), "t": (i64(), R.T_I64), "v": (i64(), R.T_I64)}
    with_ = lambda **kw: {**base, **kw}
    refused(["s", "t"], with_(t=(i64(), R.T_F64)), with_(t=(i64(), R.T_F64)), "asof column type")
    refused(["s", "t"], with_(t=(i64(), R.T_SYMBOL)), with_(t=(i64(), R.T_SYMBOL)), "asof column type")
    refused(["s", "t"], with_(t=(i64(), R.T_TIMESTAMP)), base, "asof columns of different types")
    refused(["s", "t"], {"s": base["s"], "v": base["v"]}, base, "asof column missing from a table")
    refused(["s", "t"], base, {"s": base["s"], "v": base["v"]}, "asof column missing from a table")
    refused(["t"], base, base, "fewer than two key names")
    refused(["s", "t"], base, base, "expected (keys, left table, right table)", nargs=2)
    refused(H.vector(i64()), base, base, "expected (symbol vector, table, table)")
    refused(["s", "t"], H.vector(i64()), base, "expected (symbol vector, table, table)")
    refused(["s", "t"], with_(s=(i64(), R.T_F64)), with_(s=(i64(), R.T_F64)), "equality key is not an 8-byte integer column of both tables")
    refused(["s", "t"], with_(s=(i64(), R.T_TIME)), with_(s=(i64(), R.T_TIME)), "equality key is not an 8-byte integer column of both tables")
    refused(["s", "t"], with_(s=(i64(), R.T_SYMBOL)), base, "equality key is not an 8-byte integer column of both tables")
    refused(["s", "t"], with_(v=(i64(), R.T_TIME)), base, "non-8-byte column")
    refused(["s", "t"], base, with_(w=(i64(), 4)), "non-8-byte column")
    many = {**base, **{f"c{i}": (i64(), R.T_I64) for i in range(62)}}
    refused(["s", "t"], many, base, "too many columns")
    refused(["s"] + [f"c{i}" for i in range(8)] + ["t"], many, many, "more than 8 equality keys")
    # the 4-byte asof column's own vector OBJECT under a second name -- (table [s t qt v] (list S T T V)) -- is a passenger like any other: the exemption
    # of the asof column is by name (a gathered copy would be 8-byte cells written into a 4-byte vector)
    tcol = lambda: (i64(), R.T_TIME)

    def aliased(extra):
        cols = {"s": base["s"], "t": tcol(), "v": base["v"]}
        objs = {k: host_vector(ops, v, t) for k, (v, t) in cols.items()}
        names = list(cols) + [extra]
        return ops.rfx_host_table(H.symbols(names), H.list_of([objs[k] for k in cols] + [ops.rfx_host_clone(objs["t"])]))

    plain = lambda: {"s": base["s"], "t": tcol(), "v": base["v"]}
    refused(["s", "t"], plain(), aliased("qt"), "non-8-byte column")
    refused(["s", "t"], aliased("lt2"), plain(), "non-8-byte column")
    refused(["s", "t"], aliased("t2"), aliased("t2"), "non-8-byte column")
    # a column of both tables with two types is the join's own type error (select_column, core/join.c:50-51)
    lt, rt = host_table(ops, base, None), host_table(ops, with_(v=(i64(), R.T_F64)), None)
    st0 = H.to_numpy(ops.rfx_stats(None))
    r, ks = asof_join(ops, ["s", "t"], lt, rt)
    assert H.is_error(r) and "different types" in H.error_text(r) and ops.rfx_last_asof_on_gpu() == 0
    assert np.array_equal(H.to_numpy(ops.rfx_stats(None))[2:4], st0[2:4])  # (answered here, nothing handed over: neither join counter)
    for o in (r, ks, lt, rt):
        ops.rfx_host_drop(o)
    # bin / binr: atoms, 4-byte vectors, mixed and other types
    for verb in ("rfx_bin", "rfx_binr"):
        for x, y in ((H.vector(i64()), ops.rfx_host_i64(3)), (host_vector(ops, i64(), R.T_TIME), host_vector(ops, i64(), R.T_TIME)),
                     (host_vector(ops, i64(), R.T_I64), host_vector(ops, i64(), R.T_TIMESTAMP)), (host_vector(ops, i64(), R.T_F64), host_vector(ops, i64(), R.T_F64))):
            bx, by = H.vector(i64()), H.vector(i64())
            b = ops.rfx_bin(bx, by)
            assert ops.rfx_last_asof_on_gpu() == 1
            r = getattr(ops, verb)(x, y)
            assert H.is_error(r) and ops.rfx_last_asof_on_gpu() == 0
            assert "operands are not two I64 or two TIMESTAMP vectors" in ops.rfx_ops_last_error().decode()
            for o in (r, x, y, b, bx, by):
                ops.rfx_host_drop(o)


def test_a_million_rows_through_the_operator(ops):
    rng = np.random.default_rng(21)
    nl, nr = 1_000_000, 1_500_000
    left = {"s": (rng.integers(0, 5000, nl), R.T_SYMBOL), "t": (rng.integers(0, 86_400_000, nl), R.T_TIME), "q": (rng.integers(0, 100, nl), R.T_I64)}
    right = {"s": (rng.integers(0, 5000, nr), R.T_SYMBOL), "t": (np.sort(rng.integers(0, 86_400_000, nr)), R.T_TIME),
             "bid": (rng.standard_normal(nr).view(np.int64), R.T_F64), "q": (rng.integers(100, 200, nr), R.T_I64)}
    want = R.asof_join(["s", "t"], left, right)
    lt, rt = host_table(ops, left, np.arange(5000, dtype=np.int64)), host_table(ops, right, np.arange(5000, dtype=np.int64))
    r, _ = asof_join(ops, ["s", "t"], lt, rt)
    assert not H.is_error(r), H.error_text(r)
    assert ops.rfx_last_asof_on_gpu() == 1
    for (col, (cells, nul, t)), c in zip(want.items(), H.list_items(H.list_items(r)[1])):
        assert H.header(c).type == t, col
        assert np.array_equal(raw_cells(c), np.where(nul == 1, R.typed_null(t), cells)), col
    assert want["bid"][1].any() and not want["bid"][1].all()
    for o in (r, _, lt, rt):
        ops.rfx_host_drop(o)


_SHARDED_DOOR = '''
import ctypes as C, sys
sys.path.insert(0, ROOT)
import numpy as np
from rayforce_amd import hostobj as H
ops = H.lib()
ops.rfx_host_bind()
n = 1000
col = lambda: np.arange(n, dtype=np.int64) % 9
lt, rt, ks = H.table({"s": col(), "t": col(), "v": col()}), H.table({"s": col(), "t": col(), "w": col()}), H.symbols(["s", "t"])
r = ops.rfx_asof_join((C.c_void_p * 3)(ks, lt, rt), 3)
assert H.is_error(r) and ops.rfx_last_asof_on_gpu() == 0, H.error_text(r)
assert "asof join over a sharded table" in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error().decode()
x, y = H.vector(col()), H.vector(col())
for verb in (ops.rfx_bin, ops.rfx_binr):
    r = verb(x, y)
    assert H.is_error(r) and ops.rfx_last_asof_on_gpu() == 0
    assert "bin over a sharded table" in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error().decode()
print("SHARDED-ASOF-DOOR-OK")
'''


def test_the_door_hands_sharded_columns_back(built):
    """RFX_SHARDS=2 in a process of its own (the operator layer's shards are fixed at its first call): the three verbs are the host's, and without a
    host an error object naming the reason"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RFX_SHARDS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {root!r}\n" + _SHARDED_DOOR], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "SHARDED-ASOF-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
