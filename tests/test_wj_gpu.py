"""window-join / window-join1 on the GPU, all by equality of bits: every case of the reference's fixture (tests/golden/wj_golden.npz) through
Engine.window_join and through rfx_window_join / rfx_window_join1 with host objects, both verbs, all seven aggregates over an I64 and an F64 column;
the shapes handed back to the host with their reasons; the counters; two million trades against four million quotes against the numpy restatement
(tests/wj_ref.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wj_ref as R
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError
from test_wj_cpu import GOLD

pytestmark = pytest.mark.gpu
T_I64, T_SYMBOL, T_TIME, T_TIMESTAMP, T_F64, T_DATE, T_I32 = 5, 6, 8, 9, 10, 7, 4
AGG_NAMES = {f"{a}_{x}": (a, "v" + x) for x in "if" for a in R.AGGS}


def gold_cases():
    gold = np.load(GOLD)
    return [R.load_case(gold, ci) for ci in range(len(gold["cases"]))]


# ---------------------------------------------------------------------------------------------------- Engine
def test_every_fixture_case_through_engine(eng):
    done = 0
    for c in gold_cases():
        nk = c["nk"]
        names = [f"k{j}" for j in range(nk)]
        left = {**{n: eng.column(k) for n, k in zip(names, c["lk"])}, "t": eng.column(R.widen(c["lt"]))}
        right = {**{n: eng.column(k) for n, k in zip(names, c["rk"])}, "t": eng.column(R.widen(c["rt"])), "vi": eng.column(c["vi"]), "vf": eng.column(c["vf"])}
        windows = (eng.column(R.widen(c["lo"])), eng.column(R.widen(c["hi"])))
        for closed in (0, 1):
            got = eng.window_join(names + ["t"], windows, left, right, AGG_NAMES, closed=bool(closed))
            assert list(got) == names + ["t"] + list(AGG_NAMES), c["name"]
            for n in names + ["t"]:
                assert got[n] is left[n]
            for name, (a, col) in AGG_NAMES.items():
                want = c["out"][closed][col][a]
                g = got[name].cpu().numpy()
                assert g.dtype == (np.int64 if a == "count" or (col == "vi" and a != "avg") else np.float64), (c["name"], name)
                assert np.array_equal(g.view(np.int64), want), (c["name"], closed, name, int((g.view(np.int64) != want).sum()))
            done += 1
    assert done == 2 * len(np.load(GOLD)["cases"])


def test_ranges_stats_choose_the_fold_and_presorted_columns_fold_the_same(eng):
    """the (li, ri) pass counts the windows a lane does not fold; a column handed over in the sorted order already folds to the same cells"""
    from rayforce_amd import joins
    c = {x["name"]: x for x in gold_cases()}["window_lengths"]
    left, right = {"k": eng.column(c["lk"][0])}, {"k": eng.column(c["rk"][0]), "t": eng.column(R.widen(c["rt"]))}
    perm, li, ri, nlong, longest = joins.window_ranges(eng, ["k"], "t", (eng.column(R.widen(c["lo"])), eng.column(R.widen(c["hi"]))), left, right, closed=True)
    _, wli, wri = R.window_ranges(c["lk"], c["rk"], c["lo"], c["hi"], c["rt"], 1)
    lens = np.where(wli < 0, 0, wri - wli + 1)
    assert nlong == int((lens > 16).sum()) and longest == int(lens.max())
    assert np.array_equal(li.cpu().numpy(), wli) and np.array_equal(ri.cpu().numpy(), wri)  # (one group: the positions are the restatement's)
    v = eng.column(c["vf"])
    a = joins.window_fold(eng, v, perm, li, ri, nlong, R.AGGS)
    b = joins.window_fold(eng, v[perm].contiguous(), None, li, ri, nlong, R.AGGS)
    lanes = joins.window_fold(eng, v, perm, li, ri, 0, R.AGGS)  # (the count only decides how many rows go to a wave, never an answer)
    for k in R.AGGS:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) and torch.equal(a[k].view(torch.int64), lanes[k].view(torch.int64)), k
    short = lens <= 16  # a table whose every window is a lane's
    few = {"k": eng.column(c["lk"][0][short])}
    perm, li, ri, nlong, longest = joins.window_ranges(eng, ["k"], "t", (eng.column(R.widen(c["lo"][short])), eng.column(R.widen(c["hi"][short]))), few, right, closed=True)
    assert nlong == 0 and longest == int(lens[short].max())
    s = joins.window_fold(eng, v, perm, li, ri, 0, R.AGGS)
    for k in R.AGGS:
        assert np.array_equal(s[k].cpu().numpy().view(np.int64), a[k].cpu().numpy().view(np.int64)[short]), k


def test_engine_refuses_what_it_does_not_take(eng):
    c = torch.arange(100, device="cuda:0")
    f = c.to(torch.float64)
    t = {"k": c, "t": c, "v": c, "f": f}
    with pytest.raises(RfxError, match="at least one equality key"):
        eng.window_join(["t"], (c, c), t, t, {"a": ("sum", "v")})
    with pytest.raises(RfxError, match="i64-like"):
        eng.window_join(["k", "t"], (f, c), t, t, {"a": ("sum", "v")})
    with pytest.raises(RfxError, match="is not one of"):
        eng.window_join(["k", "t"], (c, c), t, t, {"a": ("med", "v")})
    with pytest.raises(RfxError, match="no column"):
        eng.window_join(["k", "t"], (c, c), t, t, {"a": ("sum", "nope")})
    e = Engine(0, shards=2)
    try:
        with pytest.raises(RfxError, match="window join over a sharded table"):
            e.window_join(["k", "t"], (c, c), t, t, {"a": ("sum", "v")})
    finally:
        e.close()


def test_two_million_trades_against_four_million_quotes(eng):
    rng = np.random.default_rng(77)
    nl, nr, nsym = 2_000_000, 4_000_000, 3000
    lk, rk = rng.integers(0, nsym + 30, nl), rng.integers(0, nsym, nr)  # (30 symbols the quotes lack)
    lt, rt = rng.integers(0, 10_000_000, nl), rng.integers(0, 10_000_000, nr)
    lo, hi = lt - rng.integers(0, 80_000, nl), lt + rng.integers(0, 80_000, nl)
    wide = rng.choice(nl, 400, replace=False)  # a few windows over most of a group: a wave's
    lo[wide], hi[wide] = rng.integers(-5, 2_000_000, 400), rng.integers(8_000_000, 10_000_005, 400)
    vi = rng.integers(-(2**40), 2**40, nr)
    vi[rng.random(nr) < 0.02] = R.NULL
    for a in (lo, hi, rt):
        a[rng.random(len(a)) < 0.001] = R.NULL32
    left = {"s": eng.column(lk), "t": eng.column(lt)}
    right = {"s": eng.column(rk), "t": eng.column(R.widen(rt)), "v": eng.column(vi)}
    windows = (eng.column(R.widen(lo)), eng.column(R.widen(hi)))
    aggs = {a: (a, "v") for a in ("sum", "min", "max", "count", "first", "last")}
    for closed in (0, 1):
        got = eng.window_join(["s", "t"], windows, left, right, aggs, closed=bool(closed))
        want = R.window_join([lk], [rk], lo, hi, rt, closed, {"v": vi}, aggs=tuple(aggs))
        counts = want[("count", "v")]
        assert (counts == 0).any() and (counts > 1000).any() and ((counts > 0) & (counts <= 16)).any() and ((counts > 16) & (counts < 200)).any()
        for a in aggs:
            g = got[a].cpu().numpy()
            assert np.array_equal(g, want[(a, "v")]), (closed, a, int((g != want[(a, "v")]).sum()))


# ---------------------------------------------------------------------------------------------------- the door
@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    o.rfx_host_bind()
    return o


def host_vector(ops, cells, t):
    cells = np.asarray(cells)
    o = ops.rfx_host_vector(t, cells.size)
    data = np.ascontiguousarray(cells.astype(np.int32) if t in (T_I32, T_DATE, T_TIME) else cells)
    if cells.size:
        C.memmove(H.payload(o), data.ctypes.data, data.nbytes)
    return o


def raw_cells(o):
    h = H.header(o)
    if h.type in (T_I32, T_DATE, T_TIME):
        return np.frombuffer((C.c_char * (h.len * 4)).from_address(H.payload(o)), dtype=np.int32).astype(np.int64)
    return np.frombuffer((C.c_char * (h.len * 8)).from_address(H.payload(o)), dtype=np.int64).copy()


def host_table(ops, cols):
    """cols: {name: (cells, type)}"""
    return ops.rfx_host_table(H.symbols(list(cols)), H.list_of([host_vector(ops, v, t) for v, t in cols.values()]))


def agg_dict(ops, aggs, by_name=False):
    """{name: (agg, col)} -> DICT of (agg col) lists: the head a function object, as the parser leaves it, or (by_name) the aggregate's symbol"""
    vals = [H.list_of([H.atom(a), H.atom(col)]) if by_name else H.expr((a, col)) for a, col in aggs.values()]
    return ops.rfx_host_dict(H.symbols(list(aggs)), H.list_of(vals))


def window_join(ops, closed, keys, wins, lt, rt, d, nargs=5):
    ks = H.symbols(keys) if isinstance(keys, list) else keys
    fn = ops.rfx_window_join1 if closed else ops.rfx_window_join
    return fn((C.c_void_p * 5)(ks, wins, lt, rt, d), nargs), ks


def case_tables(ops, c, syms, ttype=T_TIME):
    names = [f"k{j}" for j in range(c["nk"])]
    key = lambda cells, kind: (syms[cells] if kind == "sym" else cells, T_SYMBOL if kind == "sym" else T_I64)
    left = {**{n: key(k, kind) for n, k, kind in zip(names, c["lk"], c["kinds"])}, "t": (c["lt"], ttype)}
    right = {**{n: key(k, kind) for n, k, kind in zip(names, c["rk"], c["kinds"])}, "t": (c["rt"], ttype), "vi": (c["vi"], T_I64), "vf": (c["vf"].view(np.int64), T_F64)}
    wins = H.list_of([host_vector(ops, c["lo"], ttype), host_vector(ops, c["hi"], ttype)])
    return names, left, right, wins


def test_every_fixture_case_through_the_operators(ops):
    gold = np.load(GOLD)
    syms = np.array([ops.rfx_host_intern(str(s).encode(), len(str(s))) for s in gold["symbols"]], np.int64)
    for ci, c in enumerate(gold_cases()):
        nl = len(c["lt"])
        for closed in (0, 1):
            names, left, right, wins = case_tables(ops, c, syms, ttype=(T_TIME, T_I32, T_DATE)[ci % 3] if ci else T_TIME)
            lt, rt = host_table(ops, left), host_table(ops, right)
            d = agg_dict(ops, AGG_NAMES, by_name=(ci + closed) % 2 == 1)
            st0 = H.to_numpy(ops.rfx_stats(None))
            r, ks = window_join(ops, closed, names + ["t"], wins, lt, rt, d)
            st1 = H.to_numpy(ops.rfx_stats(None))
            assert not H.is_error(r), (c["name"], H.error_text(r))
            assert H.header(r).type == H.T_TABLE
            assert ops.rfx_last_window_on_gpu() == int(nl > 0), c["name"]
            assert st1[2] - st0[2] == int(nl > 0) and st1[3] - st0[3] == 0, c["name"]  # ST_JOIN_GPU / ST_JOIN_DELEGATED (an empty left table: neither)
            rk, rv = H.list_items(r)
            assert [ops.rfx_host_symbol_name(int(s)).decode() for s in raw_cells(rk)] == list(left) + list(AGG_NAMES), c["name"]
            cols = H.list_items(rv)
            for (n, (cells, t)), o in zip(left.items(), cols):
                assert H.header(o).type == t and np.array_equal(raw_cells(o), cells), (c["name"], n)
            for (name, (a, col)), o in zip(AGG_NAMES.items(), cols[len(left):]):
                want_t = T_I64 if a == "count" or (col == "vi" and a != "avg") else T_F64
                assert H.header(o).type == want_t and H.header(o).len == nl, (c["name"], name)
                want = c["out"][closed][col][a]
                got = raw_cells(o)
                assert np.array_equal(got, want), (c["name"], closed, name, int((got != want).sum()))
            for o in (r, ks, wins, lt, rt, d):
                ops.rfx_host_drop(o)


def test_shapes_outside_the_device_path_are_handed_back(ops):
    # (standalone: no host verb behind the door, so an error object naming the reason -- never an answer of ours)
    n = 10
    i64 = lambda: np.arange(n, dtype=np.int64)
    base = {"s": (i64(), T_I64), "t": (i64(), T_TIME), "v": (i64(), T_I64), "f": (i64(), T_F64)}
    with_ = lambda **kw: {**base, **kw}
    win = lambda t=T_TIME, m=n: H.list_of([host_vector(ops, np.arange(m), t), host_vector(ops, np.arange(m) + 3, t)])
    good = lambda: agg_dict(ops, {"a": ("min", "v")})

    def answered():
        lt, rt, w, d = host_table(ops, base), host_table(ops, base), win(), good()
        r, ks = window_join(ops, 0, ["s", "t"], w, lt, rt, d)
        assert not H.is_error(r) and ops.rfx_last_window_on_gpu() == 1
        for o in (r, ks, lt, rt, w, d):
            ops.rfx_host_drop(o)

    def refused(why, keys=None, left=None, right=None, wins=None, d=None, nargs=5, closed=0):
        answered()
        lt, rt = (host_table(ops, t) if isinstance(t, dict) else t for t in (left or base, right or base))
        w = wins if wins is not None else win()
        d = d if d is not None else good()
        st0 = H.to_numpy(ops.rfx_stats(None))
        r, ks = window_join(ops, closed, keys or ["s", "t"], w, lt, rt, d, nargs)
        st1 = H.to_numpy(ops.rfx_stats(None))
        assert H.is_error(r), why
        assert ops.rfx_last_window_on_gpu() == 0, why
        err = ops.rfx_ops_last_error().decode()
        assert why in err and ("window_join1" if closed else "window_join:") in err, (why, err)
        assert st1[2] == st0[2] and st1[3] - st0[3] == 1, why  # (a hand-over counts as a delegated join)
        for o in (r, ks, lt, rt, w, d):
            ops.rfx_host_drop(o)

    # raw columns, med / dev, nested expressions, other value types
    raw = lambda: ops.rfx_host_dict(H.symbols(["bids"]), H.list_of([H.atom("v")]))
    refused("a raw column or an atom", d=raw())
    refused("a raw column or an atom", d=raw(), closed=1)
    refused("an aggregate other than sum, min, max, count, avg, first, last", d=agg_dict(ops, {"a": ("med", "v")}))
    refused("an aggregate other than sum, min, max, count, avg, first, last", d=agg_dict(ops, {"a": ("dev", "v")}, by_name=True))
    refused("an aggregate of an expression", d=ops.rfx_host_dict(H.symbols(["a"]), H.list_of([H.expr(("sum", ("+", "v", "v")))])))
    refused("an aggregate is not of the form (agg column)", d=ops.rfx_host_dict(H.symbols(["a"]), H.list_of([H.expr(("+", "v", "v"))])))
    refused("an aggregate of a column the right table lacks", d=agg_dict(ops, {"a": ("sum", "nope")}))
    for t in (T_TIMESTAMP, T_SYMBOL, T_TIME, T_I32):
        refused("an aggregate of a column that is neither I64 nor F64", right=with_(v=(i64(), t)))
    # an 8-byte window column, whatever the reference answers; window columns missing or of two types
    for t in (T_I64, T_TIMESTAMP, T_F64):
        refused("window column type", left=with_(t=(i64(), t)), right=with_(t=(i64(), t)))
    refused("window columns of different types", left=with_(t=(i64(), T_DATE)))
    refused("window column missing from a table", right={"s": base["s"], "v": base["v"]})
    # the windows
    refused("windows are not a list of two vectors", wins=H.list_of([host_vector(ops, i64(), T_TIME)]))
    refused("windows are not two 4-byte integer vectors of the left table's length", wins=win(T_I64))
    refused("windows are not two 4-byte integer vectors of the left table's length", wins=win(T_TIME, n - 1))
    # keys
    refused("fewer than two key names", keys=["t"])
    refused("equality key is not an 8-byte integer column of both tables", left=with_(s=(i64(), T_F64)), right=with_(s=(i64(), T_F64)))
    refused("equality key is not an 8-byte integer column of both tables", left=with_(s=(i64(), T_SYMBOL)))
    many = {**base, **{f"c{i}": (i64(), T_I64) for i in range(9)}}
    refused("more than 8 equality keys", keys=[f"c{i}" for i in range(9)] + ["t"], left=many, right=many)
    # the reference's own arity and type errors
    refused("expected (keys, windows, left table, right table, aggregates)", nargs=4)
    refused("expected (symbol vector, list, table, table, dict)", keys=H.vector(i64()))
    refused("expected (symbol vector, list, table, table, dict)", wins=host_vector(ops, i64(), T_TIME))
    refused("expected (symbol vector, list, table, table, dict)", left=H.vector(i64()))
    refused("expected (symbol vector, list, table, table, dict)", d=H.list_of([H.atom("v")]))
    # a parted table: a column that is one vector per partition (type PARTEDLIST + I64)
    parts = H.list_of([H.vector(i64()[:5]), H.vector(i64()[5:])])
    H.header(parts).type = 77 + T_I64
    parted = ops.rfx_host_table(H.symbols(["s", "t", "v"]), H.list_of([parts, host_vector(ops, i64(), T_TIME), H.vector(i64())]))
    refused("parted table", right=parted)


_SHARDED_DOOR = '''
import ctypes as C, sys
sys.path.insert(0, ROOT)
import numpy as np
from rayforce_amd import hostobj as H
ops = H.lib()
ops.rfx_host_bind()
n = 1000
def tvec():
    o = ops.rfx_host_vector(8, n)
    a = (np.arange(n) % 9).astype(np.int32)
    C.memmove(H.payload(o), a.ctypes.data, a.nbytes)
    return o
col = lambda: np.arange(n, dtype=np.int64) % 9
tab = lambda: ops.rfx_host_table(H.symbols(["s", "t", "v"]), H.list_of([H.vector(col()), tvec(), H.vector(col())]))
d = ops.rfx_host_dict(H.symbols(["a"]), H.list_of([H.expr(("sum", "v"))]))
for fn in (ops.rfx_window_join, ops.rfx_window_join1):
    r = fn((C.c_void_p * 5)(H.symbols(["s", "t"]), H.list_of([tvec(), tvec()]), tab(), tab(), d), 5)
    assert H.is_error(r) and ops.rfx_last_window_on_gpu() == 0, H.error_text(r)
    assert "window join over a sharded table" in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error().decode()
print("SHARDED-WJ-DOOR-OK")
'''


def test_the_door_hands_sharded_columns_back(built):
    """RFX_SHARDS=2 in a process of its own (the operator layer's shards are fixed at its first call): both verbs are the host's, and without a host an
    error object naming the reason"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RFX_SHARDS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {root!r}\n" + _SHARDED_DOOR], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "SHARDED-WJ-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
