"""Sparse keys routed by the SAMPLE alone (gb_scope's `sparse_sampled`, rfx_exec_groupby.c): from 2^24 rows on a single I64 key whose sampled range
already exceeds the row count goes to the hashed tables without the exact scope pass, and the one thing that catches a null key the sample missed is
the tables' null entry, read back after the passes (gb_null_slot) -- cell `cap` of the array-per-field layout, cell `cap * W` of the PACKED one.

Every case runs at n = 2^24 + 12 345 rows (the planner's threshold is fixed) against plain numpy -- first-occurrence group order, counts by
bincount, i64 sums / max / first by reduceat over the rows sorted by group, f64 sums in long double held to 1e-9 of the group's sum of |x| --
and against the device itself under the exact scope (RFX_NO_SAMPLED_SCOPE=1) on everything that does not depend on the summation order.
RFX_XSTAT_SCOPE_SPARSE_SAMPLED proves which route answered.  The layouts: array-per-field at 2^22 slots (D = 1 000 keys) and grown to 2^26
(D = 4 000 000), with the first-row probe at both sizes (the grown one is packed by default), and -- in processes of their own --
RFX_EMIT_BY_ROWS=2 (packed at 2^22 slots) with and without RFX_NO_PACKED_TABLE=1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import rfo
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from test_gpu_parity import same_f64

gpu = pytest.mark.gpu

NULL = -(2**63)
N = (1 << 24) + 12_345
SPOT = 5 + 64 * 65_537  # the sample's stride is N >> 18 = 64 from row 0, plus 2^11 rows at both ends: this row is never sampled
KEY_MUL, KEY_OFF = 1_000_003, 1 << 45  # the key family: j * 1 000 003 - 2^45
# keys of that family whose home slot -- hash_index_u64(U64_HASH_SEED, key) & (cap - 1) -- is exactly cap / 2 and cap / 4: cell `cap` past the packed
# table's `first` cells is the first row of entry cap / 2 with zero aggregates (W = 2 cells an entry) and of entry cap / 4 with `sum` of an i64 column
# (W = 4: key, first row, sum, count), entries which these keys occupy; for W = 3 and W = 7 it is an accumulator or a count, never the empty marker;
# for W = 8 (`wide`) it is the first row of entry cap / 8, which no key of either key set reaches (test_entries_behind_the_layout_blind_address): the
# one width at which that address reads the EMPTY marker, so that a null key hidden from the sample goes unnoticed there
J_HOME_2_22, J_HOME_2_26 = 21_048_582, 50_783_221
J_QUARTER_2_22, J_QUARTER_2_26 = 3_744_714, 138_774_775
KEY_HOME_2_22, KEY_HOME_2_26 = J_HOME_2_22 * KEY_MUL - KEY_OFF, J_HOME_2_26 * KEY_MUL - KEY_OFF
KEY_QUARTER_2_22, KEY_QUARTER_2_26 = J_QUARTER_2_22 * KEY_MUL - KEY_OFF, J_QUARTER_2_26 * KEY_MUL - KEY_OFF
PLANTED = {KEY_HOME_2_22: (1_000, 7_000_003, N - 2), KEY_HOME_2_26: (2_001, 9_000_001, N - 5), KEY_QUARTER_2_22: (3_002, 11_000_005, N - 7),
           KEY_QUARTER_2_26: (4_003, 13_000_007, N - 9)}  # key -> its rows, in both key sets
D_SMALL, D_LARGE = 1_000, 4_000_000  # distinct keys: the 2^22-slot table holds them / reports full and grows to 2^26 slots
CUT = 500_000  # the filter `a < CUT` (a is uniform below 1 000 000; a[SPOT] = 999 999 is dropped by it)

REFUSE = L.RFX_Q_REFUSE_NULL_KEY
AGG_SETS = {"none": [], "sum_i64": [("sum", "a")], "sum_f64": [("sum", "v")], "four": [("sum", "a"), ("count", "a"), ("max", "a"), ("first", "a")]}
AGG_SETS["wide"] = AGG_SETS["four"] + AGG_SETS["sum_f64"]
# cells an entry of the hashed table: key, first row, one per aggregate, a count beside an i64 sum.  Cell `cap` past the `first` cells of a PACKED table
# -- what an address that ignores the layout reads -- is cell (cap + 1) % W of entry (cap + 1) // W: the first row of entry cap / 2, cap / 4, cap / 8
# for W = 2, 4, 8, an accumulator or a count for W = 3 and 7
WIDTH = {"none": 2, "sum_i64": 4, "sum_f64": 3, "four": 7, "wide": 8}
# layout -> (distinct keys, probe_first)
LAYOUTS = {"fields_small": (D_SMALL, False), "fields_grown": (D_LARGE, False), "probe_small": (D_SMALL, True), "probe_grown": (D_LARGE, True)}


def test_home_slots_of_the_committed_keys():
    """The premise of the W = 2 and W = 4 cases, without a GPU: the committed keys home at cap / 2 and cap / 4 of the 2^22- and the 2^26-slot table."""
    for key, cap, home in ((KEY_HOME_2_22, 1 << 22, 1 << 21), (KEY_HOME_2_26, 1 << 26, 1 << 25), (KEY_QUARTER_2_22, 1 << 22, 1 << 20), (KEY_QUARTER_2_26, 1 << 26, 1 << 24)):
        h = rfo.hash_index_u64(rfo.U64_HASH_SEED, np.array([key], np.int64).view(np.uint64))
        assert int(h[0] & np.uint64(cap - 1)) == home, (key, cap)
    assert SPOT % (N >> 18) != 0 and (1 << 11) <= SPOT < N - (1 << 11)


# ---------------------------------------------------------------- inputs and the numpy reference, once per module
def rows_by_key(k):
    """The rows with equal keys brought together, each key's in row order, by ONE sort: of (j << 25 | row), j = the key's place in its family."""
    n = len(k)
    j, rem = np.divmod(k + KEY_OFF, KEY_MUL)
    assert n < 1 << 25 and not rem.any() and int(j.min()) >= 0 and int(j.max()) < 1 << 38
    c = np.sort((j << 25) | np.arange(n, dtype=np.int64))
    return c & ((1 << 25) - 1), c >> 25


def reference(k, a, v, keep=None, by_key=None):
    """Plain numpy over the selected rows (`keep`: a boolean mask, None = all): groups in first-occurrence order, integers exactly, f64 sums in long
    double.  What np.unique(..., return_index=True, return_inverse=True) and a stable sort by group give (test_the_reference_against_np_unique), from
    rows_by_key's one sort: a tenth of the time at 2^24 rows."""
    n = len(k)
    rows, code = by_key if by_key is not None else rows_by_key(k)
    if keep is not None:
        m = keep[rows]
        rows, code = rows[m], code[m]
    starts = np.flatnonzero(np.concatenate(([True], code[1:] != code[:-1])))  # every group's first cell: its first row, rows being in row order
    groups = len(starts)
    order = np.argsort(rows[starts])  # groups by first occurrence
    rank = np.empty(groups, np.int64)
    rank[order] = np.arange(groups)
    per_row = np.repeat(rank, np.diff(np.concatenate((starts, [len(rows)]))))  # the group of every sorted row
    gid = np.full(n, -1, np.int64)
    gid[rows] = per_row
    aa = a[rows]
    vv = v[rows].astype(np.longdouble)
    return {"groups": groups, "keys": k[rows[starts]][order], "first": rows[starts][order], "gid": gid, "count": np.bincount(per_row, minlength=groups).astype(np.int64),
            "sum_a": np.add.reduceat(aa, starts)[order], "max_a": np.maximum.reduceat(aa, starts)[order], "first_a": aa[starts][order],
            "sum_v": np.add.reduceat(vv, starts)[order], "abs_v": np.add.reduceat(np.abs(vv), starts)[order]}


def test_the_reference_against_np_unique():
    """The reference's one-sort grouping, without a GPU: first-occurrence order from np.unique(..., return_index=True, return_inverse=True), counts by
    bincount, sums / max / first by reduceat over the rows sorted by group -- all rows and under a filter."""
    n = 300_007
    k = rfo.gen_i64(n, 31, 5_000) * KEY_MUL - KEY_OFF
    k[[17, 4_000, n - 1]] = KEY_HOME_2_26
    a, v = rfo.gen_i64(n, 2, 1_000_000), rfo.gen_f64(n, 5) - 0.25
    for keep in (None, a < CUT):
        rows = np.arange(n) if keep is None else np.flatnonzero(keep)
        uniq, idx, inv = np.unique(k[rows], return_index=True, return_inverse=True)
        order = np.argsort(idx, kind="stable")
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        gid = rank[inv.reshape(-1)]
        by_group = rows[np.argsort(gid, kind="stable")]
        count = np.bincount(gid, minlength=len(uniq))
        starts = np.concatenate(([0], np.cumsum(count)[:-1]))
        r = reference(k, a, v, keep)
        assert r["groups"] == len(uniq) and np.array_equal(r["keys"], uniq[order]) and np.array_equal(r["first"], rows[idx[order]])
        assert np.array_equal(r["gid"][rows], gid) and np.array_equal(r["count"], count) and (keep is None or np.all(r["gid"][~keep] == -1))
        assert np.array_equal(r["sum_a"], np.add.reduceat(a[by_group], starts)) and np.array_equal(r["max_a"], np.maximum.reduceat(a[by_group], starts))
        assert np.array_equal(r["first_a"], a[by_group][starts])
        vv = v[by_group].astype(np.longdouble)
        assert np.array_equal(r["sum_v"], np.add.reduceat(vv, starts)) and np.array_equal(r["abs_v"], np.add.reduceat(np.abs(vv), starts))


def host_keys(d):
    """The key column of `d` distinct keys (the oracle's generator: the same cells on any machine), the committed keys planted."""
    k = rfo.gen_i64(N, 31, d) * KEY_MUL - KEY_OFF
    for key, at in PLANTED.items():
        k[list(at)] = key
    return k


def occupied_entries(keys, cap):
    """The entries a linear-probing table of `cap` slots holds after `keys` (distinct) went in, in any order: the keys' home slots in ascending order, each
    pushed past its predecessor's place."""
    home = np.sort((rfo.hash_index_u64(rfo.U64_HASH_SEED, keys.view(np.uint64)) & np.uint64(cap - 1)).astype(np.int64))
    i = np.arange(len(home))
    at = np.maximum.accumulate(home - i) + i
    assert at[-1] < cap  # (no run wraps round the table's end)
    return at


def test_entries_behind_the_layout_blind_address():
    """Without a GPU: in both key sets, at the capacity their packed table has, the entries cap / 2 and cap / 4 are occupied (W = 2 and 4: a first row
    where the empty marker is expected -- a spurious report) and the entry cap / 8 is EMPTY (W = 8: the empty marker although a null key came by -- the
    hidden null goes unnoticed).  A row's key replaced by the null only takes a key away."""
    for d, cap in ((D_SMALL, 1 << 22), (D_LARGE, 1 << 26)):
        at = occupied_entries(np.unique(host_keys(d)), cap)
        assert np.isin([cap // 2, cap // 4, cap // 8], at).tolist() == [True, True, False], (d, cap)
    for name, aggs in AGG_SETS.items():  # the widths as rfx_hip_group_table_arrays counts them, + the key
        assert WIDTH[name] == 2 + len(aggs) + sum(fn == "sum" and col == "a" for fn, col in aggs), name


_DATA = {}


def dataset(eng, d):
    """Columns on the device (the value columns are shared by both key sets), their host copies, and the references: all rows / `a < CUT`."""
    if "a" not in _DATA:
        a = eng.gen_i64(N, 2, 1_000_000)
        a[SPOT] = 999_999
        v = eng.gen_f64(N, 5) - 0.25
        _DATA["a"], _DATA["v"] = a, v
        _DATA["ha"], _DATA["hv"] = a.cpu().numpy(), v.cpu().numpy()
    if d not in _DATA:
        hk = host_keys(d)
        k = eng.column(hk)
        ha, hv = _DATA["ha"], _DATA["hv"]
        by_key = rows_by_key(hk)
        _DATA[d] = {"t": {"k": k, "a": _DATA["a"], "v": _DATA["v"]}, "hk": hk, "all": reference(hk, ha, hv, None, by_key),
                    "cut": reference(hk, ha, hv, ha < CUT, by_key)}
    return _DATA[d]


@pytest.fixture(scope="module", autouse=True)
def _release_the_columns():
    yield
    _DATA.clear()


@pytest.fixture(scope="module")
def ops(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    l = H.lib()
    assert l.rfx_host_bind() == 0
    yield l
    l.rfx_cache_clear()


# ---------------------------------------------------------------- helpers
class Route:
    """The two planner counters of one query: did the sample alone route it, was the table grown."""

    def __init__(self, stat):
        self.stat = stat

    def __enter__(self):
        self.s0, self.g0 = self.stat(L.RFX_XSTAT_SCOPE_SPARSE_SAMPLED), self.stat(L.RFX_XSTAT_HASH_GROWN)
        return self

    def __exit__(self, *exc):
        self.sampled, self.grown = self.stat(L.RFX_XSTAT_SCOPE_SPARSE_SAMPLED) - self.s0, self.stat(L.RFX_XSTAT_HASH_GROWN) - self.g0
        return False


class exact_scope:
    def __enter__(self):
        os.environ["RFX_NO_SAMPLED_SCOPE"] = "1"

    def __exit__(self, *exc):
        del os.environ["RFX_NO_SAMPLED_SCOPE"]
        return False


def both(e, run, grown=False):
    """`run` under the sampled sparse route (the counter moved, the table grew if it should) and under the exact scope (the counter did not move)."""
    e.forget_scopes()
    with Route(e.xstat) as r:
        got = run()
    assert r.sampled >= 1, "the sample alone did not route this query"
    assert (r.grown >= 1) == grown, r.grown
    with Route(e.xstat) as r, exact_scope():
        want = run()
    assert r.sampled == 0
    return got, want


def refused(e, run):
    """`run` ends with RFX_EXEC_NULL_KEY under the sampled sparse route exactly as under the exact scope."""
    e.forget_scopes()
    with Route(e.xstat) as r:
        with pytest.raises(L.RfxError, match=r"failed with code 1\b"):
            run()
    assert r.sampled >= 1
    with Route(e.xstat) as r, exact_scope():
        with pytest.raises(L.RfxError, match=r"failed with code 1\b"):
            run()
    assert r.sampled == 0


def same_bits(r1, r2, aggs):
    """Two answers of the device agree bit for bit on everything that does not depend on the order of an f64 summation."""
    import torch
    assert r1["groups"] == r2["groups"] and r1["path"] == r2["path"]
    assert torch.equal(r1["keys"], r2["keys"]) and torch.equal(r1["first"], r2["first"])
    for (fn, col), x, y in zip(aggs, r1["results"], r2["results"]):
        if not (fn == "sum" and col == "v"):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), (fn, col)
    assert ("probe" in r1) == ("probe" in r2)
    if "probe" in r1:
        assert torch.equal(r1["probe"], r2["probe"])


def against(r, ref, aggs, probe_first, rows=None):
    """One answer of the device against the numpy reference: group order, keys, first rows, integer results and the per-row probe bit for bit."""
    assert r["groups"] == ref["groups"] and not r["dense"]
    assert np.array_equal(r["keys"].cpu().numpy(), ref["keys"])
    assert np.array_equal(r["first"].cpu().numpy(), ref["first"])
    for (fn, col), x in zip(aggs, r["results"]):
        x = x.cpu().numpy()
        if fn == "sum" and col == "v":
            assert x.dtype == np.float64
            same_f64(x, ref["sum_v"].astype(np.float64), scale=ref["abs_v"].astype(np.float64))
        else:
            want = ref[{"sum": "sum_a", "count": "count", "max": "max_a", "first": "first_a"}[fn]]
            assert x.dtype == np.int64 and np.array_equal(x, want), (fn, col)
    if probe_first:
        probe = r["probe"].cpu().numpy()
        sel = slice(None) if rows is None else rows  # (a row the filter drops has no group)
        assert np.array_equal(probe[sel], ref["first"][ref["gid"][sel]])


class planted:
    """A null key at row `spot` of the key column for the duration (the column is shared by the module's tests)."""

    def __init__(self, k, spot=SPOT):
        self.k, self.spot = k, spot

    def __enter__(self):
        self.keep = int(self.k[self.spot])
        self.k[self.spot] = NULL

    def __exit__(self, *exc):
        self.k[self.spot] = self.keep
        return False


# ---------------------------------------------------------------- the planner, one shard
@gpu
@pytest.mark.parametrize("aggs", list(AGG_SETS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_no_null_key(eng, layout, aggs):
    """No null key, RFX_Q_REFUSE_NULL_KEY: no report -- whatever cell of the table an address that ignores the layout would land on: an occupied first
    row (W = 2 and 4: the keys homed at cap / 2 and cap / 4), an accumulator or a count (W = 3 and 7), an empty entry's first row (W = 8) -- and the reference's answer."""
    d, probe = LAYOUTS[layout]
    D = dataset(eng, d)
    A = AGG_SETS[aggs]
    got, want = both(eng, lambda: eng.group_by("k", A, None, D["t"], flags=REFUSE, probe_first=probe), grown=d == D_LARGE)
    assert got["cap"] == (1 << 26 if d == D_LARGE else 1 << 22)
    against(got, D["all"], A, probe)
    same_bits(got, want, A)


@gpu
@pytest.mark.parametrize("aggs", list(AGG_SETS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_hidden_null_key_is_refused(eng, layout, aggs):
    """A null key at a row the sample does not read, RFX_Q_REFUSE_NULL_KEY: RFX_EXEC_NULL_KEY, as under the exact scope, at every entry width -- `wide`
    (W = 8) is the one at which an address that ignores the packed layout reads the empty marker and lets the null pass."""
    d, probe = LAYOUTS[layout]
    D = dataset(eng, d)
    A = AGG_SETS[aggs]
    with planted(D["t"]["k"]):
        refused(eng, lambda: eng.group_by("k", A, None, D["t"], flags=REFUSE, probe_first=probe))


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_hidden_null_key_is_a_group(eng, layout):
    """The same null without the flag: the null keys form one group of one row -- one more group than the reference's, unless the row's own key had
    no other row -- bit for bit as under the exact scope."""
    d, probe = LAYOUTS[layout]
    D = dataset(eng, d)
    ref, A = D["all"], AGG_SETS["four"]
    lost = int(ref["count"][ref["gid"][SPOT]]) == 1
    with planted(D["t"]["k"]):
        got, want = both(eng, lambda: eng.group_by("k", A, None, D["t"], flags=0, probe_first=probe), grown=d == D_LARGE)
    same_bits(got, want, A)
    assert got["groups"] == ref["groups"] + 1 - lost
    keys = got["keys"].cpu().numpy()
    at = np.flatnonzero(keys == NULL)
    assert len(at) == 1 and int(got["first"][at[0]]) == SPOT
    assert [int(x[at[0]]) for x in got["results"]] == [999_999, 1, 999_999, 999_999]  # sum, count, max, first of the one row (a[SPOT])
    assert int(got["results"][1].sum()) == N
    if probe:
        assert int(got["probe"][SPOT]) == SPOT


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_null_key_dropped_by_the_filter(eng, layout):
    """The same null under a filter that drops its row, RFX_Q_REFUSE_NULL_KEY: nothing to report, the reference's answer over the selected rows."""
    d, probe = LAYOUTS[layout]
    D = dataset(eng, d)
    A = AGG_SETS["wide"]
    with planted(D["t"]["k"]):
        got, want = both(eng, lambda: eng.group_by("k", A, ("<", "a", CUT), D["t"], flags=REFUSE, probe_first=probe), grown=d == D_LARGE)
    assert D["cut"]["groups"] > 3 << 20 or d == D_SMALL  # (the selected half still holds more keys than 3/4 of 2^22 slots: the table grows)
    rows = np.flatnonzero(_DATA["ha"] < CUT)
    against(got, D["cut"], A, probe, rows)
    same_bits(got, want, A)


# ---------------------------------------------------------------- three shards of one device
@gpu
def test_three_shards(eng):
    """The same route over 3 row-range shards (every shard samples its own rows; the tables are merged into the lead's): no null / a null in the LAST
    shard's rows only, at a row that shard's sample does not read."""
    from rayforce_amd.engine import Engine
    D = dataset(eng, D_SMALL)
    A = AGG_SETS["wide"]
    e = Engine(0, shards=3)
    try:
        r0, ln = C.c_int64(), C.c_int64()
        e.lib.rfx_exec_split(N, 3, 2, C.byref(r0), C.byref(ln))
        stride = ln.value >> 18
        local = 5 + stride * 65_537
        assert stride > 5 and (1 << 11) <= local < ln.value - (1 << 11)
        spot = r0.value + local
        got, want = both(e, lambda: e.group_by("k", A, None, D["t"], flags=REFUSE))
        against(got, D["all"], A, False)
        same_bits(got, want, A)
        assert e.xstat(L.RFX_XSTAT_MERGES_KERNEL) > 0
        with planted(D["t"]["k"], spot):
            refused(e, lambda: e.group_by("k", A, None, D["t"], flags=REFUSE))
            got, want = both(e, lambda: e.group_by("k", A, None, D["t"], flags=0))
        same_bits(got, want, A)
        keys = got["keys"].cpu().numpy()
        at = np.flatnonzero(keys == NULL)
        assert got["groups"] == D["all"]["groups"] + 1 and len(at) == 1
        assert int(got["first"][at[0]]) == spot and int(got["results"][1][at[0]]) == 1
    finally:
        e.close()


# ---------------------------------------------------------------- the layouts that are chosen once per process
KNOBS = ["RFX_EMIT_BY_ROWS=2", "RFX_EMIT_BY_ROWS=2,RFX_NO_PACKED_TABLE=1"]


@gpu
def test_probe_cases_in_processes_of_their_own(built):
    """RFX_EMIT_BY_ROWS=2 is read once per process: the first-row probe's table is then PACKED at every size -- here at 2^22 slots -- and the result is
    emitted by rows; with RFX_NO_PACKED_TABLE=1 the same tail reads the array-per-field table.  Every `probe_small` case of this file under each (the
    two processes run side by side: most of their time is the interpreter's start and the reference).  No counter and no field of the result says which
    layout a table had (want_packed may decline, ph_pass falls back to the fields when the packed insert does not carry a query): what these cases
    assert is the answer under each setting; that the first one reaches a packed table is known from want_packed's rule for these queries -- one
    key, one shard, no expression tree, the first-row probe -- and from these same cases failing when the null entry is addressed as `d_first + cap`."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "-k", "probe_small"]
    procs = [subprocess.Popen(cmd, env=dict(os.environ, **dict(kv.split("=") for kv in knob.split(","))), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=os.path.dirname(here)) for knob in KNOBS]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for knob, p, (out, err) in zip(KNOBS, procs, outs):
        assert p.returncode == 0 and "12 passed" in out, knob + "\n" + out[-2500:] + err[-1500:]  # (5 + 5 + 1 + 1 cases are named probe_small)


# ---------------------------------------------------------------- the operator door
def door_stat(ops, which):
    x = ops.rfx_ops_exec()
    return int(ops.rfx_exec_stat(C.c_void_p(x), which)) if x else 0


def ask(ops, q, tab):
    d = H.select_dict(q, tab)
    r = ops.rfx_select(d)
    assert r, "null result"
    if H.is_error(r):
        msg = H.error_text(r)
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(d)
        raise RuntimeError(msg)
    out = H.table_to_numpy(r)
    ops.rfx_host_drop(r)
    ops.rfx_host_drop(d)
    return out


@gpu
def test_rfx_group_over_sparse_keys_from_2_24_rows(ops, eng):
    """rfx_group sets REFUSE_NULL_KEY | PROBE_FIRST: over 4 000 000 sparse keys the table grows to 2^26 slots and is packed with W = 2 -- with the key
    homed at cap / 2 among them.  An IDS index, no error object, the oracle's group count and per-row ids (first-occurrence order)."""
    hk = dataset(eng, D_LARGE)["hk"]
    want, _, groups, dense = rfo.group_index(hk, None)
    assert not dense and groups == dataset(eng, D_LARGE)["all"]["groups"] and (hk == KEY_HOME_2_26).sum() == 3
    kv = H.vector(hk)
    with Route(lambda w: door_stat(ops, w)) as r:
        ix = ops.rfx_group(kv)
    try:
        assert ix and not H.is_error(ix), H.error_text(ix)
        assert r.sampled >= 1 and r.grown >= 1
        slots = H.list_items(ix)
        assert H.header(ix).len == 7
        assert C.c_int64.from_address(slots[0] + 8).value == 0 and C.c_int64.from_address(slots[1] + 8).value == groups  # INDEX_TYPE_IDS
        assert np.array_equal(H.to_numpy(slots[2]), want)
    finally:
        for o in (ix, kv):
            ops.rfx_host_drop(o)
        ops.rfx_cache_clear()


@gpu
def test_rfx_select_by_sparse_keys_from_2_24_rows(ops, eng):
    """rfx_select {s: (sum a) c: (count a) by: k} over the same keys equals the oracle's select; with the hidden null key the query is handed back
    ("null group key"), as the dense keys of test_sampled_scope_at_the_operator_boundary are."""
    hk = dataset(eng, D_LARGE)["hk"]
    host = {"k": hk, "a": _DATA["ha"]}
    q = {"s": ("sum", "a"), "c": ("count", "a"), "by": "k"}
    tab = H.table(host)
    try:
        with Route(lambda w: door_stat(ops, w)) as r:
            got = ask(ops, q, tab)
        assert r.sampled >= 1 and r.grown >= 1 and ops.rfx_last_select_on_gpu() == 1
        want = rfo.select({"from": host, **q})
        assert list(got) == list(want)
        for name in want:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    finally:
        ops.rfx_host_drop(tab)
        ops.rfx_cache_clear()
    hidden = hk.copy()
    hidden[SPOT] = NULL
    tab = H.table({"k": hidden, "a": _DATA["ha"]})
    try:
        with Route(lambda w: door_stat(ops, w)) as r:
            with pytest.raises(RuntimeError, match="null group key"):
                ask(ops, q, tab)
        assert r.sampled >= 1
    finally:
        ops.rfx_host_drop(tab)
        ops.rfx_cache_clear()
