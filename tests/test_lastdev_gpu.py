"""`last` and `dev` on the MI355X (rfx_lastdev.hip, rfx_exec_lastdev.c): every golden case of the compiled reference (tests/golden/lastdev_golden.npz) through
the Engine and through rfx_last / rfx_dev over the fixture's own MAPGROUP indexes; every grouped kernel family forced by its tune flag against the numpy
restatement (tests/lastdev_ref.py); several `last` aggregates in one query; shards of one device; the select door.  last is checked bit for bit, dev
within the bounds derived from a 1e-9 relative f64 sum (lastdev_ref.group_dev_close / dev_close)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lastdev_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H

pytestmark = pytest.mark.gpu
T_MAPFILTER, T_MAPGROUP = 71, 72
NULL = R.NULL_I64
Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lastdev_golden.npz"))

NO_LDS_TABLES, NO_PARTITION, CHUNK_SMALL, CHUNK_QUEUE, CHUNK_BINS, NO_RTC, NO_PLANE = 1, 2, 32768, 131072, 262144, 524288, 1048576


def dev(eng, host):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(eng.device) for k, v in host.items()}


def by_first_occurrence(keys: np.ndarray, sel: np.ndarray):
    """(group id per row or -1, the groups' keys in first-occurrence order of the selected rows) -- keys: one column or a tuple of columns"""
    cols = keys if isinstance(keys, tuple) else (keys,)
    rows = np.flatnonzero(sel)
    tup = np.stack([c[rows] for c in cols], 1)
    uk, first, inv = np.unique(tup, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uk), np.int64)
    rank[order] = np.arange(len(uk))
    g = np.full(len(cols[0]), -1, np.int64)
    g[rows] = rank[inv.reshape(-1)]
    return g, uk[order]


# ---------------------------------------------------------------------------------------------------- the goldens
def golden_selection(ci):
    _, vt, itype, groups, shift, filt = (int(x) for x in Z["group_cases"][ci])
    p = f"g{ci}_"
    keys, vals, ix = Z[p + "keys"], Z[p + "vals"], Z[p + "ix"]
    sel = np.zeros(len(keys), bool)
    sel[Z[p + "filter"] if filt else np.arange(len(keys))] = True
    rows = np.flatnonzero(sel)
    gid_of_row = np.full(len(keys), -1, np.int64)
    gid_of_row[rows] = ix if itype == 0 else ix[keys[rows] - shift]
    return p, keys, vals, sel, gid_of_row, groups


@pytest.mark.parametrize("ci", range(12))
def test_golden_grouped_cases_through_the_engine(eng, ci):
    p, keys, vals, sel, gid_of_row, groups = golden_selection(ci)
    d = dev(eng, {"k": keys, "v": vals, "m": sel.astype(np.int8)})
    where = d["m"] if not sel.all() else None
    r = eng.group_by("k", [("last", "v"), ("count", "v")], where, d)
    assert r["groups"] == groups
    # the engine's groups by key -> the index's group ids (the key of a group is the key of any of its rows)
    gid_of_key = dict(zip(keys[sel].tolist(), gid_of_row[sel].tolist()))
    pos = np.array([gid_of_key[k] for k in r["keys"].cpu().numpy().tolist()], np.int64)
    got = np.empty(groups, vals.dtype)
    got[pos] = r["results"][0].cpu().numpy()
    assert R.same_bits(got, Z[p + "last"]), ci
    gd = eng.group_dev("k", "v", where, d)
    assert gd["groups"] == groups and np.array_equal(gd["keys"].cpu().numpy(), r["keys"].cpu().numpy())
    gotd = np.empty(groups)
    gotd[pos] = gd["dev"].cpu().numpy()
    v, g = vals[sel], gid_of_row[sel]
    print("dev got", gotd[:6], "want", Z[p + "dev"][:6])
    assert R.group_dev_close(gotd, Z[p + "dev"], v, g, groups) is None, (ci, R.group_dev_close(gotd, Z[p + "dev"], v, g, groups))


def test_golden_scalar_cases_through_the_engine(eng):
    for si in range(int(Z["scalar_cases"])):
        v = Z[f"s{si}_vals"]
        if len(v) == 0:
            continue  # (an Engine column has at least one row; the empty vector goes through rfx_last / rfx_dev below)
        d = dev(eng, {"v": v})
        got = eng.last("v", None, d)
        want = Z[f"s{si}_last"][0]
        if v.dtype == np.float64:
            assert R.same_bits(np.float64(got), want), (si, got, want)
        else:
            assert (NULL if got is None else got) == int(want), (si, got, want)
        gd = eng.dev("v", None, d)
        print("scalar dev", si, gd, float(Z[f"s{si}_dev"][0]))
        assert R.dev_close(gd, float(Z[f"s{si}_dev"][0]), v), (si, gd, Z[f"s{si}_dev"][0])


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    o.rfx_host_bind()
    return o


def mapgroup_pair(vals, vt, itype, groups, ix, shift, keys, filt):
    index = H.lib().rfx_host_list(7)
    arr = (C.c_void_p * 7).from_address(H.payload(index))
    arr[0], arr[1] = H.atom(itype), H.atom(groups)
    arr[2] = H.vector(ix)
    arr[3] = H.atom(shift)
    if itype == 1:
        arr[4] = H.vector(keys)
    if filt is not None:
        arr[5] = H.vector(filt)
    v = H.vector(vals)
    H.header(v).type = vt  # (TIMESTAMP values keep their type)
    pair = H.list_of([v, index])
    H.header(pair).type = T_MAPGROUP
    return pair


def test_golden_cases_through_rfx_last_and_rfx_dev(ops):
    """aggr_last / aggr_dev / ray_last / ray_dev's own answers through rfx_last / rfx_dev over the same MAPGROUP indexes and vectors"""
    for ci in range(len(Z["group_cases"])):
        _, vt, itype, groups, shift, filt = (int(x) for x in Z["group_cases"][ci])
        p, keys, vals, sel, gid_of_row, _ = golden_selection(ci)
        pair = mapgroup_pair(vals, vt, itype, groups, Z[p + "ix"], shift, keys, Z[p + "filter"] if filt else None)
        r = ops.rfx_last(pair)
        assert not H.is_error(r), H.error_text(r)
        assert H.header(r).type in (L.RFX_I64, L.RFX_F64) and R.same_bits(H.to_numpy(r), Z[p + "last"]), ci
        ops.rfx_host_drop(r)
        r = ops.rfx_dev(pair)
        assert not H.is_error(r), H.error_text(r)
        got = H.to_numpy(r)
        assert R.group_dev_close(got, Z[p + "dev"], vals[sel], gid_of_row[sel], groups) is None, ci
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(pair)
    for si in range(int(Z["scalar_cases"])):
        v = Z[f"s{si}_vals"]
        r = ops.rfx_last(H.vector(v))
        assert not H.is_error(r), H.error_text(r)
        assert bytes((C.c_char * 8).from_address(r + 8)) == Z[f"s{si}_last"].tobytes() or (v.dtype == np.float64 and np.isnan(Z[f"s{si}_last"][0]) and
                                                                                       np.isnan(C.c_double.from_address(r + 8).value)), si
        ops.rfx_host_drop(r)
        r = ops.rfx_dev(H.vector(v))
        assert not H.is_error(r), H.error_text(r)
        assert H.header(r).type == -L.RFX_F64
        assert R.dev_close(C.c_double.from_address(r + 8).value, float(Z[f"s{si}_dev"][0]), v), si
        ops.rfx_host_drop(r)


def test_mapfilter_pairs(ops):
    rng = np.random.default_rng(12)
    v = rng.standard_normal(5000)
    v[rng.random(5000) < 0.3] = np.nan
    ids = np.sort(rng.choice(5000, 1700, replace=False)).astype(np.int64)
    v[ids[-1]] = np.nan  # the last collected cell is null: last is positional
    for fn, want in ((ops.rfx_last, None), (ops.rfx_dev, R.dev(v[ids]))):
        pair = H.list_of([H.vector(v), H.vector(ids)])
        H.header(pair).type = T_MAPFILTER
        r = fn(pair)
        assert not H.is_error(r), H.error_text(r)
        got = C.c_double.from_address(r + 8).value
        assert np.isnan(got) if want is None else R.dev_close(got, want, v[ids])
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(pair)


# ---------------------------------------------------------------------------------------------------- every grouped kernel family
def family_table(n, nkeys, seed):
    """30 % nulls in `v` (other rows in `w`); per group the nulls are PLACED: in a fifth of the groups the last selected row is null, and the
    highest unselected row lies above the answer in more than a tenth"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, nkeys, n)
    a = rng.integers(0, 100, n)
    v = rng.integers(-(2**40), 2**40, n)
    v[rng.random(n) < 0.3] = NULL
    w = rng.standard_normal(n) * 100
    w[rng.random(n) < 0.3] = np.nan
    # the last row of every fifth key: null in both columns
    lastrow = np.full(nkeys, -1, np.int64)
    lastrow[k] = np.arange(n)
    hit = lastrow[(np.arange(nkeys) % 5 == 0) & (lastrow >= 0)]
    v[hit] = NULL
    w[hit] = np.nan
    # ... and of every key = 1 mod 3: unselected by `a < 70`, with a value
    out = lastrow[(np.arange(nkeys) % 3 == 1) & (lastrow >= 0)]
    a[out] = 99
    v[out] = 123456789
    w[out] = 1.25
    return {"k": k, "a": a, "v": v, "w": w, "k2": rng.integers(0, 7, n), "ks": k * 1_000_003 - 77_777}


def shares(host, key, sel):
    """(share of groups whose last selected row is null in v, share of groups whose highest unselected row lies above v's answer)"""
    g, _ = by_first_occurrence(host[key], sel)
    groups = int(g.max()) + 1
    lastsel = np.full(groups, -1, np.int64)
    rows = np.flatnonzero(sel)
    lastsel[g[rows]] = rows
    ans = R.group_last_rows(host["v"], g, groups)
    gall, _ = by_first_occurrence(host[key], np.ones(len(sel), bool))
    # (groups of the selection, numbered as in `g`, for the unselected rows: through the key)
    first_of = {kk: gg for kk, gg in zip(host[key][rows].tolist(), g[rows].tolist())}
    hi_unsel = np.full(groups, -1, np.int64)
    for r_ in np.flatnonzero(~sel):
        gg = first_of.get(int(host[key][r_]))
        if gg is not None:
            hi_unsel[gg] = r_
    return float(np.mean(R.is_null(host["v"][lastsel]))), float(np.mean(hi_unsel > ans))


def check_last(eng, host, d, key, where, sel, aggs=(("last", "v"), ("last", "w"))):
    keys = tuple(host[c] for c in key) if isinstance(key, list) else host[key]
    g, gkeys = by_first_occurrence(keys, sel)
    groups = len(gkeys)
    r = eng.group_by(key, list(aggs), where, d)
    assert r["groups"] == groups
    if isinstance(key, list):
        assert np.array_equal(np.stack([c.cpu().numpy() for c in r["key_columns"]], 1), gkeys)
    else:
        assert np.array_equal(r["keys"].cpu().numpy(), gkeys[:, 0])
    for (fn, col), res in zip(aggs, r["results"]):
        assert fn == "last"
        assert R.same_bits(res.cpu().numpy(), R.group_last(host[col], g, groups)), (key, col)
    return r


FAMILIES = [("lds tables", 0, 1000), ("lds tables, no run-time compiler", NO_RTC, 1000), ("device atomics", NO_LDS_TABLES | NO_PARTITION, 1000),
            ("partitioned", NO_LDS_TABLES, 50_000), ("device atomics, many keys", NO_PARTITION, 50_000), ("planes", CHUNK_SMALL, 50_000),
            ("chunks", CHUNK_SMALL | NO_PLANE, 50_000), ("chunks, sorted queue", CHUNK_SMALL | NO_PLANE | CHUNK_QUEUE, 50_000),
            ("chunks, bins", CHUNK_SMALL | NO_PLANE | CHUNK_BINS, 50_000)]


@pytest.mark.parametrize("name,flags,nkeys", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_last_through_every_grouped_kernel_family(eng, name, flags, nkeys):
    n = 1 << 17
    host = family_table(n, nkeys, 7 + nkeys)
    sel = host["a"] < 70
    null_last, unsel_above = shares(host, "k", sel)
    assert null_last >= 0.10 and unsel_above >= 0.10, (null_last, unsel_above)
    d = dev(eng, host)
    try:
        eng.tune(flags=flags)
        before = [eng.stat(i) for i in range(5)]
        # (the chunk kernels carry ONE value column, the planes several: tests/test_gpu_parity.py)
        for aggs in ([(("last", "v"),), (("last", "w"),)] if name.startswith("chunks") else [(("last", "v"), ("last", "w"))]):
            for where, s_ in ((None, np.ones(n, bool)), (("<", "a", 70), sel)):
                r = check_last(eng, host, d, "k", where, s_, aggs)
                # (no counter tells LDS tables, device atomics and the partitioned kernels apart: what can be said is that the dense tables answered)
                assert r["path"] in (L.RFX_PATH_DENSE, L.RFX_PATH_DENSE_SMALL), (name, r["path"])
        after = [eng.stat(i) for i in range(5)]
        if name == "planes":
            assert after[0] > before[0] and after[2] > before[2], (before, after)
        if name.startswith("chunks"):
            assert after[0] == before[0] and after[3] > before[3] and after[4] > before[4], (before, after)
        if not (flags & CHUNK_SMALL):
            assert after[0] == before[0] and after[3] == before[3], (before, after)
        # sparse keys (the hashed tables), a two-column by: (composite key) and, with a key column beyond 2^62 apart, a row-hash tuple
        r = check_last(eng, host, d, "ks", ("<", "a", 70), sel)
        assert r["path"] == L.RFX_PATH_HASH
        check_last(eng, host, d, ["k2", "k"], None, np.ones(n, bool))
        check_last(eng, host, d, ["k2", "k"], ("<", "a", 70), sel)
    finally:
        eng.tune(flags=0)


def test_last_over_a_row_hash_tuple(eng):
    n = 1 << 17
    host = family_table(n, 1000, 99)
    host["kw"] = np.where(host["k"] % 2 == 0, host["k"] * (2**52), -host["k"] * (2**52))  # two wide ranges: no composite key fits 64 bits
    host["kx"] = host["k2"] * (2**60) - 2**62
    d = dev(eng, host)
    r = check_last(eng, host, d, ["kw", "kx"], None, np.ones(n, bool))
    assert r["path"] == L.RFX_PATH_ROWHASH
    check_last(eng, host, d, ["kw", "kx"], ("<", "a", 70), host["a"] < 70)


def test_dev_through_the_grouped_kernel_families(eng):
    n = 1 << 17
    for flags, nkeys, key in ((0, 1000, "k"), (NO_LDS_TABLES | NO_PARTITION, 1000, "k"), (CHUNK_SMALL, 50_000, "k"), (CHUNK_SMALL | NO_PLANE, 50_000, "k"),
                              (0, 50_000, "ks")):
        host = family_table(n, nkeys, 31 + nkeys)
        d = dev(eng, host)
        try:
            eng.tune(flags=flags)
            for where, sel in ((None, np.ones(n, bool)), (("<", "a", 70), host["a"] < 70)):
                g, gkeys = by_first_occurrence(host[key], sel)
                for col in ("v", "w"):
                    r = eng.group_dev(key, col, where, d)
                    assert r["groups"] == len(gkeys) and np.array_equal(r["keys"].cpu().numpy(), gkeys[:, 0])
                    got, want = r["dev"].cpu().numpy(), R.group_dev(host[col], g, len(gkeys))
                    assert R.group_dev_close(got, want, host[col], g, len(gkeys)) is None, (flags, key, col)
        finally:
            eng.tune(flags=0)


# ---------------------------------------------------------------------------------------------------- kernels compiled at run time
def _rtc_stats(eng):
    a, b = C.c_int64(), C.c_int64()
    eng.lib.rfx_hip_rtc_stats(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def test_scalar_last_beside_the_run_time_compiled_fold(eng):
    """scalar `last` is answered beside the fused fold (rfx_scalar.hip: the last id of the ordered compaction, k_last_fill), the other aggregates of the
    same call by the fold -- by its per-plan kernel compiled at first sight under RFX_RTC_EAGER=1 (the launch counter moves for the plans that have a
    fold) or by the prebuilt kernels (RFX_TUNE_NO_RTC): I64 and F64, with and without where:, selections ending in a null cell, bit for bit either way"""
    rng = np.random.default_rng(77)
    n = 300_007
    host = {"v": rng.integers(-1000, 1000, n), "f": rng.standard_normal(n), "a": rng.integers(0, 100, n), "b": rng.integers(0, 100, n)}
    host["v"][-1], host["f"][-1], host["a"][-1], host["b"][-1] = NULL, np.nan, 5, 90  # the table, and the selection a < 30, end in a null cell
    d = dev(eng, host)
    plans = [([("last", "v")], None), ([("last", "f")], None), ([("last", "v"), ("last", "f"), ("first", "v")], ("<", "a", 30)),
             ([("last", "f"), ("sum", "a"), ("last", "v"), ("last", "a"), ("max", "f")], ("and", (">", "b", 50), ("<", "b", 80))),
             ([("last", "v"), ("last", "f")], (">", "a", 1000))]
    l0, c0 = _rtc_stats(eng)
    os.environ["RFX_RTC_EAGER"] = "1"
    try:
        fast = [eng.filter_aggr(aggs, where, d) for aggs, where in plans]
    finally:
        del os.environ["RFX_RTC_EAGER"]
    l1, c1 = _rtc_stats(eng)
    if l1 == l0:
        pytest.skip("no run-time compiler on this box (libhiprtc.so / kernel sources): the prebuilt kernels answered")
    assert l1 - l0 >= 2  # (the two plans with other aggregates and predicates beside their lasts)
    try:
        eng.tune(flags=NO_RTC)
        slow = [eng.filter_aggr(aggs, where, d) for aggs, where in plans]
        assert _rtc_stats(eng)[0] == l1  # the flag kept every launch on the prebuilt kernels
    finally:
        eng.tune(flags=0)
    same = lambda x, y: (x is None and y is None) or (isinstance(x, float) and np.float64(x).tobytes() == np.float64(y).tobytes()) or (not isinstance(x, float) and x == y)
    for (aggs, where), (fv, fs), (sv, ss) in zip(plans, fast, slow):
        assert fs == ss and all(same(x, y) or (isinstance(x, float) and np.isnan(x) and np.isnan(y)) for x, y in zip(fv, sv)), (aggs, where, fv, sv)
    assert fast[0][0] == [None] and np.isnan(fast[1][0][0])
    rows = np.flatnonzero(host["a"] < 30)
    assert rows[-1] == n - 1 and fast[2][0][0] is None and np.isnan(fast[2][0][1]) and fast[2][0][2] == int(host["v"][rows[0]])
    rows = np.flatnonzero((host["b"] > 50) & (host["b"] < 80))
    assert fast[3][0][0] == host["f"][rows[-1]] and fast[3][0][2] == int(host["v"][rows[-1]]) and fast[3][0][3] == int(host["a"][rows[-1]]) and fast[3][1] == len(rows)
    assert fast[4][0][0] is None and np.isnan(fast[4][0][1]) and fast[4][1] == 0


@pytest.mark.parametrize("groups", [1, 6, 8])
def test_grouped_last_over_at_most_8_slots_through_the_run_time_compiled_kernel(eng, groups):
    """group-bys over at most 8 slots take a kernel generated for the plan (rfx_group_few_rtc.hpp): `last` rides through it as the MAX over derived rows"""
    n = 200_003
    host = family_table(n, groups, 60 + groups)
    host["k"] = host["k"] + 1000
    sel = host["a"] < 70
    d = dev(eng, host)
    l0, c0 = _rtc_stats(eng)
    os.environ["RFX_RTC_EAGER"] = "1"
    try:
        fast = [check_last(eng, host, d, "k", where, s_) for where, s_ in ((None, np.ones(n, bool)), (("<", "a", 70), sel))]
    finally:
        del os.environ["RFX_RTC_EAGER"]
    l1, c1 = _rtc_stats(eng)
    if l1 == l0:
        pytest.skip("no run-time compiler on this box (libhiprtc.so / kernel sources): the prebuilt kernels answered")
    assert l1 - l0 >= 2
    try:
        eng.tune(flags=NO_RTC)
        slow = [check_last(eng, host, d, "k", where, s_) for where, s_ in ((None, np.ones(n, bool)), (("<", "a", 70), sel))]
        assert _rtc_stats(eng)[0] == l1
    finally:
        eng.tune(flags=0)
    for f, s_ in zip(fast, slow):
        for x, y in zip(f["results"], s_["results"]):
            assert np.array_equal(x.cpu().numpy().view(np.int64), y.cpu().numpy().view(np.int64))


# ---------------------------------------------------------------------------------------------------- indexes built here (rfx_group)
@pytest.mark.parametrize("sparse", [False, True])
def test_rfx_last_and_rfx_dev_over_an_index_built_by_rfx_group(ops, sparse):
    """fold_mapgroup's LAST path and rfx_dev answer in the order of the index's own group ids: pinned over indexes rfx_group builds (SHIFT over dense
    keys, IDS over sparse ones), cell by cell against the ids the index itself holds"""
    rng = np.random.default_rng(14 + sparse)
    n, nkeys = 50_000, 700
    keys = rng.integers(0, nkeys, n) + 100
    if sparse:
        keys = keys * 1_000_003_000 - 77
    for vals in (np.where(rng.random(n) < 0.3, NULL, rng.integers(-(2**40), 2**40, n)), np.where(rng.random(n) < 0.3, np.nan, rng.standard_normal(n) * 10 + 1000)):
        kv = H.vector(keys)
        ix = ops.rfx_group(kv)
        assert not H.is_error(ix), H.error_text(ix)
        slots = H.list_items(ix)
        itype, groups = C.c_int64.from_address(slots[0] + 8).value, C.c_int64.from_address(slots[1] + 8).value
        assert itype == (0 if sparse else 1)
        table = H.to_numpy(slots[2])
        gids = table if itype == 0 else table[keys - C.c_int64.from_address(slots[3] + 8).value]
        assert groups == len(np.unique(keys)) and gids.min() == 0 and gids.max() == groups - 1
        pair = H.list_of([H.vector(vals), ix])
        H.header(pair).type = T_MAPGROUP
        r = ops.rfx_last(pair)
        assert not H.is_error(r), H.error_text(r)
        assert R.same_bits(H.to_numpy(r), R.group_last(vals, gids, groups))
        ops.rfx_host_drop(r)
        r = ops.rfx_dev(pair)
        assert not H.is_error(r), H.error_text(r)
        assert R.group_dev_close(H.to_numpy(r), R.group_dev(vals, gids, groups), vals, gids, groups) is None
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(pair)
        ops.rfx_host_drop(kv)


# ---------------------------------------------------------------------------------------------------- several aggregates
def test_two_lasts_beside_first_min_max_sum(eng):
    n = 100_003
    host = family_table(n, 3000, 5)
    d = dev(eng, host)
    sel = host["a"] < 70
    g, gkeys = by_first_occurrence(host["k"], sel)
    groups = len(gkeys)
    aggs = [("last", "v"), ("first", "v"), ("min", "v"), ("last", "w"), ("max", "v"), ("sum", "a")]
    r = eng.group_by("k", aggs, ("<", "a", 70), d)
    res = [x.cpu().numpy() for x in r["results"]]
    assert R.same_bits(res[0], R.group_last(host["v"], g, groups)) and R.same_bits(res[3], R.group_last(host["w"], g, groups))
    assert not np.array_equal(R.group_last_rows(host["v"], g, groups), R.group_last_rows(host["w"], g, groups))  # the two columns' nulls differ
    rows = np.flatnonzero(sel)
    first = np.full(groups, -1, np.int64)
    first[g[rows][::-1]] = rows[::-1]
    assert np.array_equal(res[1], host["v"][first])
    ok = sel & (host["v"] != NULL)
    mn, mx = np.full(groups, np.iinfo(np.int64).max), np.full(groups, np.iinfo(np.int64).min)
    np.minimum.at(mn, g[ok], host["v"][ok])
    np.maximum.at(mx, g[ok], host["v"][ok])
    has = np.bincount(g[ok], minlength=groups) > 0
    assert np.array_equal(res[2][has], mn[has]) and np.array_equal(res[4][has], mx[has])
    assert np.array_equal(res[5], np.bincount(g[rows], weights=None, minlength=groups) * 0 + np.array([host["a"][rows][g[rows] == i].sum() for i in range(groups)]))


def test_eight_aggregates_of_which_four_are_last(eng):
    n = 70_001
    rng = np.random.default_rng(3)
    host = family_table(n, 500, 8)
    for c in ("x", "y"):
        host[c] = rng.integers(0, 10**9, n)
        host[c][rng.random(n) < 0.4] = NULL
    d = dev(eng, host)
    g, gkeys = by_first_occurrence(host["k"], np.ones(n, bool))
    groups = len(gkeys)
    aggs = [("last", "v"), ("count", "a"), ("last", "w"), ("max", "x"), ("last", "x"), ("min", "y"), ("last", "y"), ("sum", "a")]
    r = eng.group_by("k", aggs, None, d)
    for i, col in ((0, "v"), (2, "w"), (4, "x"), (6, "y")):
        assert R.same_bits(r["results"][i].cpu().numpy(), R.group_last(host[col], g, groups)), col
    assert np.array_equal(r["results"][1].cpu().numpy(), np.bincount(g, minlength=groups))


# ---------------------------------------------------------------------------------------------------- shards of one device
@pytest.mark.parametrize("shards", [2, 3, 4, 5])
def test_shards_of_one_device(shards):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rayforce_amd.engine import Engine
    e = Engine(0, shards=shards)
    try:
        n = 60_000
        host = family_table(n, 800, 40 + shards)
        # half of the rows: keys that live in one stretch of the table, so that groups end in every shard
        local = np.random.default_rng(shards).random(n) < 0.5
        host["k"] = np.where(local, 800 + (np.arange(n) * 400) // n, host["k"])
        host["ks"] = host["k"] * 1_000_003 - 77_777
        d = dev(e, host)
        for where, sel in ((None, np.ones(n, bool)), (("<", "a", 70), host["a"] < 70)):
            g, gkeys = by_first_occurrence(host["k"], sel)
            check_last(e, host, d, "k", where, sel)
            # answers whose last row lies in each shard are present
            ans = R.group_last_rows(host["v"], g, len(gkeys))
            r0, ln = C.c_int64(), C.c_int64()
            for s in range(shards):
                e.lib.rfx_exec_split(n, shards, s, C.byref(r0), C.byref(ln))
                assert ((ans >= r0.value) & (ans < r0.value + ln.value)).any(), s
            # scalar: the last selected row, null or not
            rows = np.flatnonzero(sel)
            for col in ("v", "w"):
                got = e.last(col, where, d)
                want = host[col][rows[-1]]
                if col == "v":
                    assert (NULL if got is None else got) == int(want), (col, got, want)
                else:
                    assert R.same_bits(np.float64(got), want), (col, got, want)
        check_last(e, host, d, "ks", None, np.ones(n, bool))
    finally:
        e.close()


DOOR_SHARDS_CODE = """
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import lastdev_ref as R
from rayforce_amd import hostobj as H
shards = int(os.environ["RFX_SHARDS"])
o = H.lib(); o.rfx_host_bind()
rng = np.random.default_rng(2); n = 50_000
host = {"s": rng.integers(0, 300, n), "p": rng.integers(1, 10**6, n), "a": rng.integers(0, 100, n)}
# half of the rows: symbols that live in one stretch of the table, so that groups end in every shard
host["s"] = np.where(rng.random(n) < 0.5, 300 + (np.arange(n) * 200) // n, host["s"])
host["p"][rng.random(n) < 0.3] = R.NULL_I64
host["p"][-1] = R.NULL_I64; host["a"][-1] = 5
tab = H.table(host)
def ask(q):
    d = H.select_dict(q, tab); r = o.rfx_select(d)
    assert not H.is_error(r), H.error_text(r)
    assert o.rfx_last_select_on_gpu() == 1, o.rfx_ops_last_error()
    return H.table_to_numpy(r)
for where, sel in ((None, np.ones(n, bool)), (("<", "a", 60), host["a"] < 60)):
    q = {"by": "s", "c": ("last", "p")}
    if where: q = {"where": where, **q}
    got = ask(q)
    rows = np.flatnonzero(sel); uk, first, inv = np.unique(host["s"][rows], return_index=True, return_inverse=True)
    order = np.argsort(first); rank = np.empty(len(uk), np.int64); rank[order] = np.arange(len(uk))
    g = np.full(n, -1, np.int64); g[rows] = rank[inv]
    assert np.array_equal(got["s"], uk[order]) and np.array_equal(got["c"], R.group_last(host["p"], g, len(uk)))
    ans = R.group_last_rows(host["p"], g, len(uk))
    r0, ln = C.c_int64(), C.c_int64()
    for sh in range(shards):  # answers whose last row lies in each shard are present
        o.rfx_exec_split(C.c_int64(n), C.c_int(shards), C.c_int(sh), C.byref(r0), C.byref(ln))
        assert ((ans >= r0.value) & (ans < r0.value + ln.value)).any(), sh
    # scalar, through rfx_select: the last selected row, null or not
    q = {"c": ("last", "p"), "ca": ("last", "a")}
    if where: q = {"where": where, **q}
    got = ask(q)
    assert int(got["c"][0]) == int(host["p"][rows[-1]]) == R.NULL_I64 and int(got["ca"][0]) == int(host["a"][rows[-1]])
# scalar, through rfx_last: the vector, and a MAPFILTER pair (a where: as row ids)
r = o.rfx_last(H.vector(host["p"])); assert not H.is_error(r), H.error_text(r)
assert C.c_int64.from_address(r + 8).value == int(host["p"][-1])
ids = np.flatnonzero(host["a"] > 60).astype(np.int64)
pair = H.list_of([H.vector(host["p"]), H.vector(ids)]); H.header(pair).type = 71
r = o.rfx_last(pair); assert not H.is_error(r), H.error_text(r)
assert C.c_int64.from_address(r + 8).value == int(host["p"][ids[-1]])
# grouped, through rfx_last over a MAPGROUP pair (an IDS index: every row's group id, groups numbered by first occurrence): fold_mapgroup's sharded branch
uk, first, inv = np.unique(host["s"], return_index=True, return_inverse=True)
order = np.argsort(first); rank = np.empty(len(uk), np.int64); rank[order] = np.arange(len(uk)); gids = rank[inv]
ix = o.rfx_host_list(7)
arr = (C.c_void_p * 7).from_address(H.payload(ix))
arr[0], arr[1], arr[2], arr[3] = H.atom(0), H.atom(len(uk)), H.vector(gids), H.atom(R.NULL_I64)
pair = H.list_of([H.vector(host["p"]), ix]); H.header(pair).type = 72
r = o.rfx_last(pair); assert not H.is_error(r), H.error_text(r)
assert np.array_equal(H.to_numpy(r), R.group_last(host["p"], gids, len(uk)))
assert o.rfx_ops_shards() == shards
print("ok")
"""


@pytest.mark.parametrize("shards", [2, 3, 4, 5])
def test_shards_through_the_door(shards):
    """RFX_SHARDS=k in a fresh process (the operator layer reads it once): grouped and scalar `last` through rfx_select and rfx_last over k shards of
    one device, with and without where:; groups whose answer lies in every shard"""
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    code = DOOR_SHARDS_CODE % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RFX_SHARDS=str(shards))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------- scalar
def test_scalar_last(eng):
    rng = np.random.default_rng(21)
    n = 300_007  # (several workgroups and a ragged tail)
    host = {"v": rng.integers(-1000, 1000, n), "f": rng.standard_normal(n), "a": rng.integers(0, 100, n)}
    host["v"][-1] = NULL
    host["f"][-1] = np.nan
    host["a"][-1] = 5
    host["a"][-2] = 80
    d = dev(eng, host)
    assert eng.last("v", None, d) is None and np.isnan(eng.last("f", None, d))  # a selection ending in a null cell: positional
    assert eng.last("v", ("<", "a", 50), d) is None
    assert eng.last("v", (">", "a", 50), d) == int(host["v"][-2]) and eng.last("f", (">", "a", 50), d) == host["f"][-2]
    assert eng.last("v", (">", "a", 1000), d) is None and np.isnan(eng.last("f", (">", "a", 1000), d))  # an empty selection: the typed null
    vals, nsel = eng.filter_aggr([("last", "v"), ("first", "v"), ("last", "f"), ("sum", "a"), ("last", "a")], ("<", "a", 30), d)
    rows = np.flatnonzero(host["a"] < 30)
    assert rows[-1] == n - 1 and nsel == len(rows) and vals[0] is None and vals[1] == int(host["v"][rows[0]]) and np.isnan(vals[2])  # (the last selected row is the null row)
    assert vals[3] == int(host["a"][rows].sum()) and vals[4] == int(host["a"][rows[-1]])
    one = dev(eng, {"v": np.array([7], np.int64), "f": np.array([2.5])})
    assert eng.last("v", None, one) == 7 and eng.last("f", None, one) == 2.5 and eng.dev("v", None, one) == 0.0


def test_scalar_dev(eng):
    rng = np.random.default_rng(22)
    n = 400_003
    host = {"v": rng.integers(-(2**50), 2**50, n), "f": rng.standard_normal(n) * 50 + 1e6, "a": rng.integers(0, 100, n)}
    host["v"][rng.random(n) < 0.1] = NULL
    host["f"][rng.random(n) < 0.1] = np.nan
    d = dev(eng, host)
    for col in ("v", "f"):
        for where, sel in ((None, np.ones(n, bool)), (("<", "a", 40), host["a"] < 40), ((">", "a", 1000), np.zeros(n, bool))):
            got, want = eng.dev(col, where, d), R.dev(host[col][sel])
            assert R.dev_close(got, want, host[col][sel]), (col, where, got, want)
    big = dev(eng, {"v": np.full(9, 2**62, np.int64)})  # the integer sum wraps: ray_dev's favg comes from the wrapped sum
    assert R.dev_close(eng.dev("v", None, big), R.dev(np.full(9, 2**62, np.int64)), np.full(9, 2**62, np.int64))
    assert R.dev(np.full(9, 2**62, np.int64)) > 0


# ---------------------------------------------------------------------------------------------------- the select door
def ask(ops, q, tab):
    d = H.select_dict(q, tab)
    r = ops.rfx_select(d)
    ops.rfx_host_drop(d)
    on_gpu = ops.rfx_last_select_on_gpu()
    if H.is_error(r):
        ops.rfx_host_drop(r)
        return None, on_gpu
    out = H.table_to_numpy(r)
    ops.rfx_host_drop(r)
    return out, on_gpu


def trades(n=200_000, seed=4):
    rng = np.random.default_rng(seed)
    host = {"s": rng.integers(0, 500, n), "ts": np.sort(rng.integers(0, 10**6, n)), "p": rng.integers(1, 10**6, n), "f": rng.standard_normal(n) + 100.0,
            "a": rng.integers(0, 100, n)}
    host["p"][rng.random(n) < 0.3] = NULL
    return host


def test_the_ohlc_select_is_answered_by_the_device(ops):
    """select {o: (first p) h: (max p) l: (min p) c: (last p) from: trades by: {s: s b: (xbar ts w)}} -- handed to the host before `last` was a device fold"""
    host = trades()
    tab = H.table(host)
    got, on_gpu = ask(ops, {"by": {"s": "s", "b": ("xbar", "ts", 50_000)}, "o": ("first", "p"), "h": ("max", "p"), "l": ("min", "p"), "c": ("last", "p")}, tab)
    assert on_gpu == 1, ops.rfx_ops_last_error()
    b = (host["ts"] // 50_000) * 50_000
    g, gkeys = by_first_occurrence((host["s"], b), np.ones(len(b), bool))
    groups = len(gkeys)
    assert np.array_equal(got["s"], gkeys[:, 0]) and np.array_equal(got["b"], gkeys[:, 1])
    assert np.array_equal(got["c"], R.group_last(host["p"], g, groups))
    first = np.full(groups, -1, np.int64)
    first[g[::-1]] = np.arange(len(g))[::-1]
    assert np.array_equal(got["o"], host["p"][first])
    # one key column, with and without where:, and the scalar forms
    for q, sel in (({"by": "s", "c": ("last", "p"), "cf": ("last", "f")}, np.ones(len(b), bool)),
                   ({"where": ("<", "a", 60), "by": "s", "c": ("last", "p"), "cf": ("last", "f")}, host["a"] < 60)):
        got, on_gpu = ask(ops, q, tab)
        assert on_gpu == 1, ops.rfx_ops_last_error()
        g, gkeys = by_first_occurrence(host["s"], sel)
        assert np.array_equal(got["s"], gkeys[:, 0])
        assert np.array_equal(got["c"], R.group_last(host["p"], g, len(gkeys))) and R.same_bits(got["cf"], R.group_last(host["f"], g, len(gkeys)))
    got, on_gpu = ask(ops, {"c": ("last", "p"), "cf": ("last", "f")}, tab)
    assert on_gpu == 1 and int(got["c"][0]) == int(host["p"][-1]) and got["cf"][0] == host["f"][-1]
    rows = np.flatnonzero(host["a"] < 60)
    got, on_gpu = ask(ops, {"where": ("<", "a", 60), "c": ("last", "p")}, tab)
    assert on_gpu == 1 and int(got["c"][0]) == int(host["p"][rows[-1]])
    ops.rfx_host_drop(tab)


def test_scalar_dev_through_the_door(ops):
    host = trades(50_000)
    tab = H.table(host)
    got, on_gpu = ask(ops, {"d": ("dev", "p"), "df": ("dev", "f"), "t": ("sum", "a")}, tab)
    ops.rfx_host_drop(tab)
    assert on_gpu == 1, ops.rfx_ops_last_error()
    assert R.dev_close(float(got["d"][0]), R.dev(host["p"]), host["p"]) and R.dev_close(float(got["df"][0]), R.dev(host["f"]), host["f"])
    assert int(got["t"][0]) == int(host["a"].sum())


@pytest.mark.parametrize("q,why", [({"by": "s", "d": ("dev", "p")}, "dev under by:"),                  # ray_dev of a MAPGROUP pair: null there
                                   ({"where": ("<", "a", 50), "d": ("dev", "p")}, "dev under where:"),  # ... of a MAPFILTER pair: null there
                                   ({"d": ("dev", ("+", "p", "a"))}, "dev of an expression"),
                                   ({"by": "s", "c": ("last", ("+", "p", "a"))}, "last of an expression")])
def test_shapes_handed_back_with_their_reason(ops, q, why):
    host = trades(10_000)
    tab = H.table(host)
    _, on_gpu = ask(ops, q, tab)
    ops.rfx_host_drop(tab)
    assert on_gpu == 0
    assert why in ops.rfx_ops_last_error().decode()  # (standalone: no host ray_select behind the door, so an error object naming the reason)


def test_window_join_still_refuses_dev(eng):
    """(the door's own wording for it is pinned by tests/test_wj_gpu.py; `dev` now has a function object, and window_agg still does not list it)"""
    from rayforce_amd._lib import RfxError
    c = torch.arange(100, device=eng.device)
    t = {"k": c, "t": c, "v": c}
    with pytest.raises(RfxError, match="is not one of"):
        eng.window_join(["k", "t"], (c, c), t, t, {"a": ("dev", "v")})
