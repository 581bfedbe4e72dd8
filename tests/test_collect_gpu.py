"""`row` and the collected column of select ... by: on the GPU by equality of bits: every case of the compiled reference's fixture
(tests/golden/collect_golden.npz) through rfx_select over standalone host objects -- the razed cells, the groups' lengths, the items' type codes and
attribute byte 0, the key and aggregate columns, i.e. the group order too -- and through rfx_row / rfx_collect over MAPGROUP pairs: the index rfx_group
builds for the case's key column, and, for the filtered cases, the reference-shaped IDS and SHIFT indexes with filter ids.  Then the shapes handed to the
host with their reasons, the malformed indexes refused as errors BEFORE any kernel uses them, and a sharded door."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import collect_ref as R
from rayforce_amd import hostobj as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "collect_golden.npz")
CASES = R.cases()
NULL = R.NULL_I64


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    l = H.lib()
    assert l.rfx_host_bind() == 0
    yield l
    l.rfx_cache_clear()


@pytest.fixture(scope="module")
def gold():
    return json.loads(bytes(np.load(GOLD)["json"]).decode())


def host_table(t, symbol=()):
    names = list(t)
    cols = [H.typed_vector(t[n], "symbol" if n in symbol else (n[2:] if n.startswith("v_") else "i64")) for n in names]
    return H.lib().rfx_host_table(H.symbols(names), H.list_of(cols))


def read_table(o):
    keys, vals = H.list_items(o)
    names = [H.lib().rfx_host_symbol_name(int(i)).decode() for i in H.to_numpy(keys)]
    return {n: (H.list_to_numpy(c) if H.header(c).type == H.T_LIST else H.to_numpy(c)) for n, c in zip(names, H.list_items(vals))}


def check_list(items, ans, col, kind, want_cells, want_n):
    """a LIST column against the fixture (when the case's answer has one) and the restatement: cells, lengths, type codes, attribute bytes"""
    code = R.TYPE_CODE[kind]
    assert all(t == code and a == 0 for t, a, _ in items), (col, "type code / attribute byte")
    lens = np.array([len(v) for _, _, v in items], dtype=np.int64)
    razed = np.concatenate([v for _, _, v in items]) if items else np.empty(0, R.DTYPES[kind])
    assert np.array_equal(lens, want_n) and np.array_equal(razed.view(np.uint8), np.ascontiguousarray(want_cells).view(np.uint8)), col
    if ans is not None and col in ans:
        assert ans[col]["digest"] == R.digest(razed) and ans["n_" + col]["digest"] == R.digest(lens) and ans[col]["type"] == code, col


def run_select(ops, c, symbol=()):
    t = R.case_table(c)
    tab = host_table(t, symbol)
    q = {n: tup for n, _, tup in R.case_mappings(c)}
    if c["where"]:
        q["where"] = {"none": ("<", "i", 0), "one": ("==", "i", 0), "all": (">=", "i", 0), "some": ("<", "a", 37)}[c["where"]]
    q["by"] = "k"
    d = H.select_dict(q, tab)
    r = ops.rfx_select(d)
    assert r and not H.is_error(r), H.error_text(r)
    assert ops.rfx_last_select_on_gpu() == 1, ops.rfx_ops_last_error().decode()
    got = read_table(r)
    for o in (r, d, tab):
        ops.rfx_host_drop(o)
    return t, got


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_select_answers_the_fixture(ops, gold, c):
    ans = gold["answers"][c["name"]]
    t, got = run_select(ops, c)
    want = R.case_expected(c, t)
    assert list(got) == ["k"] + [n for n, _, _ in R.case_mappings(c)], "column order"
    for col in ("k", "s", "c", "f"):
        if col in want:
            assert np.array_equal(got[col], want[col]) and ans[col]["digest"] == R.digest(got[col]), col
    for kind in c["kinds"]:
        check_list(got[f"p_{kind}"], ans, f"p_{kind}", kind, want[f"p_{kind}"], want["n"])
    if c["row"]:
        check_list(got["r"], ans, "r", "i64", want["r"], want["n"])


def test_select_symbol_values_and_symbol_key(ops, gold):
    """SYMBOL cells are interned ids: the I64 case under the SYMBOL code, value column and key column"""
    c = [x for x in CASES if x["name"] == "groups257"][0]
    t, got = run_select(ops, c, symbol=("v_i64", "k"))
    want = R.case_expected(c, t)
    check_list(got["p_i64"], None, "p_i64", "symbol", want["p_i64"], want["n"])
    assert gold["answers"]["groups257"]["p_i64"]["digest"] == R.digest(np.concatenate([v for _, _, v in got["p_i64"]]))
    assert np.array_equal(got["k"], want["k"])


def test_select_by_dict_and_other_shapes_go_where_they_went(ops):
    c = [x for x in CASES if x["name"] == "rows65"][0]
    t = R.case_table(c)
    tab = host_table(t)
    for q, on_gpu, reason in (({"p": "v_i64", "by": {"kk": "k"}}, 1, None),
                              ({"p": "v_i64"}, 0, "mapping shape"),                           # no by:
                              ({"p": "v_i64", "by": {"k": "k", "a": "a"}}, 0, "mapping shape"),  # several keys
                              ({"p": "v_i64", "by": {"k": ("xbar", "k", 3)}}, 0, "mapping shape"),
                              ({"r": ("row", "vi"), "by": {"k": "k", "a": "a"}}, 0, "mapping is not (aggr ...)")):
        d = H.select_dict(q, tab)
        r = ops.rfx_select(d)
        assert ops.rfx_last_select_on_gpu() == on_gpu
        if on_gpu:
            got = read_table(r)
            want = R.group_collect(t["k"], [t["v_i64"]])
            assert list(got) == ["kk", "p"] and np.array_equal(got["kk"], want[0])
            check_list(got["p"], None, "p", "i64", want[2][0], np.diff(want[1]))
        else:
            assert H.is_error(r) and reason in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error().decode()
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(d)
    ops.rfx_host_drop(tab)


# ---- rfx_row / rfx_collect over MAPGROUP pairs ----
def call_pair(ops, fn, val, index, t=H.T_MAPGROUP):
    p = H.pair(val, index, t)
    r = getattr(ops, fn)(p)
    return p, r


@pytest.mark.parametrize("c", [c for c in CASES if c["where"] is None and c["n"] > 0], ids=lambda c: c["name"])
def test_row_and_collect_over_rfx_group_indexes(ops, c):
    t = R.case_table(c)
    want = R.case_expected(c, t)
    want["r"] = R.group_collect(t["k"], [])[3]  # (also for the cases whose query has no row mapping)
    itype = None
    for kind in c["kinds"] + ["row"]:
        kv = H.vector(t["k"])
        ix = ops.rfx_group(kv)
        assert ix and not H.is_error(ix), H.error_text(ix)
        itype = C.c_int64.from_address(H.list_items(ix)[0] + 8).value
        val = H.typed_vector(t["vi"] if kind == "row" else t[f"v_{kind}"], "i64" if kind == "row" else kind)
        p, r = call_pair(ops, "rfx_row" if kind == "row" else "rfx_collect", val, ix)
        assert r and not H.is_error(r), H.error_text(r)
        assert ops.rfx_last_collect_on_gpu() == 1
        check_list(H.list_to_numpy(r), None, kind, "i64" if kind == "row" else kind, want["r"] if kind == "row" else want[f"p_{kind}"], want["n"])
        for o in (r, p, kv):
            ops.rfx_host_drop(o)
    k = t["k"]
    rng = int(k.max() - k.min()) + 1
    assert itype == (1 if c["route"] == "shift" else 0), "the case's keys did not take the index flavour its route names"
    assert rng > 0


def filtered_index(t, mask, flavour):
    rows = np.flatnonzero(mask).astype(np.int64)
    sel = t["k"][rows]
    keys, gid = R.first_occurrence_ids(sel)
    if flavour == "ids":
        return rows, len(keys), H.group_index(0, len(keys), gid, filt=rows)
    lo = int(sel.min())
    table = np.full(int(sel.max()) - lo + 1, NULL, np.int64)
    table[keys - lo] = np.arange(len(keys))
    return rows, len(keys), H.group_index(1, len(keys), table, shift=lo, source=t["k"], filt=rows)


@pytest.mark.parametrize("flavour", ["ids", "shift"])
@pytest.mark.parametrize("name", ["where_one", "where_all", "where_some", "where_types", "where_some_65537"])
def test_row_and_collect_over_filtered_indexes(ops, gold, name, flavour):
    c = [x for x in CASES if x["name"] == name][0]
    t = R.case_table(c)
    want = R.case_expected(c, t)
    ans = gold["answers"][name]
    for kind in c["kinds"] + ["row"]:
        _, groups, ix = filtered_index(t, R.case_mask(c, t), flavour)
        val = H.typed_vector(t["vi"] if kind == "row" else t[f"v_{kind}"], "i64" if kind == "row" else kind)
        p, r = call_pair(ops, "rfx_row" if kind == "row" else "rfx_collect", val, ix)
        assert r and not H.is_error(r), H.error_text(r)
        assert ops.rfx_last_collect_on_gpu() == 1 and groups == len(want["k"])
        col = "r" if kind == "row" else f"p_{kind}"
        check_list(H.list_to_numpy(r), ans, col, "i64" if kind == "row" else kind, want[col], want["n"])
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(p)


def test_empty_answers_launch_nothing(ops):
    for groups, n in ((0, 0), (3, 0)):
        ix = H.group_index(0, groups, np.empty(n, np.int64))
        p, r = call_pair(ops, "rfx_collect", H.typed_vector(np.empty(n, np.int16), "i16"), ix)
        items = H.list_to_numpy(r)
        assert len(items) == groups and all(tp == 3 and a == 0 and len(v) == 0 for tp, a, v in items) and ops.rfx_last_collect_on_gpu() == 1
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(p)


def refused(ops, fn, p, reason):
    r = getattr(ops, fn)(p)
    assert H.is_error(r) and ops.rfx_last_collect_on_gpu() == 0
    text = ops.rfx_ops_last_error().decode()
    assert reason in text and reason in H.error_text(r), text
    ops.rfx_host_drop(r)
    ops.rfx_host_drop(p)


def test_shapes_handed_to_the_host(ops):
    k = R.key_column(100, 7)
    ids = lambda: H.group_index(0, 7, k)  # noqa: E731
    v = lambda: H.vector(np.arange(100, dtype=np.int64))  # noqa: E731
    for fn in ("rfx_row", "rfx_collect"):
        refused(ops, fn, H.pair(v(), H.vector(np.arange(5, dtype=np.int64)), H.T_MAPFILTER), R.HOST_SHAPES["mapfilter"])
        refused(ops, fn, v(), R.HOST_SHAPES["plain_vector"])
        refused(ops, fn, H.pair(v(), H.group_index(2, 7, k)), R.HOST_SHAPES["index_type"])
    refused(ops, "rfx_collect", H.pair(H.list_of([]), ids()), R.HOST_SHAPES["list_value"])
    c8 = H.lib().rfx_host_vector(12, 100)  # (C8: a type collect has no cells for)
    refused(ops, "rfx_collect", H.pair(c8, ids()), R.HOST_SHAPES["c8_value"])
    d = torch.arange(100, dtype=torch.int32, device="cuda")
    h = H.lib().rfx_host_device_vector(4, 100, (C.c_void_p * 1)(d.data_ptr()), 1)
    refused(ops, "rfx_collect", H.pair(h, ids()), R.HOST_SHAPES["device_i32"])


def failed(ops, fn, p, text):
    r = getattr(ops, fn)(p)
    assert H.is_error(r) and text in H.error_text(r), H.error_text(r)
    assert ops.rfx_last_collect_on_gpu() == 0
    ops.rfx_host_drop(r)
    ops.rfx_host_drop(p)


def test_malformed_indexes_are_errors(ops):
    """the check refuses: none of these inputs reaches a kernel that would use the bad cell as an index"""
    n = 5000
    k = R.key_column(n, 7)
    v = lambda: H.vector(np.arange(n, dtype=np.int64))  # noqa: E731
    for fn in ("rfx_row", "rfx_collect"):
        for bad in (7, -1, NULL):
            g = k.copy()
            g[n - 3] = bad
            failed(ops, fn, H.pair(v(), H.group_index(0, 7, g)), "a group id outside [0, groups)")
        table = np.arange(7, dtype=np.int64)
        src = k.copy()
        src[11] = 7  # one cell past the key table
        failed(ops, fn, H.pair(v(), H.group_index(1, 7, table, shift=0, source=src)), "a source cell outside the key table")
        src[11] = -1
        failed(ops, fn, H.pair(v(), H.group_index(1, 7, table, shift=0, source=src)), "a source cell outside the key table")
        failed(ops, fn, H.pair(v(), H.group_index(0, 7, k, filt=np.arange(n - 1, dtype=np.int64))), "group ids / filter length mismatch")
        short = H.list_of([H.atom(0), H.atom(7), H.vector(k)])
        failed(ops, fn, H.pair(v(), short), "malformed group index")
    failed(ops, "rfx_collect", H.pair(H.vector(np.arange(n - 1, dtype=np.int64)), H.group_index(0, 7, k)), "length")
    filt = np.arange(n, dtype=np.int64)
    filt[5] = n  # a filter id one past the column
    failed(ops, "rfx_collect", H.pair(v(), H.group_index(0, 7, k, filt=filt)), "a filter id outside the column")


_CHILD = """
import os, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np
import collect_ref as R
from rayforce_amd import hostobj as H
ops = H.lib(); ops.rfx_host_bind()
{body}
"""


def test_a_sharded_door_hands_back(built):
    """RFX_SHARDS=2 in a process of its own (the operator layer's shards are fixed at its first call)"""
    body = """
k = R.key_column(4096, 7)
p = H.pair(H.vector(np.arange(4096, dtype=np.int64)), H.group_index(0, 7, k))
r = ops.rfx_row(p)
assert H.is_error(r) and ops.rfx_last_collect_on_gpu() == 0 and ops.rfx_ops_shards() == 2
print(ops.rfx_ops_last_error().decode())
tab = H.table({"k": k, "v": np.arange(4096, dtype=np.int64)})
r = ops.rfx_select(H.select_dict({"p": "v", "by": "k"}, tab))
assert H.is_error(r) and ops.rfx_last_select_on_gpu() == 0
print(ops.rfx_ops_last_error().decode())
"""
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT, body=body)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RFX_SHARDS="2", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "collect over a sharded table" in p.stdout and "mapping shape" in p.stdout
