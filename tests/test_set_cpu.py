"""The set verbs without a GPU: the numpy restatement (tests/set_ref.py) against the fixture the compiled reference wrote
(tests/golden/set_golden.npz, maker beside it), the priority-insert construction of the device's hash-route `distinct` against the same
fixture, and the built library's exports."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import set_ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "set_golden.npz")
SYMBOLS = ("rfx_distinct", "rfx_find", "rfx_in", "rfx_sect", "rfx_except", "rfx_union", "rfx_last_set_on_gpu", "rfx_set_stats")


def unplane(p):
    return np.ascontiguousarray(p.T).reshape(-1).view(np.int64).copy()


def load_cases():
    z = np.load(GOLDEN)
    out = []
    for k, meta in enumerate(z["cases"]):
        name, verb, tp, atom, route, rtype, attrs, threads = str(meta).split("|")
        c = dict(name=name, verb=verb, type=int(tp), atom=atom == "1", route=route, rtype=int(rtype), attrs=int(attrs), x=unplane(z[f"c{k}_x"]),
                 y=unplane(z[f"c{k}_y"]) if f"c{k}_y" in z.files else None, out=unplane(z[f"c{k}_out"]) if f"c{k}_out" in z.files else None)
        out.append(c)
    return out


CASES = load_cases()
DEFINED = [c for c in CASES if not c["name"].startswith("host_")]
HOST = [c for c in CASES if c["name"].startswith("host_")]


def restated(c):
    if c["verb"] == "distinct":
        return set_ref.distinct(c["x"])
    return set_ref.VERBS[c["verb"]](c["x"], int(c["y"][0]) if c["atom"] else c["y"])


def test_fixture_shape():
    assert len(DEFINED) >= 120 and len(HOST) >= 10
    verbs = {c["verb"] for c in DEFINED}
    assert verbs == {"distinct", "in", "find", "sect", "except", "union"}
    for v in verbs:
        assert {c["route"] for c in DEFINED if c["verb"] == v} >= {"dense", "hash"}, v
    for c in DEFINED:  # a case's name says the route it was built for
        for r in ("dense", "hash"):  # (an empty operand takes no route at all, an empty set or two scopes that do not meet the disjoint one)
            if f"_{r}" in c["name"] and not c["name"].startswith("union_dense_hal"):
                assert c["route"] in (r, "none", "disjoint"), c["name"]
    assert all(c["route"] == "undefined" and c["out"] is None for c in HOST)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("c", DEFINED, ids=lambda c: c["name"])
def test_restatement_equals_reference(c):
    got, route = restated(c)
    assert not isinstance(got, str), (c["name"], route)
    assert route == c["route"]
    assert np.array_equal(got.astype(np.int64), c["out"]), c["name"]
    # the answer's type: x's for distinct / union / sect / except, B8 for in, I64 for find; ATTR_DISTINCT (1) on distinct / union only
    want_type = {"in": 1, "find": 5}.get(c["verb"], c["type"])
    assert c["rtype"] == want_type
    if c["attrs"] >= 0:
        assert c["attrs"] == (1 if c["verb"] in ("distinct", "union") else 0)


@pytest.mark.parametrize("c", HOST, ids=lambda c: c["name"])
def test_restatement_declines_the_undefined_shapes(c):
    got, why = restated(c)
    assert got == set_ref.UNDEFINED and why


@pytest.mark.parametrize("c", [c for c in DEFINED if c["verb"] in ("distinct", "union") and c["route"] == "hash" and c["x"].size < 100000], ids=lambda c: c["name"])
def test_priority_insert_rebuilds_the_reference_table(c):
    """What k_set_prio_insert does, in shuffled orders: the first row of every distinct key goes into cell key % P by MIN, the displaced larger
    row walks on.  The cells read in slot order must be the fixture's answer, whatever the order of the inserts."""
    a = c["x"] if c["y"] is None else np.concatenate([c["x"], c["y"]])
    keys, first = np.unique(a[a != set_ref.NULL], return_index=True)
    P = set_ref.table_cells(a.size)
    rng = np.random.default_rng(len(c["name"]))
    for order in (np.arange(keys.size), np.arange(keys.size)[::-1], rng.permutation(keys.size), rng.permutation(keys.size)):
        cells = set_ref.priority_table(first, keys, P, order)
        got = np.array([a[r] for r in cells if r is not None], np.int64)
        assert np.array_equal(got, c["out"]), c["name"]


def test_table_cells():
    assert [set_ref.table_cells(n) for n in (0, 1, 3, 4, 63, 4097)] == [2, 2, 5, 7, 89, 5471]


def test_library_exports_the_set_verbs():
    path = os.environ.get("RFX_LIB") or os.path.join(os.path.dirname(HERE), "rayforce_amd", "librfx.so")
    assert os.path.exists(path), "librfx.so is not built"
    lib = ctypes.CDLL(path)
    for s in SYMBOLS + ("rfx_exec_distinct", "rfx_exec_member", "rfx_exec_set_filter", "rfx_hip_set_probe", "rfx_hip_set_priority_insert", "rfx_hip_set_compact"):
        assert hasattr(lib, s), s
    lib.rfx_set_table_cells.restype = ctypes.c_int64
    lib.rfx_set_table_cells.argtypes = [ctypes.c_int64]
    assert [lib.rfx_set_table_cells(n) for n in (0, 1, 3, 4, 63, 4097, 20011, 10**8)] == [set_ref.table_cells(n) for n in (0, 1, 3, 4, 63, 4097, 20011, 10**8)]
