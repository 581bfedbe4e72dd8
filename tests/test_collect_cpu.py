"""`row` and the collected column of select ... by: without a GPU: the numpy restatement (tests/collect_ref.py) against every case of the compiled reference's
fixture (tests/golden/collect_golden.npz, made by tests/golden/make_collect_golden.py), and the fixture's own integrity -- every case of the list has an
answer, every answer column a digest, a type code and an attribute byte."""
import json
import os

import numpy as np
import pytest

import collect_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collect_golden.npz")
CASES = R.cases()


@pytest.fixture(scope="module")
def gold():
    return json.loads(bytes(np.load(GOLD)["json"]).decode())


def test_fixture_holds_every_case(gold):
    assert gold["cases"] == [c["name"] for c in CASES]
    assert gold["failed"] == {}, "cases the reference did not answer, or answered differently with 1 and 8 threads"
    assert sorted(gold["answers"]) == sorted(gold["cases"])
    assert os.path.getsize(GOLD) < 2_000_000
    # the group ORDER under where: with many groups follows the pool (the maker checks that nothing else does): the fixture keeps the one-thread order
    assert set(gold["order_differs_with_8_threads"]) <= {c["name"] for c in CASES if c["where"] and c["groups"] > 4097}
    for name, ans in gold["answers"].items():
        for col, d in ans.items():
            dt, n, sha = d["digest"].split("|")
            assert len(sha) == 64 and int(n) >= 0 and np.dtype(dt).itemsize in (1, 2, 4, 8), (name, col)
            assert d["attrs"] == 0 or col in ("k", "s", "c", "f"), (name, col)


def test_cases_cover_the_listed_shapes():
    assert {c["n"] for c in CASES} >= {0, 1, 63, 64, 65, 4097, 70001}
    assert {c["groups"] for c in CASES} >= {1, 2, 255, 256, 257, 65537}
    assert {k for c in CASES for k in c["kinds"]} == set(R.RECORDED)
    assert {c["where"] for c in CASES} == {None, "none", "one", "all", "some"}
    assert {c["route"] for c in CASES} == {"shift", "dense", "sparse"} and {c["shape"] for c in CASES} == {"cycle", "heavy", "own"}
    for c in CASES:  # the key ranges really are what the routes' names say (rfx_group: range <= rows -> table / dense ids by 524 288, else hashed)
        k = R.case_table(c)["k"]
        if len(k) == 0:
            continue
        rng = int(k.max() - k.min()) + 1
        assert {"shift": rng <= len(k) and rng <= 524288, "dense": 524288 < rng <= len(k), "sparse": rng > len(k)}[c["route"]], c["name"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_the_reference(gold, c):
    ans = gold["answers"][c["name"]]
    want = R.case_expected(c)
    empty = len(want["k"]) == 0
    seen = set()
    for col, d in ans.items():
        if col.startswith("n_"):
            assert d["digest"] == R.digest(want["n"]), col
            continue
        assert d["digest"] == R.digest(want[col]), col
        seen.add(col)
        if col.startswith("p_"):
            assert d["type"] == R.TYPE_CODE[col[2:]]
        elif col != "k":
            assert d["type"] == R.TYPE_CODE["i64"]
    nested = {n for n, _, t in R.case_mappings(c) if not (isinstance(t, tuple) and t[0] != "row")}
    assert seen == set(want) - {"n"} - (nested if empty else set()), "a column of the query without an answer in the fixture"


def test_restatement_index_flavours():
    """IDS and SHIFT, with and without a filter, name the same groups; malformed indexes raise"""
    key = R.key_column(4097, 257, base=-40)
    rows = np.flatnonzero(R.value_column("i64", 4097, 9) % 100 < 37)
    for filt in (None, rows):
        sel = key if filt is None else key[filt]
        keys, gid = R.first_occurrence_ids(sel)
        table = np.full(int(sel.max() - sel.min()) + 1, R.NULL_I64, np.int64)
        table[keys - sel.min()] = np.arange(len(keys))
        assert np.array_equal(R.ids_of_index("ids", len(sel), ids=gid, rows=filt), gid)
        assert np.array_equal(R.ids_of_index("shift", len(sel), source=key, table=table, shift=sel.min(), rows=filt), gid)
        with pytest.raises(ValueError):
            R.ids_of_index("shift", len(sel), source=key, table=table[:-1], shift=sel.min(), rows=filt)
    with pytest.raises(ValueError):
        R.partition(np.array([0, 3]), 3)
    off, perm = R.partition(np.array([2, 0, 2, 0]), 4)
    assert off.tolist() == [0, 2, 2, 4, 4] and perm.tolist() == [1, 3, 0, 2]
    assert [x.tolist() for x in R.lists(off, np.array([10, 11, 12, 13])[perm])] == [[11, 13], [], [10, 12], []]
