"""What the operator door decides before it touches a device -- the verb table behind rfx_host_fn, every hand-off reason a call can reach without one, the
null-argument failures, the answers that need no device -- against tests/golden/handoff_golden.json (tests/golden/make_handoff_golden.py recorded it from
the library itself), byte for byte: error texts, rfx_ops_last_error(), the families' rfx_last_*_on_gpu() and counters.  No GPU."""
import json
import os

import pytest

import handoff_door as D

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "handoff_golden.json")))
CALLS = GOLDEN["calls"]
# the reasons of the nine families and of med / dev that lie before ensure_ctx() in rayforce_amd/csrc/rfx_ops_*.c
REASONS = {
    "sort": ["key type", "a device column that is not I64 / F64 / TIMESTAMP / B8", "the reference's reverse has no I16 arm", "not a table",
             "sort columns are not symbols", "parted table", "too many columns", "a column that is not an 8-byte vector", "no such column"],
    "asof": ["expected (keys, left table, right table)", "expected (symbol vector, table, table)", "fewer than two key names", "parted table",
             "more than 8 equality keys", "asof column missing from a table", "asof columns of different types", "asof column type",
             "equality key is not an 8-byte integer column of both tables", "non-8-byte column", "columns of different lengths", "too many columns",
             "operands are not two I64 or two TIMESTAMP vectors"],
    "window": ["expected (keys, windows, left table, right table, aggregates)", "expected (symbol vector, list, table, table, dict)", "fewer than two key names",
               "parted table", "more than 8 equality keys", "window column missing from a table", "window columns of different types", "window column type",
               "equality key is not an 8-byte integer column of both tables", "columns of different lengths", "windows are not a list of two vectors",
               "windows are not two 4-byte integer vectors of the left table's length", "aggregates are not a dict of expressions by name", "more than 64 aggregates",
               "an aggregate is not of the form (agg column): a raw column or an atom", "an aggregate is not of the form (agg column)",
               "an aggregate other than sum, min, max, count, avg, first, last", "an aggregate of an expression", "an aggregate of a column the right table lacks",
               "an aggregate of a column that is neither I64 nor F64", "more than 16 aggregated columns"],
    "set": ["the first operand is not a plain I64, SYMBOL or TIMESTAMP vector", "the operands are not two vectors of one 8-byte integer type",
            "sect / except take I64 or SYMBOL pairs"],
    "bucket": ["bucket count type", "domain", "key type", "(len - 1) * n does not fit 63 bits", "atom and atom", "operand types", "length", "a 4-byte device column",
               "an atom", "not an F64 vector", "not an I32 / I64 / F64 vector", "not an I64 vector against a 2-cell I64 vector"],
    "rows": ["a parted table", "a table with no columns", "a column that is not a vector of a row type", "not a vector of a row type", "a 4-byte device column",
             "columns of unequal length", "a mask that is not a B8 vector", "length", "a negative range amount", "start + amount does not fit 63 bits", "count type",
             "a count of INT64_MIN", "not an atom of a row type", "device memory", "take from an empty table", "take from an empty vector", "a table"],
    "cast": ["the type name is not a symbol atom", "a type name outside the nine numeric and temporal types", "an atom",
             "not a vector of the nine numeric and temporal types", "a device column that is not I64 / F64 / TIMESTAMP / B8",
             "the reference has no cast between B8 and U8 vectors"],
    "fold": ["value type", "filter ids"],
}
FAMILY = {"rfx_last_sort_on_gpu": "sort", "rfx_last_asof_on_gpu": "asof", "rfx_last_window_on_gpu": "window", "rfx_last_set_on_gpu": "set",
          "rfx_last_bucket_on_gpu": "bucket", "rfx_last_rows_on_gpu": "rows", "rfx_last_cast_on_gpu": "cast", None: "fold"}
NULLS = ["sort: null argument", "bin: null argument", "set verb: null argument", "xrank: null argument", "xbar: null argument", "round: null argument",
         "neg: null argument", "within: null argument", "filter: null argument", "take: null argument", "reverse: null argument", "as: null argument",
         "med: null argument", "dev: null argument"]


@pytest.fixture(scope="module")
def ops(built):
    from rayforce_amd import hostobj as H
    lib = H.lib()
    lib.rfx_host_bind()
    return lib


@pytest.fixture(scope="module")
def replayed(ops):
    """every call of the fixture again, in its order, in one go (a call that leaves the last error or a flag alone shows what the one before it left)"""
    return [D.run_case(ops, c) for c in CALLS]


def test_the_verb_table_behind_rfx_host_fn(ops):
    by_address = D.exported(ops)
    assert len(GOLDEN["functions"]) == 53
    for name, want in GOLDEN["functions"].items():
        assert D.fn_record(ops, name, by_address) == want, name
    for name in GOLDEN["unknown"]:
        assert ops.rfx_host_fn(name.encode()) is None, name
    # the pairings that look odd and are meant
    assert GOLDEN["functions"]["div"][2] == "rfx_div" and GOLDEN["functions"]["/"][2] == "rfx_floordiv" and GOLDEN["functions"]["and"][2] == "rfx_and"


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[c["name"] for c in CALLS])
def test_call_before_the_device(replayed, i):
    assert json.dumps(replayed[i], sort_keys=True) == json.dumps(CALLS[i]["record"], sort_keys=True), CALLS[i]["name"]


def test_the_fixture_covers_the_door():
    assert len(CALLS) >= 80 and {c["verb"] for c in CALLS} == set(D.VERBS)
    texts = {}
    for c in CALLS:
        err = c["record"]["answer"].get("error")
        assert "no usable MI355X" not in json.dumps(c["record"]), c["name"]  # (nothing here reaches ensure_ctx())
        if err:
            texts.setdefault(FAMILY[D.VERBS[c["verb"]][2]], set()).add(err)
    for family, reasons in REASONS.items():
        for why in reasons:
            assert any(f"({why}) and no host" in t for t in texts[family]), (family, why)
    every = set().union(*texts.values())
    assert set(NULLS) <= every and "join: a column has different types in the two tables" in every
    answers = {c["name"]: c["record"] for c in CALLS if "error" not in c["record"]["answer"]}
    assert answers["as_same_type"]["answer"]["is_argument"] == 1 and answers["as_same_type"]["on_gpu"] == 1
    assert answers["asc_of_asc_i64"]["answer"]["is_argument"] == 0 and answers["desc_of_asc_i64"]["answer"]["attrs"] == 4
    assert answers["rank_of_desc_i64"]["answer"]["attrs"] == 0 and answers["iasc_of_desc_i64"]["answer"]["attrs"] == 5
    assert {"xasc_empty_symbols", "xrank_empty_count_i64", "filter_empty_table", "filter_empty_5", "as_empty_5_F64", "wj_empty_left", "bin_empty_right"} <= set(answers)
    assert "asc_of_desc_i16" not in answers and "the reference's reverse has no I16 arm" in CALLS[[c["name"] for c in CALLS].index("asc_of_desc_i16")]["record"]["last_error"]
    assert all(len(t) < 256 for t in every)  # no reason reachable without a device is long enough to be cut by a message buffer
