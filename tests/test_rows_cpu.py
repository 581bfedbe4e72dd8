"""The numpy restatement of the row verbs (tests/rows_ref.py) against every case of tests/golden/rows_golden.npz -- the compiled reference's own answers,
with one thread and with eight -- bit for bit, type code and attributes included; and the library's surface for them.  No GPU."""
import os
import re

import numpy as np
import pytest

import rows_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_cases()
LENS = {0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4097, 20011, 2**20 + 5}


@pytest.mark.parametrize("verb", ["filter", "take", "reverse"])
def test_restatement_matches_reference(verb):
    mine = [c for c in CASES if c["verb"] == verb and c["host"] is None]
    assert mine
    for c in mine:
        got = R.answer(c)
        assert len(got) == len(c["out"]), c["name"]
        for (gt, ga, gc), (wt, wa, wc) in zip(got, c["out"]):
            assert (gt, ga) == (wt, wa), (c["name"], gt, ga, wt, wa)
            g, w = R.as_bits(gc), R.as_bits(wc)
            assert g.dtype == w.dtype and g.shape == w.shape, (c["name"], g.dtype, w.dtype, g.shape, w.shape)
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (c["name"], bad[:5], g[bad[:5]], w[bad[:5]])


def test_fixture_covers_what_it_names():
    names = {c["name"] for c in CASES}
    ok = [c for c in CASES if c["host"] is None]
    assert all(c["threads"] == "1,8" for c in CASES)
    assert LENS <= {len(c["cols"][0][2]) for c in ok if c["verb"] == "filter"}
    for mask in ("zero", "one", "first", "last", "row511", "row512", "alternating", "every64th", "random1", "random50", "random99", "true2", "true128", "true255"):
        assert {f"filter_i64_len{n}_{mask}" for n in (1, 129, 513, 1025, 20011)} <= names, mask
    assert {len(c["cols"]) for c in ok if c["verb"] == "filter" and c["table"]} >= {1, 8, 9}
    assert any(max(c["alias"]) >= 0 for c in ok if c["verb"] == "filter")  # one vector under two names
    for verb in ("filter", "take", "reverse"):
        assert {tp for c in ok if c["verb"] == verb for tp, _a, _c in c["cols"]} >= {R.I64, R.TS, R.F64, R.I32, R.DATE, R.TIME, R.B8}, verb
    takes = [c for c in ok if c["verb"] == "take"]
    assert {len(c["cols"][0][2]) for c in takes if not c["atom"]} >= {1, 2, 63, 64, 65, 4097}
    assert {c["count"][1] for c in takes if c["count"][0] == "atom"} == {R.I64, R.I32, R.I16}
    for l in (1, 2, 63, 64, 65, 4097):  # every m with both signs and all three count types at every length
        for k in range(7):
            for sign in ("pos", "neg"):
                assert {f"take_len{l}_m{k}_{sign}_t{ct}" for ct in (R.I64, R.I32, R.I16)} <= names, (l, k, sign)
        for start in (0, 1, -1, -l, -l - 5, l, l + 5):
            assert {f"take_len{l}_range_{start}_{amount}" for amount in (0, 1, l, l + 7)} <= names, (l, start)
    assert any(c["count"][0] == "atom" and c["count"][2] < 0 for c in takes) and any(c["count"][0] == "range" and c["count"][1] < 0 for c in takes)
    assert {tp for c in takes if c["atom"] for tp, _a, _c in c["cols"]} >= {R.I64, R.TS, R.F64, R.I32, R.DATE, R.TIME, R.B8}
    assert {c["cols"][0][1] for c in ok if c["verb"] == "reverse"} >= {0, R.ATTR_ASC, R.ATTR_DESC, R.ATTR_ASC | R.ATTR_DISTINCT}
    hosts = {c["host"] for c in CASES if c["host"]}
    assert {"not a vector of a row type", "a parted table", "a table with no columns", "a mask that is not a B8 vector", "length", "a negative range amount",
            "count type", "take from an empty vector", "take from an empty table", "a count of INT64_MIN", "start + amount does not fit 63 bits", "a table"} <= hosts
    assert all(c["ref_error"] for c in CASES if c["name"] in ("host_filter_mask_not_b8", "host_filter_lengths_differ", "host_take_negative_amount",
                                                               "host_take_count_f64", "host_reverse_table"))
    assert os.path.getsize(R.GOLDEN) < 2**20


def test_take_window_is_the_references_arithmetic():
    # j0 = (l - m % l) * (count < 0), every index taken mod l (core/items.c:451)
    for l in (1, 2, 63, 64, 65):
        for m in range(0, 3 * l + 2):
            j0, mm = R.take_window(l, ("atom", R.I64, -m))
            assert mm == m and j0 == ((l - m % l) * 1) % l
            assert R.take_window(l, ("atom", R.I32, m)) == (0, m)
    assert R.take_window(10, ("range", -3, 9)) == (7, 3) and R.take_window(10, ("range", -15, 4)) == (0, 4) and R.take_window(10, ("range", 15, 4)) == (10, 0)
    assert R.take_window(10, ("range", 1, -2)) is None and R.take_window(0, ("atom", R.I64, 0)) is None and R.take_window(5, ("atom", R.F64, 2)) is None


def test_headers_declare_the_row_entry_points():
    text = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("rfx_hip.h", "rfx_exec.h", "rfx_ops.h")}
    for fn in ("rfx_hip_rows_compact", "rfx_hip_rows_take", "rfx_hip_rows_reverse", "rfx_hip_rows_fill"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_hip.h"]), fn
    for fn in ("rfx_exec_filter", "rfx_exec_rows_piece", "rfx_exec_rows_free", "rfx_exec_take", "rfx_exec_take_atom", "rfx_exec_reverse"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_exec.h"]), fn
    for fn in ("rfx_filter", "rfx_take", "rfx_reverse", "rfx_last_rows_on_gpu"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_ops.h"]), fn
    # appended after the last id that existed, nothing renumbered
    assert re.search(r"RFX_XSTAT_BUCKET_MAPS = 30", text["rfx_exec.h"]) and re.search(r"RFX_XSTAT_ROWS_FILTERS = 31", text["rfx_exec.h"])
    from rayforce_amd import _lib as L
    from rayforce_amd import hostobj as H
    assert {"rfx_hip_rows_compact", "rfx_exec_filter", "rfx_exec_take", "rfx_exec_reverse"} <= set(L.PROTOTYPES)
    assert {"rfx_filter", "rfx_take", "rfx_reverse", "rfx_last_rows_on_gpu"} <= set(H.OPS_PROTOTYPES)
