"""The numpy restatement of the bucket verbs (tests/bucket_ref.py) against every case of tests/golden/bucket_golden.npz -- the compiled reference's own
answers, with one thread and with eight -- bit for bit, type code included; and the library's surface for them.  No GPU."""
import os
import re

import numpy as np
import pytest

import bucket_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = B.load_cases()


@pytest.mark.parametrize("verb", ["xrank", "xbar", "within", "floor", "ceil", "round", "neg"])
def test_restatement_matches_reference(verb):
    mine = [c for c in CASES if c["verb"] == verb]
    assert mine
    for c in mine:
        got, ot = B.answer(c)
        assert ot == c["ot"], c["name"]
        want = B.as_bits(c["out"])
        got = B.as_bits(got)
        assert got.dtype == want.dtype and got.shape == want.shape, (c["name"], got.dtype, want.dtype, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (c["name"], bad[:5], got[bad[:5]], want[bad[:5]])


def test_fixture_covers_what_it_names():
    names = {c["name"] for c in CASES}
    lens = {len(c["x"]) for c in CASES if not c["xa"]}
    assert {0, 1, 63, 64, 65, 4097, 20011, 2**20 + 5} <= lens
    for verb in ("xrank", "xbar", "within", "floor", "ceil", "round", "neg"):
        assert any(c["verb"] == verb and len(c["x"]) == 2**20 + 5 for c in CASES), verb
    assert {c["attrs"] for c in CASES if c["verb"] == "xrank"} == {0, 2, 4}
    assert {c["yt"] for c in CASES if c["verb"] == "xrank"} == {2, 3, 4, 5}  # the bucket count as -U8, -I16, -I32, -I64
    arms = {(c["xt"], c["yt"], c["xa"], c["ya"]) for c in CASES if c["verb"] == "xbar"}
    for xt, yt in [(4, 4), (4, 5), (4, 10), (5, 4), (5, 5), (5, 10), (10, 4), (10, 5), (10, 10), (7, 4), (7, 5), (8, 4), (8, 5), (8, 8), (9, 4), (9, 5), (9, 8)]:
        assert B.xbar_arm(xt, yt) is not None
        assert {(xt, yt, False, True), (xt, yt, True, False), (xt, yt, False, False)} <= arms, (xt, yt)
    assert {"within_lo_gt_hi", "within_lo_null", "xbar_f64_y_zero", "xbar_f64_beyond_2p63", "floor_edges", "ceil_edges", "round_edges"} <= names


def test_headers_declare_the_bucket_entry_points():
    text = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("rfx_hip.h", "rfx_exec.h", "rfx_ops.h")}
    for fn in ("rfx_hip_xrank", "rfx_hip_xrank_sorted", "rfx_hip_xbar", "rfx_hip_round_f64", "rfx_hip_neg", "rfx_hip_within_i64"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_hip.h"]), fn
    for fn in ("rfx_exec_xrank", "rfx_exec_xbar", "rfx_exec_round", "rfx_exec_neg", "rfx_exec_within"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_exec.h"]), fn
    for fn in ("rfx_xrank", "rfx_xbar", "rfx_within", "rfx_floor", "rfx_ceil", "rfx_round", "rfx_neg", "rfx_last_bucket_on_gpu"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_ops.h"]), fn
    # appended after the last id that existed, nothing renumbered
    assert re.search(r"RFX_XSTAT_NS_SET_PROBE = 27", text["rfx_exec.h"]) and re.search(r"RFX_XSTAT_XRANKS = 28", text["rfx_exec.h"])
