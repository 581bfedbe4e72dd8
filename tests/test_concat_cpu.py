"""concat and raze without a GPU: the numpy restatement (tests/concat_ref.py) equals every case the compiled reference answered
(tests/golden/concat_golden.npz); the two verb rows behind rfx_host_fn; every reason the door gives before it needs a device, with its text in
rfx_ops_last_error(); the null-argument failure; the answers that launch nothing."""
import ctypes as C

import numpy as np
import pytest

import concat_door as D
import concat_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H

CASES = R.load_cases()


@pytest.fixture(scope="module")
def ops(built):
    o = H.lib()
    o.rfx_host_bind()
    return o


def test_the_fixture_holds_what_the_issue_lists():
    names = {c["name"] for c in CASES}
    for tp, w in ((R.B8, 1), (R.I16, 2), (R.I32, 4), (R.DATE, 4), (R.TIME, 4), (R.I64, 8), (R.TS, 8), (R.F64, 8)):
        xlens = {1: (0, 1, 15, 16, 17), 2: (0, 7, 8, 9), 4: (0, 3, 4, 5), 8: (0, 1, 2, 3)}[w]
        for xl in xlens:
            for yl in (0, 1, 5, 64, 4097):
                assert f"concat_vv_t{tp}_x{xl}_y{yl}" in names
            assert f"concat_va_t{tp}_len{xl}" in names and f"concat_av_t{tp}_len{xl}" in names
    assert {f"concat_big_t{tp}" for tp in (R.B8, R.I16, R.I32, R.I64)} <= names
    assert {"table1", "table3", "table9", "table3_x0", "table3_y0", "table3_both0"} <= names
    for tp in (R.B8, R.I16, R.I32, R.I64):
        assert {f"raze_t{tp}_n{n}" for n in (1, 2, 7, 1000, 5000)} | {f"raze_t{tp}_all_empty"} <= names
    assert {c["shape"] for c in CASES if c.get("host")} == set(R.HOST_SHAPES)


def test_the_restatement_equals_every_golden_case():
    ran = 0
    for c in CASES:
        if c.get("host"):
            continue
        got = R.answer(c)
        assert len(got) == len(c["out"]), c["name"]
        for (tp, attrs, cells), want in zip(got, c["out"]):
            D.same_column(c["name"], tp, attrs, cells, want)
        ran += 1
    assert ran > 300


def test_the_long_cases_put_a_span_boundary_inside_a_later_tile():
    for c in CASES:
        if c["name"].startswith("concat_big"):
            tp, parts = c["cols"][0]
            nbytes = len(parts[0]) * np.dtype(R.DTYPE[tp]).itemsize
            assert len(parts[0]) + len(parts[1]) == 2**20 + 5 and nbytes > 16384 and nbytes % 16 != 0 and nbytes % 16384 != 0, c["name"]


def test_the_verb_rows_are_bound_by_name(ops):
    for name, tp in (("concat", 102), ("raze", 101)):
        fn = ops.rfx_host_fn(name.encode())
        assert fn and H.header(fn).type == tp and H.header(fn).attrs == 0
        addr = C.c_int64.from_address(H.payload(fn) - 8).value
        assert addr == C.cast(getattr(ops, "rfx_" + name), C.c_void_p).value, name
        ops.rfx_host_drop(fn)


def test_every_reason_reachable_without_a_device(ops):
    hosts = [c for c in CASES if c.get("host")]
    assert len(hosts) == len(R.HOST_SHAPES)
    for c in hosts:
        D.check_refused(ops, c)


def test_null_arguments_fail(ops):
    v = D.host_vector(ops, np.arange(3, dtype=np.int64), R.I64)
    for f, text in ((lambda: ops.rfx_concat(None, v), "concat: null argument"), (lambda: ops.rfx_concat(v, None), "concat: null argument"),
                    (lambda: ops.rfx_raze(None), "raze: null argument")):
        r = f()
        assert r and H.is_error(r) and ops.rfx_ops_last_error().decode() == text and text in H.error_text(r)
        ops.rfx_host_drop(r)
    ops.rfx_host_drop(v)


def test_empty_answers_launch_nothing(ops):
    """(no context is made: these pass without a device)"""
    for c in CASES:
        if not c.get("host") and all(len(cells) == 0 for _tp, _a, cells in c["out"]):
            D.check_door(ops, c)


def test_ctypes_mirror_the_headers():
    assert C.sizeof(L.Span) == 24 and C.sizeof(L.ConcatCol) == 32
    assert (L.RFX_XSTAT_CONCATS, L.RFX_XSTAT_CONCAT_SPANS, L.RFX_XSTAT_CONCAT_CELLS) == (41, 42, 43)
