"""The numpy restatement of `as` over vectors (tests/cast_ref.py) against every case of tests/golden/cast_golden.npz -- the compiled reference's own
answers, with one thread and with eight, under both spellings of the type name -- bit for bit, type code and attribute byte included; and the library's
surface for the verb.  No GPU."""
import os
import re

import numpy as np
import pytest

import cast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_cases()


@pytest.mark.parametrize("st", R.TYPES)
def test_restatement_matches_reference(st):
    mine = [c for c in CASES if c["st"] == st and not c["host"]]
    assert mine
    for c in mine:
        got = R.cast(c["x"], c["st"], c["dt"])
        assert c["ot"] == c["dt"] and got.dtype == c["out"].dtype, (c["name"], c["ot"], got.dtype, c["out"].dtype)
        assert c["oattrs"] == (c["attrs"] if c["st"] == c["dt"] else 0), c["name"]  # a clone keeps its attributes, a converted vector has none
        got, want = R.as_bits(got), R.as_bits(c["out"])
        assert got.shape == want.shape, (c["name"], got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (c["name"], bad[:5], got[bad[:5]], want[bad[:5]])


def test_fixture_covers_what_it_names():
    arms = {(c["st"], c["dt"], c["spelling"], c["n"]) for c in CASES if not c["host"]}
    for st in R.TYPES:
        for dt in R.TYPES:
            for sp in ("atom", "vector"):
                for n in R.LENS:
                    assert ((st, dt, sp, n) in arms) == (n == 0 or R.has_arm(st, dt)), (st, dt, sp, n)
    big = {(c["st"], c["dt"]) for c in CASES if c["n"] == R.BIG}
    assert {(R.I64, R.F64), (R.F64, R.I64), (R.I64, R.I32), (R.I32, R.I64), (R.F64, R.U8)} <= big
    assert {c["threads"] for c in CASES if not c["host"]} == {"1,8"}
    hosts = [c for c in CASES if c["host"]]
    assert {(c["st"], c["dt"], c["spelling"]) for c in hosts} >= {(R.B8, R.U8, "atom"), (R.B8, R.U8, "vector"), (R.U8, R.B8, "atom"), (R.U8, R.B8, "vector")}
    assert all(c["ref_error"] for c in hosts)  # each of them is an error of the reference's own
    # the cells the table of arms was observed over, in every integer and F64 source long enough to hold the period
    ints = {0, 1, -1, 255, 256, 32768, -32768, 2**31, -(2**31), 2**31 - 1, R.NULL64, 2**63 - 1}
    x = next(c["x"] for c in CASES if c["st"] == R.I64 and c["n"] == 63)
    assert ints <= set(x.tolist())
    x = next(c["x"] for c in CASES if c["st"] == R.I32 and c["n"] == 63)
    assert {v for v in ints if -(2**31) <= v < 2**31} <= set(x.tolist())
    f = next(c["x"] for c in CASES if c["st"] == R.F64 and c["n"] == 63)
    want = [0.0, -0.0, 0.5, -0.5, 1.9, -1.9, 255.0, 256.0, 300.7, 32767.9, 32768.0, -32769.0, 2147483647.0, 2147483648.0, -2147483648.5, -2147483649.0,
            2.0**32 + 5, 9.3e18, -9.3e18, np.inf, -np.inf, 5e-324]
    assert set(np.array(want).view(np.uint64).tolist()) <= set(f.view(np.uint64).tolist()) and np.isnan(f).any()


def test_the_table_of_arms_as_observed():
    """the rows of the reference's behaviour the device path was built to, each read off the fixture's own cells"""
    def answer(st, dt, cell):
        for c in CASES:
            if c["st"] == st and c["dt"] == dt and not c["host"] and c["n"] >= 63:
                at = np.flatnonzero(R.as_bits(c["x"]) == R.as_bits(np.array([cell], R.DTYPE[st]))[0])
                if at.size:
                    return c["out"][at[0]].item()
        raise AssertionError((st, dt, cell))
    assert answer(R.I64, R.B8, -1) == -1 and answer(R.I64, R.U8, -1) == 255  # the low byte, not != 0
    assert answer(R.I64, R.I32, R.NULL64) == 0 and answer(R.I32, R.I64, R.NULL32) == R.NULL32
    assert answer(R.I64, R.F64, R.NULL64) == -(2.0**63)
    assert answer(R.F64, R.I64, np.nan) == R.NULL64 and answer(R.F64, R.I64, 9.3e18) == R.NULL64 and answer(R.F64, R.I32, 2147483648.0) == R.NULL32
    assert answer(R.F64, R.I32, -2147483648.5) == R.NULL32 and answer(R.F64, R.I32, -2147483649.0) == R.NULL32
    assert answer(R.F64, R.I16, 32768.0) == -32768 and answer(R.F64, R.I16, 2147483648.0) == 0 and answer(R.F64, R.I16, np.nan) == 0
    assert answer(R.F64, R.U8, 300.7) == 44 and answer(R.F64, R.U8, -1.9) == 255 and answer(R.F64, R.U8, 256.0) == 0 and answer(R.F64, R.U8, np.nan) == 0
    assert answer(R.B8, R.I64, -1) == 255 and answer(R.B8, R.F64, -1) == 255.0  # the byte zero-extended


def test_headers_declare_the_cast_entry_points():
    text = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("rfx_hip.h", "rfx_exec.h", "rfx_ops.h")}
    for fn in ("rfx_hip_cast", "rfx_hip_cast_arm"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_hip.h"]), fn
    assert re.search(r"\brfx_exec_cast\s*\(", text["rfx_exec.h"])
    for fn in ("rfx_as", "rfx_last_cast_on_gpu"):
        assert re.search(rf"\b{fn}\s*\(", text["rfx_ops.h"]), fn
    # appended after the last id that existed, nothing renumbered
    assert re.search(r"RFX_XSTAT_ROWS_OUT = 35", text["rfx_exec.h"]) and re.search(r"RFX_XSTAT_CASTS = 36", text["rfx_exec.h"])


def test_lib_declares_the_cast_entry_points():
    from rayforce_amd import _lib as L
    from rayforce_amd import hostobj as H
    assert "rfx_hip_cast" in L.PROTOTYPES and "rfx_hip_cast_arm" in L.PROTOTYPES and "rfx_exec_cast" in L.EXEC_PROTOTYPES
    assert "rfx_as" in H.OPS_PROTOTYPES and "rfx_last_cast_on_gpu" in H.OPS_PROTOTYPES
    assert L.RFX_XSTAT_CASTS == 36 and L.RFX_CAST == {R.ATOM_NAME[t]: t for t in R.TYPES}


def test_the_arm_matrix_of_the_library_is_the_restatements(built):
    from rayforce_amd import hostobj as H
    ops = H.lib()
    for st in range(0, 13):
        for dt in range(0, 13):
            want = st != dt and R.has_arm(st, dt)
            assert bool(ops.rfx_hip_cast_arm(st, dt)) == want, (st, dt)
    assert ops.rfx_hip_cast_arm(R.I32 | 0x100, R.I64) and not ops.rfx_hip_cast_arm(R.I64 | 0x100, R.I32)  # (the widened image: a 4-byte source's alone)


def test_the_standalone_host_binds_as(built):
    import ctypes as C

    from rayforce_amd import hostobj as H
    ops = H.lib()
    f = ops.rfx_host_fn(b"as")
    assert f and H.header(f).type == 102  # a binary function object
    assert C.c_int64.from_address(H.payload(f) - 8).value == C.cast(ops.rfx_as, C.c_void_p).value  # the verb, not a stub
