"""`as` over vectors on the GPU by equality of bits: every case of the reference's fixture (tests/golden/cast_golden.npz; its lengths, cast_ref.LENS, lie
around a lane's run of 4 / 8 / 16 cells, the 64-lane wave and the 256-lane block of rfx_cast.hip) through the Engine over device tensors and through the C
door over host vectors, type code and attribute byte included; the same cases over 2 and 3 shards; device-column handles; the same type and the empty
vector; the shapes handed back with their recorded reasons; and 2^20 + 5 rows per source cell class against the restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cast_door as D
import cast_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.load_cases()
SHARDED_LENS = (1, 5, 1025, 4097)


@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    assert o.rfx_host_bind() == 0  # standalone host: nothing behind the door to hand a shape to
    return o


@pytest.mark.parametrize("st", R.TYPES)
def test_fixture_through_the_engine(eng, st):
    before = eng.xstat(L.RFX_XSTAT_CASTS)
    ran = 0
    for c in CASES:
        if c["st"] == st and not c["host"] and c["spelling"] == "vector":  # (the Engine names types one way)
            D.check_engine(eng, c)
            ran += c["n"] > 0 and c["st"] != c["dt"]
    assert ran and eng.xstat(L.RFX_XSTAT_CASTS) - before == ran  # every converting case ran the kernel; the same type and the empty column ran nothing


@pytest.mark.parametrize("st", R.TYPES)
def test_fixture_through_the_door(ops, st):
    ran = 0
    for c in CASES:
        if c["st"] == st and not c["host"]:
            D.check_door(ops, c)
            ran += 1
    assert ran


def test_the_same_type_is_the_argument_with_its_attributes(ops):
    for tp in R.TYPES:
        for attrs in (0, 2, 5):
            x = D.host_vector(ops, np.arange(17) % 2, tp, attrs)
            for name in (R.VECTOR_NAME[tp], R.ATOM_NAME[tp]):
                r = D.door(ops, name, x)
                assert r == x and H.header(r).attrs == attrs and H.header(r).type == tp and ops.rfx_last_cast_on_gpu() == 1, (tp, attrs, name)
                ops.rfx_host_drop(r)
            ops.rfx_host_drop(x)


def test_every_empty_vector_answers_an_empty_vector_of_the_target_type(ops, eng):
    for st in R.TYPES:
        x = D.host_vector(ops, np.empty(0), st, 2)
        for dt in R.TYPES:  # (B8 <-> U8 too: the reference answers an empty vector before it looks at its arms)
            if dt != st:
                r = D.door(ops, R.VECTOR_NAME[dt], x)
                h = H.header(r)
                assert not H.is_error(r) and (h.type, h.len, h.attrs) == (dt, 0, 0) and ops.rfx_last_cast_on_gpu() == 1, (st, dt)
                ops.rfx_host_drop(r)
                got = eng.cast(torch.empty(0, dtype=eng._CAST_DTYPE[st], device=eng.device), R.ATOM_NAME[dt], R.ATOM_NAME[st])
                assert got.numel() == 0 and got.dtype == eng._CAST_DTYPE[dt]
        ops.rfx_host_drop(x)


def test_device_column_handles_go_in(ops):
    n = 4097
    i64 = next(c for c in CASES if c["st"] == R.I64 and c["dt"] == R.I16 and c["n"] == n and c["spelling"] == "vector")
    b8 = next(c for c in CASES if c["st"] == R.B8 and c["dt"] == R.F64 and c["n"] == n and c["spelling"] == "atom")
    ts = next(c for c in CASES if c["st"] == R.TS and c["dt"] == R.U8 and c["n"] == n and c["spelling"] == "vector")
    f64 = next(c for c in CASES if c["st"] == R.F64 and c["dt"] == R.DATE and c["n"] == n and c["spelling"] == "vector")
    for c in (i64, b8, ts, f64):
        cells = torch.from_numpy(np.array(c["x"])).cuda()
        x = ops.rfx_host_device_vector(c["st"], n, (C.c_void_p * 1)(cells.data_ptr()), 1)
        torch.cuda.synchronize()
        r = D.door(ops, c["type_name"], x)
        D.check_answer(ops, c, r, x)
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(x)


def refused(ops, r, reason):
    assert r and H.is_error(r), reason
    assert ops.rfx_last_cast_on_gpu() == 0, reason
    assert ops.rfx_ops_last_error().decode() == f"as: not covered by the MI355X path ({reason}) and no host function to delegate to", ops.rfx_ops_last_error()
    assert H.error_text(r) == ops.rfx_ops_last_error().decode()
    ops.rfx_host_drop(r)


def test_every_host_case_is_an_error_naming_the_recorded_reason(ops):
    hosts = [c for c in CASES if c["host"]]
    assert len(hosts) >= 6
    for c in hosts:
        x = D.host_vector(ops, c["x"], c["st"])
        refused(ops, D.door(ops, c["type_name"], x), c["host"])
        ops.rfx_host_drop(x)


def test_shapes_outside_the_device_path_are_handed_back(ops):
    i64v = D.host_vector(ops, np.arange(10), R.I64)
    name = ops.rfx_host_symbol(b"F64")
    refused(ops, ops.rfx_as(ops.rfx_host_i64(7), i64v), "the type name is not a symbol atom")
    refused(ops, ops.rfx_as(name, ops.rfx_host_i64(7)), "an atom")
    for code in (0, 6, 11, 12):  # LIST, SYMBOL, GUID, C8
        v = D.host_vector(ops, np.arange(10), R.I64)
        H.header(v).type = code
        refused(ops, ops.rfx_as(name, v), "not a vector of the nine numeric and temporal types")
        H.header(v).type = R.I64
    refused(ops, ops.rfx_as(name, H.table({"a": np.arange(3)})), "not a vector of the nine numeric and temporal types")
    refused(ops, D.door(ops, "SYMBOL", i64v), "a type name outside the nine numeric and temporal types")
    cells = torch.arange(16, dtype=torch.int64, device="cuda")  # behind the handles below (the door refuses them before it reads a cell)
    for tp in (R.I32, R.DATE, R.I16, R.U8):
        refused(ops, ops.rfx_as(name, ops.rfx_host_device_vector(tp, 10, (C.c_void_p * 1)(cells.data_ptr()), 1)), "a device column that is not I64 / F64 / TIMESTAMP / B8")
    # ... and a device shape right after answers again
    r = ops.rfx_as(name, i64v)
    assert not H.is_error(r) and ops.rfx_last_cast_on_gpu() == 1 and D.result_cells(r).tolist() == [float(i) for i in range(10)]


def test_engine_refuses_what_the_reference_has_no_arm_for(eng):
    with pytest.raises(RfxError, match="no cast from type 1 to type 2"):
        eng.cast(torch.ones(5, dtype=torch.int8, device=eng.device), "u8")
    with pytest.raises(RfxError, match="names none"):
        eng.cast(torch.ones(5, dtype=torch.int64, device=eng.device), "symbol")
    with pytest.raises(RfxError, match="cannot be"):
        eng.cast(torch.ones(5, dtype=torch.int64, device=eng.device), "f64", "date")
    with pytest.raises(RfxError, match="cannot be"):
        eng.cast(torch.ones(5, dtype=torch.float32, device=eng.device), "f64")
    odd = torch.arange(33, dtype=torch.int64, device=eng.device)[1:]  # a view that starts 8 bytes into its allocation
    assert torch.equal(eng.cast(odd, "f64"), odd.to(torch.float64))


BIG_ARMS = ((R.U8, R.I64), (R.B8, R.I16), (R.I16, R.F64), (R.I32, R.U8), (R.TIME, R.TS), (R.I64, R.I16), (R.I64, R.F64), (R.F64, R.I32), (R.F64, R.U8), (R.F64, R.TS))


def big_cells(st):
    rng = np.random.default_rng(st)
    if st == R.F64:
        x = rng.standard_normal(R.BIG) * 10.0 ** rng.integers(-2, 20, R.BIG)
        x[::1001] = np.nan
        x[1::1001] = np.inf
        return x
    info = np.iinfo(R.DTYPE[st])
    return rng.integers(info.min, info.max, R.BIG, dtype=R.DTYPE[st], endpoint=True)


@pytest.mark.parametrize("st,dt", BIG_ARMS)
def test_a_long_column_against_the_restatement(eng, ops, st, dt):
    x = big_cells(st)
    want = R.cast(x, st, dt)
    got = eng.cast(torch.from_numpy(x).to(eng.device), R.ATOM_NAME[dt], R.ATOM_NAME[st])
    D.same_bits((st, dt), got.cpu().numpy(), want)
    D.check_door(ops, dict(name=f"big_{st}_{dt}", st=st, dt=dt, type_name=R.VECTOR_NAME[dt], x=x, attrs=0, out=want, ot=dt, oattrs=0, n=R.BIG))


@pytest.mark.parametrize("shards", [2, 3])
def test_fixture_over_shards_through_the_engine(built, shards):
    e = Engine(0, shards=shards)
    try:
        ran = 0
        for c in CASES:
            if not c["host"] and c["n"] in SHARDED_LENS and c["spelling"] == "vector":
                D.check_engine(e, c)
                ran += 1
        assert ran > 250, ran
    finally:
        e.close()


_SHARDED_DOOR = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import cast_door as D
import cast_ref as R
from rayforce_amd import hostobj as H
ops = H.lib()
assert ops.rfx_host_bind() == 0
ran = 0
for c in R.load_cases():
    if not c["host"] and c["n"] in LENS:
        D.check_door(ops, c)
        ran += 1
assert ops.rfx_ops_shards() == SHARDS and ran > 500, (ops.rfx_ops_shards(), ran)
print("CAST-DOOR-OK", ran)
'''


@pytest.mark.parametrize("shards", [2, 3])
def test_fixture_over_shards_through_the_door(built, shards):
    """RFX_SHARDS=k in a process of its own (the operator layer's shards are fixed at its first call): 1025 and 4097 rows split mid-vector"""
    env = dict(os.environ, RFX_SHARDS=str(shards), HSA_ENABLE_IPC_MODE_LEGACY="0")
    code = f"ROOT = {ROOT!r}\nSHARDS = {shards}\nLENS = {SHARDED_LENS!r}\n" + _SHARDED_DOOR
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CAST-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
