"""The device sort of 1-, 2- and 4-byte keys on the GPU, all by equality of bits: the flat kernels against the numpy restatement
(tests/sort_narrow_ref.py) for every source class, every case of the reference's fixture (tests/golden/sort_narrow_golden.npz) through
rfx_iasc .. rfx_rank on the standalone host, mixed-width column chains through the planner, a DATE vector over three shards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sort_narrow_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError
from test_sort_narrow_cpu import GOLD, VERBS, cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# source class -> (numpy dtype of the cells, type code the flat ABI takes)
CLASSES = {"u8": (np.uint8, L.RFX_U8), "b8": (np.uint8, L.RFX_B8), "i16": (np.int16, L.RFX_I16), "i32": (np.int32, L.RFX_I32), "i32w": (np.int32, L.RFX_I32_WIDE)}
KINDS = ("full", "one_digit", "extremes", "equal")
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 100_003]  # (the small tile is 2048 rows)
BIG = 2**23 + 3  # the first size on the 8-rows-per-thread instantiation


def cells_of(rng, dtype, kind, n):
    info = np.iinfo(dtype)
    if kind == "full":
        return rng.integers(info.min, info.max + 1, n).astype(dtype)
    if kind == "one_digit":  # only the key's top byte varies
        top = 8 * (np.dtype(dtype).itemsize - 1)
        return ((rng.integers(0, 256, n) << top) + (7 if top else 0)).astype(np.dtype(dtype).str.replace("i", "u")).view(dtype)
    if kind == "extremes":
        return rng.choice(np.array([info.min, info.min + 1, info.max, 0, 1, info.max - 1], np.int64), n).astype(dtype)
    return np.full(n, 42, dtype)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def widened(eng, cells):
    """the image the operator layer's residency cache holds, made by the library itself"""
    d = to_dev(cells)
    wide = torch.empty(d.numel(), dtype=torch.int64, device=d.device)
    L.check(eng.lib.rfx_hip_widen_i32(eng._ctx, d.data_ptr(), d.numel(), wide.data_ptr()), "widen_i32")
    eng.sync()
    return wide


def sort_index(eng, col, code, desc, perm_in=None):
    n = col.numel()
    out = torch.empty(n, dtype=torch.int64, device=col.device)
    passes = C.c_int32(-1)
    L.check(eng.lib.rfx_hip_sort_index(eng._ctx, col.data_ptr(), code, n, int(desc), perm_in.data_ptr() if perm_in is not None else None, out.data_ptr(),
                                       C.byref(passes)), "sort_index")
    eng.sync()
    return out.cpu().numpy(), passes.value


def sort_values(eng, col, code, desc, dtype, n):
    out = torch.from_numpy(np.zeros(n + 16, dtype)).to(col.device)  # (16 cells of slack: nothing may be written past n cells of the column's width)
    perm = torch.empty(n, dtype=torch.int64, device=col.device)
    passes = C.c_int32(-1)
    L.check(eng.lib.rfx_hip_sort_values(eng._ctx, col.data_ptr(), code, n, int(desc), out.data_ptr(), perm.data_ptr(), C.byref(passes)), "sort_values")
    eng.sync()
    got = out.cpu().numpy()
    assert not got[n:].any()
    return got[:n], perm.cpu().numpy(), passes.value


def is_the_stable_order(keys, perm):
    """perm is a permutation, the keys are monotone along it and equal neighbours keep ascending rows: the ONE stable order, checked in O(n)"""
    n = len(keys)
    if perm.min() < 0 or perm.max() >= n or np.bincount(perm, minlength=n).max() != 1:
        return False
    k = keys[perm]
    return bool(np.all((k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (perm[1:] > perm[:-1]))))


def check_flat(eng, cls, kind, n):
    dtype, code = CLASSES[cls]
    rng = np.random.default_rng(n * 31 + len(kind) + len(cls))
    cells = cells_of(rng, dtype, kind, n)
    col = widened(eng, cells) if cls == "i32w" else to_dev(cells)
    pin = rng.permutation(n).astype(np.int64)
    dpin = to_dev(pin)
    inv_pin = np.empty(n, np.int64)
    inv_pin[pin] = np.arange(n)
    digits = R.varying_digits(cells)
    exact = n <= 100_003  # above: the same unique answer by its properties instead of a second argsort per call
    for desc in (False, True):
        tag = (cls, kind, n, desc)
        keys = R.key32(cells, desc)
        want = R.order(cells, desc)[0] if exact else None
        got, passes = sort_index(eng, col, code, desc)
        assert np.array_equal(got, want) if exact else is_the_stable_order(keys, got), tag
        assert passes == digits, (tag, passes, digits)
        # one level of a multi-column sort: the keys read through an incoming permutation
        got, passes = sort_index(eng, col, code, desc, dpin)
        if exact:
            assert np.array_equal(got, pin[R.order(cells[pin], desc)[0]]), (tag, "perm_in")
        else:
            assert got.min() >= 0 and got.max() < n and is_the_stable_order(keys[pin], inv_pin[got]), (tag, "perm_in")
        assert passes == digits, (tag, "perm_in", passes)
        # the sorted cells: the column's own width and bits, from the widened image too
        vals, perm, passes = sort_values(eng, col, code, desc, dtype, n)
        assert vals.dtype == dtype and passes == digits, tag
        assert np.array_equal(perm, want) if exact else is_the_stable_order(keys, perm), (tag, "values' permutation")
        assert vals.tobytes() == cells[perm].tobytes(), (tag, "values")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_flat_kernels_equal_the_restatement(eng, cls, kind, n):
    check_flat(eng, cls, kind, n)


@pytest.mark.parametrize("kind", KINDS)
def test_flat_kernels_on_the_large_tile(eng, kind):
    check_flat(eng, "i32", kind, BIG)


def test_a_misaligned_column_takes_the_cell_by_cell_loads(eng):
    """a column that does not start on 16 bytes (a slice of a tensor) sorts the same"""
    rng = np.random.default_rng(11)
    for cls in ("u8", "i16", "i32"):
        dtype, code = CLASSES[cls]
        cells = cells_of(rng, dtype, "full", 5000)
        col = to_dev(cells)[1:]
        assert col.data_ptr() % 16 != 0
        got, _ = sort_index(eng, col, code, False)
        assert np.array_equal(got, R.order(cells[1:])[0]), cls


def test_engine_sorts_narrow_tensors_in_their_dtype(eng):
    rng = np.random.default_rng(12)
    n = 70_001
    for a in (rng.integers(-(2**31), 2**31, n).astype(np.int32), rng.integers(-(2**15), 2**15, n).astype(np.int16), rng.integers(0, 256, n).astype(np.uint8),
              rng.integers(0, 2, n).astype(bool)):
        col = to_dev(a)
        cells = a.view(np.uint8) if a.dtype == bool else a
        for desc in (False, True):
            perm = R.order(cells, desc)[0]
            assert np.array_equal(eng.sort_index(col, descending=desc).cpu().numpy(), perm), (a.dtype, desc)
            vals = eng.sort_values(col, descending=desc)
            assert vals.dtype == col.dtype and np.array_equal(vals.cpu().numpy(), a[perm]), (a.dtype, desc)


def lex_order(cols, descending):
    """rows by cols[0] (most significant) .. cols[-1], stable, one direction for all; a column is narrow cells or ('f64' / 'i64', int64 bits)"""
    import sort_ref as R8
    keys = []
    for c in cols:
        if isinstance(c, tuple):
            k = R8.u(c[1], c[0] == "f64")
            keys.append(~k if descending else k)
        else:
            keys.append(R.key32(c, descending))
    return np.lexsort(keys[::-1]).astype(np.int64)


def test_mixed_widths_through_the_planner(eng):
    rng = np.random.default_rng(13)
    n = 200_003
    a32 = np.where(rng.random(n) < 0.1, R.NULL_I32, rng.integers(-20, 20, n)).astype(np.int32)
    b64 = rng.integers(-5, 5, n)
    f = (rng.integers(-3, 3, n) * 0.5)
    f[::50] = np.nan
    c16, d8 = rng.integers(-4, 4, n).astype(np.int16), rng.integers(0, 300, n).astype(np.uint8)
    for desc in (False, True):
        before = eng.xstat(L.RFX_XSTAT_SORTS)
        got = eng.sort_index([to_dev(a32), to_dev(b64)], descending=desc)
        assert eng.xstat(L.RFX_XSTAT_SORTS) - before == 2
        assert np.array_equal(got.cpu().numpy(), lex_order([a32, ("i64", b64)], desc)), desc
        got = eng.sort_index([to_dev(f), to_dev(c16), to_dev(d8)], descending=desc)
        assert np.array_equal(got.cpu().numpy(), lex_order([("f64", f.view(np.int64)), c16, d8], desc)), desc


def test_narrow_columns_over_shards_are_refused_with_their_reason():
    e = Engine(0, shards=2)
    try:
        col = torch.arange(1000, device="cuda:0", dtype=torch.int32)
        with pytest.raises(RfxError, match="do not sort over shards"):
            e.sort_index(col, over_shards=True)
        with pytest.raises(RfxError, match="do not sort over shards"):
            e.sort_values(col.to(torch.int16), over_shards=True)
        with pytest.raises(RfxError, match="sort over a sharded table"):  # (the default refusal stays)
            e.sort_index(col)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- the door
@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    o.rfx_host_bind()
    return o


def host_vector(ops, cells, t, attrs=0):
    o = ops.rfx_host_vector(t, cells.size)
    if cells.size:
        C.memmove(H.payload(o), np.ascontiguousarray(cells).ctypes.data, cells.nbytes)
    H.header(o).attrs = attrs
    return o


def raw_cells(o, dtype):
    h = H.header(o)
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (h.len * dt.itemsize)).from_address(H.payload(o)), dtype=dt).copy()


def test_fixture_vectors_through_the_operators(ops):
    gold = np.load(GOLD)
    for name, cells, t, attrs, ans in cases(gold):
        for verb in VERBS:
            want, wt, wa = ans[verb]
            tag = f"{name} {verb}"
            x = host_vector(ops, cells, t, attrs)
            r = getattr(ops, "rfx_" + verb)(x)
            if want is None:  # the reference answers an error: the door hands the call to the host (standalone: none behind it)
                assert H.is_error(r) and ops.rfx_last_sort_on_gpu() == 0 and "reverse has no I16 arm" in ops.rfx_ops_last_error().decode(), tag
                ops.rfx_host_drop(x)
                continue
            assert not H.is_error(r), (tag, H.error_text(r))
            assert H.header(r).type == wt and H.header(r).attrs == wa, (tag, H.header(r).type, H.header(r).attrs)
            got = raw_cells(r, cells.dtype if verb in ("asc", "desc") else np.int64)
            assert len(got) == len(want) and got.tobytes() == want.astype(got.dtype).tobytes(), tag
            assert ops.rfx_last_sort_on_gpu() == int(len(cells) > 0 and not attrs & 6), tag
            ops.rfx_host_drop(r)
            ops.rfx_host_drop(x)


def test_a_b8_device_column_handle_sorts_as_its_bytes(ops, eng):
    rng = np.random.default_rng(14)
    cells = rng.choice(np.array([0, 1, 2, 255], np.uint8), 5000)
    dev = to_dev(cells.view(np.int8))
    x = H.device_vector(dev)
    r = ops.rfx_iasc(x)
    assert not H.is_error(r), H.error_text(r)
    assert ops.rfx_last_sort_on_gpu() == 1 and np.array_equal(raw_cells(r, np.int64), R.order(cells)[0])
    r = ops.rfx_desc(x)
    assert not H.is_error(r), H.error_text(r)
    assert H.header(r).type == R.T_B8 and H.header(r).attrs == R.ATTR_DESC and np.array_equal(raw_cells(r, np.uint8), R.values(cells, True)[0])
    c8 = host_vector(ops, cells, 12)  # C8 stays the host's: it is a string
    r2 = ops.rfx_asc(c8)
    assert H.is_error(r2) and ops.rfx_last_sort_on_gpu() == 0 and "key type" in ops.rfx_ops_last_error().decode()


_SHARDED_DOOR = r'''
import sys
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import numpy as np
import sort_narrow_ref as R
import test_sort_narrow_gpu as T
from rayforce_amd import hostobj as H
ops = H.lib()
assert ops.rfx_host_bind() == 0
date = T.sharded_date_cells()
for verb, dtype in (("iasc", np.int64), ("desc", np.int32), ("rank", np.int64)):
    x = T.host_vector(ops, date, R.T_DATE)
    r = getattr(ops, "rfx_" + verb)(x)
    assert not H.is_error(r), (verb, H.error_text(r))
    assert ops.rfx_ops_shards() == SHARDS and ops.rfx_last_sort_on_gpu() == 1, verb
    want, attrs = R.restated(verb, date)
    assert H.header(r).type == (R.T_DATE if verb == "desc" else R.T_I64) and H.header(r).attrs == attrs, verb
    assert T.raw_cells(r, dtype).tobytes() == want.astype(dtype).tobytes(), verb
    ops.rfx_host_drop(r)
    ops.rfx_host_drop(x)
x = T.host_vector(ops, np.arange(100, dtype=np.int16), R.T_I16)
r = ops.rfx_iasc(x)
assert H.is_error(r) and ops.rfx_last_sort_on_gpu() == 0
assert "1- and 2-byte keys over shards" in ops.rfx_ops_last_error().decode(), ops.rfx_ops_last_error()
print("SORT-NARROW-DOOR-OK", SHARDS)
'''


def sharded_date_cells():
    rng = np.random.default_rng(15)
    n = 20_011
    return np.where(rng.random(n) < 0.1, R.NULL_I32, rng.integers(-30, 30, n)).astype(np.int32)


def test_a_date_vector_over_three_shards_through_the_door(ops):
    """RFX_SHARDS=3 in a process of its own (the operator layer's shards are fixed at its first call): iasc / desc / rank equal the restatement bit for
    bit there, as the unsharded answers do here; an I16 vector is refused with its reason"""
    date = sharded_date_cells()
    for verb, dtype in (("iasc", np.int64), ("desc", np.int32), ("rank", np.int64)):
        x = host_vector(ops, date, R.T_DATE)
        r = getattr(ops, "rfx_" + verb)(x)
        assert not H.is_error(r) and raw_cells(r, dtype).tobytes() == R.restated(verb, date)[0].astype(dtype).tobytes(), verb
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(x)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RFX_SHARDS="3")
    code = f"ROOT = {ROOT!r}\nSHARDS = 3\n" + _SHARDED_DOOR
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "SORT-NARROW-DOOR-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
