"""Helpers of the cast's GPU tests: a golden case (tests/cast_ref.py load_cases) through the C operator door over standalone host objects, and through the
Engine over device tensors.  Also imported by the child processes of the sharded runs."""
import ctypes as C

import numpy as np

import cast_ref as R
from rayforce_amd import hostobj as H


def host_vector(ops, cells, tp, attrs=0):
    cells = np.ascontiguousarray(cells, dtype=R.DTYPE[tp])
    o = ops.rfx_host_vector(tp, cells.size)
    if cells.size:
        C.memmove(H.payload(o), cells.ctypes.data, cells.nbytes)
    H.header(o).attrs = attrs
    return o


def result_cells(o):
    h = H.header(o)
    dt = np.dtype(R.DTYPE[h.type])
    return np.frombuffer((C.c_char * (h.len * dt.itemsize)).from_address(H.payload(o)), dtype=dt).copy() if h.len else np.empty(0, dt)


def same_bits(name, got, want):
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    got, want = R.as_bits(got), R.as_bits(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])


def door(ops, type_name, x):
    t = ops.rfx_host_symbol(type_name.encode())
    r = ops.rfx_as(t, x)
    ops.rfx_host_drop(t)
    return r


def check_answer(ops, c, r, x):
    """r = (as 'name x) by the door: the golden case's type code, attribute byte and cells"""
    assert r and not H.is_error(r), (c["name"], H.error_text(r) if r else "null")
    assert ops.rfx_last_cast_on_gpu() == 1, c["name"]
    h = H.header(r)
    assert (h.type, h.attrs, h.len) == (c["ot"], c["oattrs"], c["n"]), (c["name"], h.type, h.attrs, h.len)
    if c["st"] == c["dt"]:
        assert r == x, c["name"]  # clone_obj: the argument itself, one reference more
    same_bits(c["name"], result_cells(r), c["out"])


def check_door(ops, c):
    x = host_vector(ops, c["x"], c["st"], c["attrs"])
    r = door(ops, c["type_name"], x)
    check_answer(ops, c, r, x)
    ops.rfx_host_drop(r)
    ops.rfx_host_drop(x)


def check_engine(eng, c):
    import torch
    x = torch.from_numpy(np.array(c["x"])).to(eng.device)
    got = eng.cast(x, R.ATOM_NAME[c["dt"]], R.ATOM_NAME[c["st"]])
    if c["st"] == c["dt"]:
        assert got is x, c["name"]
    assert got.dtype == eng._CAST_DTYPE[c["dt"]], (c["name"], got.dtype)
    same_bits(c["name"], got.cpu().numpy(), c["out"])
