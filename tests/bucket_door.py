"""Helpers of the bucket verbs' GPU tests: a golden case (tests/bucket_ref.py load_cases) through the C operator door over standalone host objects,
and through the Engine over device tensors.  Also imported by the child processes of the sharded runs."""
import ctypes as C

import numpy as np

import bucket_ref as B
from rayforce_amd import hostobj as H

KIND = {4: "i32", 5: "i64", 7: "date", 8: "time", 9: "timestamp", 10: "f64"}


def host_vector(ops, cells, tp, attrs=0):
    cells = np.ascontiguousarray(cells)
    o = ops.rfx_host_vector(tp, cells.size)
    if cells.size:
        C.memmove(H.payload(o), cells.ctypes.data, cells.nbytes)
    H.header(o).attrs = attrs
    return o


def host_atom(ops, cell, tp):
    """an atom of type -tp: the standalone host's i64 / f64 atom retyped (the narrower integers share the union's low bytes)"""
    o = ops.rfx_host_f64(float(cell)) if tp == B.F64 else ops.rfx_host_i64(int(cell))
    H.header(o).type = -tp
    return o


def result_cells(o):
    h = H.header(o)
    dt = np.dtype(B.DTYPE[h.type])
    return np.frombuffer((C.c_char * (h.len * dt.itemsize)).from_address(H.payload(o)), dtype=dt).copy() if h.len else np.empty(0, dt)


def door(ops, c):
    """-> (result object, [objects to drop])"""
    x = host_atom(ops, c["x"][0], c["xt"]) if c["xa"] else host_vector(ops, c["x"], c["xt"], c["attrs"])
    if c["y"] is None:
        return getattr(ops, "rfx_" + c["verb"])(x), [x]
    y = host_atom(ops, c["y"][0], c["yt"]) if c["ya"] else host_vector(ops, c["y"], c["yt"])
    return getattr(ops, "rfx_" + c["verb"])(x, y), [x, y]


def check_door(ops, c):
    r, drop = door(ops, c)
    assert r and not H.is_error(r), (c["name"], H.error_text(r) if r else "null")
    assert ops.rfx_last_bucket_on_gpu() == 1, c["name"]
    assert H.header(r).type == c["ot"], (c["name"], H.header(r).type, c["ot"])
    got, want = B.as_bits(result_cells(r)), B.as_bits(c["out"])
    assert got.shape == want.shape, (c["name"], got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (c["name"], bad[:5], got[bad[:5]], want[bad[:5]])
    for o in [r] + drop:
        ops.rfx_host_drop(o)


def engine_answer(eng, c):
    import torch

    def dev(a):
        return torch.from_numpy(np.array(a)).to(eng.device)

    v = c["verb"]
    if v == "xrank":
        return eng.xrank(dev(c["x"]), int(c["y"][0]), {0: None, 2: "asc", 4: "desc"}[c["attrs"]])
    if v == "xbar":
        def operand(a, tp, atom):
            if not atom:
                return dev(a)
            return float(a[0]) if tp == B.F64 else int(a[0])
        return eng.xbar(operand(c["x"], c["xt"], c["xa"]), operand(c["y"], c["yt"], c["ya"]), KIND[c["xt"]], KIND[c["yt"]])
    if v == "within":
        return eng.within(dev(c["x"]), int(c["y"][0]), int(c["y"][1]))
    return getattr(eng, v)(dev(c["x"]))


def check_engine(eng, c):
    got = B.as_bits(engine_answer(eng, c).cpu().numpy())
    want = B.as_bits(c["out"])
    assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (c["name"], got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want.view(got.dtype))
    assert bad.size == 0, (c["name"], bad[:5], got[bad[:5]], want[bad[:5]])
