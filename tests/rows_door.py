"""Helpers of the row verbs' GPU tests: a golden case (tests/rows_ref.py load_cases) through the C operator door over standalone host objects, and
through the Engine over device tensors.  Also imported by the child processes of the sharded runs."""
import ctypes as C

import numpy as np

import rows_ref as R
from rayforce_amd import hostobj as H


def host_vector(ops, cells, tp, attrs=0):
    """a host vector of type code tp (any code: the door decides on the code before it reads a cell)"""
    cells = np.ascontiguousarray(cells)
    o = ops.rfx_host_vector(tp if tp in R.DTYPE else R.I64, cells.size)
    if cells.size:
        C.memmove(H.payload(o), cells.ctypes.data, cells.nbytes)
    H.header(o).type = tp
    H.header(o).attrs = attrs
    return o


def host_atom(ops, cell, tp):
    o = ops.rfx_host_f64(float(cell)) if tp == R.F64 else ops.rfx_host_i64(int(cell))
    H.header(o).type = -tp
    return o


def cells_of(o):
    h = H.header(o)
    dt = np.dtype(R.DTYPE[h.type])
    return np.frombuffer((C.c_char * (h.len * dt.itemsize)).from_address(H.payload(o)), dtype=dt).copy() if h.len else np.empty(0, dt)


def operands(ops, c):
    """-> (x, y or None)"""
    if c["atom"]:
        tp, _a, cells = c["cols"][0]
        x = host_atom(ops, cells[0], tp)
    else:
        vecs = []
        for j, (tp, attrs, cells) in enumerate(c["cols"]):
            vecs.append(ops.rfx_host_clone(vecs[c["alias"][j]]) if c["alias"][j] >= 0 else host_vector(ops, cells, tp, attrs))
        x = ops.rfx_host_table(H.symbols(c["names"]), H.list_of(vecs)) if c["table"] else vecs[0]
    if c["verb"] == "filter":
        m = c["mask"]
        return x, host_vector(ops, m, R.I64 if m.dtype == np.int64 else R.B8)
    if c["verb"] == "take":
        kind, a, b = c["count"]
        return x, host_vector(ops, np.array([a, b], np.int64), R.I64) if kind == "range" else host_atom(ops, b, a)
    return x, None


def call(ops, c):
    x, y = operands(ops, c)
    return (ops.rfx_reverse(x) if y is None else getattr(ops, "rfx_" + c["verb"])(x, y)), [o for o in (x, y) if o]


def same_column(name, got_tp, got_attrs, got, want):
    wt, wa, wc = want
    assert (got_tp, got_attrs) == (wt, wa), (name, got_tp, got_attrs, wt, wa)
    g, w = R.as_bits(got), R.as_bits(wc)
    assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (name, bad[:5], g[bad[:5]], w[bad[:5]])


def check_door(ops, c, retype=None):
    """retype = (from, to): the same cells under another 8-byte type code (SYMBOL: the fixture cannot carry it)"""
    if retype:
        swap = lambda cols: [((retype[1] if tp == retype[0] else tp), a, cells) for tp, a, cells in cols]  # noqa: E731
        c = dict(c, cols=swap(c["cols"]), out=swap(c["out"]))
    r, drop = call(ops, c)
    assert r and not H.is_error(r), (c["name"], H.error_text(r) if r else "null")
    assert ops.rfx_last_rows_on_gpu() == 1, c["name"]
    if c["table"]:
        assert H.header(r).type == H.T_TABLE, c["name"]
        keys, vals = H.list_items(r)
        assert [ops.rfx_host_symbol_name(int(i)).decode() for i in H.to_numpy(keys)] == c["names"], c["name"]
        cols = H.list_items(vals)
    else:
        cols = [r]
    assert len(cols) == len(c["out"]), c["name"]
    for o, want in zip(cols, c["out"]):
        same_column(c["name"], H.header(o).type, H.header(o).attrs, cells_of(o), want)
    for o in [r] + drop:
        ops.rfx_host_drop(o)


def check_refused(ops, c):
    r, drop = call(ops, c)
    assert r and H.is_error(r), c["name"]
    assert ops.rfx_last_rows_on_gpu() == 0, c["name"]
    assert c["host"] in ops.rfx_ops_last_error().decode(), (c["name"], c["host"], ops.rfx_ops_last_error().decode())
    assert "no host function" in H.error_text(r), c["name"]
    ops.rfx_host_drop(r)


def engine_answer(eng, c, form=None):
    import torch

    def dev(a):
        return torch.from_numpy(np.array(a)).to(eng.device)

    cols = {f"c{j}": dev(cells) for j, (_tp, _a, cells) in enumerate(c["cols"])}
    x = cols if c["table"] else cols["c0"]
    if c["verb"] == "filter":
        got = eng.filter(x, dev(c["mask"].view(np.int8)), form=form)
    elif c["verb"] == "reverse":
        got = eng.reverse(x)
    else:
        kind, a, b = c["count"]
        count = (a, b) if kind == "range" else b
        if c["atom"]:
            cell = c["cols"][0][2][0]
            got = eng.take(float(cell) if c["cols"][0][0] == R.F64 else int(cell), count, dtype=cols["c0"].dtype)
        else:
            got = eng.take(x, count)
    return list(got.values()) if c["table"] else [got]


def check_engine(eng, c, form=None):
    got = engine_answer(eng, c, form)
    assert len(got) == len(c["out"]), c["name"]
    for g, (wt, _wa, wc) in zip(got, c["out"]):
        g = g.cpu().numpy()
        gb, wb = R.as_bits(g), R.as_bits(wc)
        assert gb.dtype == wb.dtype and gb.shape == wb.shape, (c["name"], gb.dtype, wb.dtype, gb.shape, wb.shape)
        bad = np.flatnonzero(gb != wb)
        assert bad.size == 0, (c["name"], form, bad[:5], gb[bad[:5]], wb[bad[:5]])
