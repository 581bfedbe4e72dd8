"""Helpers of the concat / raze tests: a golden case (tests/concat_ref.py load_cases) through the C operator door over standalone host objects and through
the Engine over device tensors, and the `host_` shapes as objects.  Also imported by the child processes of the residency and sharded runs."""
import ctypes as C

import numpy as np

import concat_ref as R
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


def host_atom(ops, bits, tp):
    """an atom of type code tp whose cell is the low bytes of `bits`"""
    o = ops.rfx_host_i64(int(np.array([bits], np.uint64).view(np.int64)[0]))
    H.header(o).type = -tp
    return o


def cells_of(o):
    h = H.header(o)
    dt = np.dtype(R.DTYPE[h.type])
    return np.frombuffer((C.c_char * (h.len * dt.itemsize)).from_address(H.payload(o)), dtype=dt).copy() if h.len else np.empty(0, dt)


def part_obj(ops, part, tp):
    return host_atom(ops, part["atom"], tp) if isinstance(part, dict) else host_vector(ops, part, tp)


def call(ops, c):
    """-> (the answer, the operands to drop)"""
    cols = [[part_obj(ops, p, tp) for p in parts] for tp, parts in c["cols"]]
    if c["verb"] == "raze":
        lst = H.list_of(cols[0])
        return ops.rfx_raze(lst), [lst]
    if c["verb"] == "concat":
        return ops.rfx_concat(cols[0][0], cols[0][1]), cols[0]
    order = [c["names"].index(nm) for nm in c["ynames"]]
    x = ops.rfx_host_table(H.symbols(c["names"]), H.list_of([col[0] for col in cols]))
    y = ops.rfx_host_table(H.symbols(c["ynames"]), H.list_of([cols[k][1] for k in order]))
    return ops.rfx_concat(x, y), [x, y]


def same_column(name, got_tp, got_attrs, got, want):
    wt, wa, wc = want
    assert (got_tp, got_attrs) == (wt, wa), (name, got_tp, got_attrs, wt, wa)
    g, w = R.as_bits(got), R.as_bits(wc)
    assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (name, bad[:5], g[bad[:5]], w[bad[:5]])


def check_door(ops, c):
    r, drop = call(ops, c)
    assert r and not H.is_error(r), (c["name"], H.error_text(r) if r else "null")
    assert ops.rfx_last_concat_on_gpu() == 1, c["name"]
    if c["verb"] == "table":
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


def host_operands(ops, shape):
    """a `host_` case's operands -> (x, y or None)"""
    i64 = lambda n=5: host_vector(ops, np.arange(n, dtype=np.int64), R.I64)  # noqa: E731
    f64 = lambda n=5: host_vector(ops, np.arange(n, dtype=np.float64), R.F64)  # noqa: E731
    coded = lambda code: host_vector(ops, np.arange(4, dtype=np.int64), code)  # noqa: E731
    tab = lambda names, cols: ops.rfx_host_table(H.symbols(names), H.list_of(cols))  # noqa: E731
    fake = (C.c_void_p * 1)(4096)  # (a device address nobody reads: the door refuses by the type code)
    device = lambda tp: ops.rfx_host_device_vector(tp, 8, fake, 1)  # noqa: E731
    return {
        "atom_atom": lambda: (host_atom(ops, 1, R.I64), host_atom(ops, 2, R.I64)),
        "types_differ": lambda: (i64(), f64()),
        "vector_atom_types_differ": lambda: (i64(), host_atom(ops, 0, R.F64)),
        "c8": lambda: (coded(R.C8), coded(R.C8)),
        "guid": lambda: (coded(R.GUID), coded(R.GUID)),
        "enum": lambda: (coded(R.ENUM), coded(R.ENUM)),
        "maplist": lambda: (coded(R.MAPLIST), coded(R.MAPLIST)),
        "list": lambda: (H.list_of([i64()]), i64()),
        "dict": lambda: (ops.rfx_host_dict(H.symbols(["a"]), H.list_of([i64()])), ops.rfx_host_dict(H.symbols(["a"]), H.list_of([i64()]))),
        "parted": lambda: (coded(77 + R.I64), coded(77 + R.I64)),
        "table_vector": lambda: (tab(["a"], [i64()]), i64()),
        "names_differ": lambda: (tab(["a", "b"], [i64(), f64()]), tab(["a", "c"], [i64(), f64()])),
        "names_extra": lambda: (tab(["a"], [i64()]), tab(["a", "b"], [i64(), f64()])),
        "col_types_differ": lambda: (tab(["a"], [i64()]), tab(["a"], [f64()])),
        "table_c8_column": lambda: (tab(["a"], [coded(R.C8)]), tab(["a"], [coded(R.C8)])),
        "table_parted": lambda: (tab(["a"], [coded(77 + R.I64)]), tab(["a"], [coded(77 + R.I64)])),
        "raze_not_list": lambda: (i64(), None),
        "raze_empty_list": lambda: (H.list_of([]), None),
        "raze_mixed_types": lambda: (H.list_of([i64(), f64()]), None),
        "raze_atom_element": lambda: (H.list_of([host_atom(ops, 1, R.I64)]), None),
        "raze_list_element": lambda: (H.list_of([H.list_of([i64()]), H.list_of([i64()])]), None),
        "raze_c8": lambda: (H.list_of([coded(R.C8), coded(R.C8)]), None),
        "device_i32": lambda: (device(R.I32), host_vector(ops, np.arange(3, dtype=np.int32), R.I32)),
        "device_i16": lambda: (host_vector(ops, np.arange(3, dtype=np.int16), R.I16), device(R.I16)),
        "device_u8": lambda: (device(R.U8), device(R.U8)),
    }[shape]()


def check_refused(ops, c):
    """the shape is handed to the host -- there is none behind the standalone door: an error naming the reason (the operands are left alone: some carry
    type codes the standalone host could not drop)"""
    x, y = host_operands(ops, c["shape"])
    r = ops.rfx_raze(x) if c["verb"] == "raze" else ops.rfx_concat(x, y)
    assert r and H.is_error(r), c["name"]
    assert ops.rfx_last_concat_on_gpu() == 0, c["name"]
    assert c["host"] in ops.rfx_ops_last_error().decode(), (c["name"], c["host"], ops.rfx_ops_last_error().decode())
    assert "no host function" in H.error_text(r), c["name"]
    ops.rfx_host_drop(r)


TORCH_OF = {R.B8: "int8", R.U8: "uint8", R.I16: "int16", R.I32: "int32", R.DATE: "int32", R.TIME: "int32", R.I64: "int64", R.SYMBOL: "int64", R.TS: "int64",
            R.F64: "float64"}


def engine_answer(eng, c):
    import struct

    import torch

    def part(p, tp):
        if isinstance(p, dict):  # the atom as the Python number Engine.concat takes
            raw = int(p["atom"]).to_bytes(8, "little")[:np.dtype(R.DTYPE[tp]).itemsize]
            return struct.unpack({np.int8: "<b", np.uint8: "<B", np.int16: "<h", np.int32: "<i", np.int64: "<q", np.float64: "<d"}[R.DTYPE[tp]], raw)[0]
        return torch.from_numpy(np.array(p)).to(eng.device)

    cols = [[part(p, tp) for p in parts] for tp, parts in c["cols"]]
    if c["verb"] == "raze":
        return [eng.raze(cols[0])]
    if c["verb"] == "concat":
        return [eng.concat(cols[0][0], cols[0][1])]
    got = eng.concat({nm: cols[k][0] for k, nm in enumerate(c["names"])}, {nm: cols[c["names"].index(nm)][1] for nm in c["ynames"]})
    assert list(got) == c["names"], c["name"]
    return list(got.values())


def check_engine(eng, c):
    got = engine_answer(eng, c)
    assert len(got) == len(c["out"]), c["name"]
    for g, (wt, _wa, wc) in zip(got, c["out"]):
        assert str(g.dtype) == "torch." + TORCH_OF[wt], (c["name"], g.dtype, wt)
        gb, wb = R.as_bits(g.cpu().numpy()), R.as_bits(wc)
        assert gb.dtype == wb.dtype and gb.shape == wb.shape, (c["name"], gb.dtype, wb.dtype, gb.shape, wb.shape)
        bad = np.flatnonzero(gb != wb)
        assert bad.size == 0, (c["name"], bad[:5], gb[bad[:5]], wb[bad[:5]])
