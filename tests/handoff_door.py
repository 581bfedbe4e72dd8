"""Helpers of tests/test_handoff_cpu.py and tests/golden/make_handoff_golden.py: what the operator door decides BEFORE it touches a device, recorded over the
standalone host object model.  A case names a verb and describes its arguments as plain data; `run_case` rebuilds them, calls the verb and describes the
answer -- an error object's text or the result's type code, attribute byte, length and cells -- with rfx_ops_last_error(), the family's
rfx_last_*_on_gpu() and the family's own counters.  Nothing here computes anything.

Argument descriptions:
    None                                        a NULL pointer
    {"vec": type, "cells": [...], "attrs": a}   a vector of the type code (cells as integers, floats for F64)
    {"atom": type, "v": value}                  an atom of the type code (given positive)
    {"sym": name, "attrs": a}                   a symbol atom
    {"syms": [names]}                           a SYMBOL vector
    {"list": [descriptions], "type": t}         a LIST (or, with "type", the same payload under another type code: a parted column, a MAPFILTER pair)
    {"table": [[name, description], ...]}       a table
    {"dict": [keys description, values description]}
    {"fn": name}                                the function object rfx_host_fn(name) answers
    {"device": type, "len": n}                  a device column handle (its address is never read before the device is)"""
import ctypes as C
import os
import re

import numpy as np

from rayforce_amd import hostobj as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPE = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 6: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}
T_LIST, T_SYMBOL, T_F64, T_TABLE, T_DICT, T_ERR = 0, 6, 10, 98, 99, 127
# verb -> (entry point, arity: 1, 2 or "n", the family's last-on-GPU accessor)
VERBS = {
    **{v: ("rfx_" + v, 1, "rfx_last_sort_on_gpu") for v in ("iasc", "idesc", "asc", "desc", "rank")},
    **{v: ("rfx_" + v, 2, "rfx_last_sort_on_gpu") for v in ("xasc", "xdesc")},
    "asof_join": ("rfx_asof_join", "n", "rfx_last_asof_on_gpu"), "bin": ("rfx_bin", 2, "rfx_last_asof_on_gpu"), "binr": ("rfx_binr", 2, "rfx_last_asof_on_gpu"),
    "window_join": ("rfx_window_join", "n", "rfx_last_window_on_gpu"), "window_join1": ("rfx_window_join1", "n", "rfx_last_window_on_gpu"),
    "distinct": ("rfx_distinct", 1, "rfx_last_set_on_gpu"),
    **{v: ("rfx_" + v, 2, "rfx_last_set_on_gpu") for v in ("find", "in", "sect", "except", "union")},
    **{v: ("rfx_" + v, 2, "rfx_last_bucket_on_gpu") for v in ("xrank", "xbar", "within")},
    **{v: ("rfx_" + v, 1, "rfx_last_bucket_on_gpu") for v in ("floor", "ceil", "round", "neg")},
    "filter": ("rfx_filter", 2, "rfx_last_rows_on_gpu"), "take": ("rfx_take", 2, "rfx_last_rows_on_gpu"), "reverse": ("rfx_reverse", 1, "rfx_last_rows_on_gpu"),
    "as": ("rfx_as", 2, "rfx_last_cast_on_gpu"),
    "med": ("rfx_med", 1, None), "dev": ("rfx_dev", 1, None),
}


def build(ops, d, retyped):
    """-> the object; `retyped` collects the lists that carry another type code (they are dropped as the lists they are)"""
    if d is None:
        return None
    if "vec" in d:
        cells = np.array(d["cells"], dtype=DTYPE[d["vec"]])
        o = ops.rfx_host_vector(d["vec"], cells.size)
        if cells.size:
            C.memmove(H.payload(o), cells.ctypes.data, cells.nbytes)
        H.header(o).attrs = d.get("attrs", 0)
        return o
    if "atom" in d:
        if d["atom"] == T_F64:
            return ops.rfx_host_f64(d["v"])
        o = ops.rfx_host_i64(0)
        cell = np.array([d["v"]], dtype=DTYPE[d["atom"]])
        C.memmove(o + 8, cell.ctypes.data, cell.nbytes)
        H.header(o).type = -d["atom"]
        return o
    if "sym" in d:
        o = ops.rfx_host_symbol(d["sym"].encode())
        H.header(o).attrs = d.get("attrs", 0)
        return o
    if "syms" in d:
        return H.symbols(d["syms"])
    if "list" in d:
        o = H.list_of([build(ops, x, retyped) for x in d["list"]])
        if "type" in d:
            H.header(o).type = d["type"]
            retyped.append(o)
        return o
    if "table" in d:
        return ops.rfx_host_table(H.symbols([n for n, _ in d["table"]]), H.list_of([build(ops, c, retyped) for _, c in d["table"]]))
    if "dict" in d:
        return ops.rfx_host_dict(build(ops, d["dict"][0], retyped), build(ops, d["dict"][1], retyped))
    if "fn" in d:
        return ops.rfx_host_fn(d["fn"].encode())
    if "device" in d:
        return ops.rfx_host_device_vector(d["device"], d["len"], (C.c_void_p * 1)(0x1000), 1)
    raise ValueError(d)


def describe(ops, o, args=()):
    """what the door answered, as plain data"""
    if not o:
        return {"null": True}
    h = H.header(o)
    if h.type == T_ERR:
        return {"error": H.error_text(o)}
    out = {"type": h.type, "attrs": h.attrs}
    same = [i for i, a in enumerate(args) if a == o]
    if same:
        out["is_argument"] = same[0]  # the argument itself, one reference more
    if h.type < 0 or h.type > 100:
        out["bits"] = C.c_int64.from_address(o + 8).value if h.type < 0 else None
        return out
    out["len"] = h.len
    if h.type in (T_LIST, T_TABLE, T_DICT):
        out["items"] = [describe(ops, x) for x in H.list_items(o)]
    elif h.type == T_SYMBOL:
        out["cells"] = [ops.rfx_host_symbol_name(int(i)).decode() for i in H.to_numpy(o)]
    else:
        out["cells"] = H.to_numpy(o).tobytes().hex()
    return out


def run_case(ops, case):
    """-> the case's record: the answer, rfx_ops_last_error(), the family's flag and counters after the call"""
    name, arity, flag = VERBS[case["verb"]]
    fn = getattr(ops, name)
    retyped = []
    args = None if case["args"] is None else [build(ops, a, retyped) for a in case["args"]]
    set0, st0 = counters(ops)
    if arity == "n":
        arr = None if args is None else (C.c_void_p * len(args))(*args)
        r = fn(arr, case.get("n", 0 if args is None else len(args)))
    else:
        r = fn(*args)
    rec = {"answer": describe(ops, r, args or ()), "last_error": ops.rfx_ops_last_error().decode(errors="replace")}
    if flag:
        rec["on_gpu"] = getattr(ops, flag)()
    set1, st1 = counters(ops)
    if flag == "rfx_last_set_on_gpu":
        rec["set_route"] = ops.rfx_last_set_route()
        rec["set_stats_delta"] = [b - a for a, b in zip(set0, set1)]
    if arity == "n":
        rec["join_stats_delta"] = [st1[2] - st0[2], st1[3] - st0[3]]  # [on the GPU, delegated]
    if r:
        ops.rfx_host_drop(r)
    for o in retyped:
        H.header(o).type = T_LIST
    for a in args or ():
        if a:
            ops.rfx_host_drop(a)
    return rec


def counters(ops):
    out = []
    for fn in (ops.rfx_set_stats, ops.rfx_stats):
        o = fn(None)
        out.append(H.to_numpy(o).tolist())
        ops.rfx_host_drop(o)
    return out


def exported(ops):
    """address -> name of every entry point include/rfx_ops.h declares"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfx_ops.h")).read(), flags=re.S)
    return {C.cast(getattr(ops, n), C.c_void_p).value: n for n in sorted(set(re.findall(r"\b(rfx_[a-z0-9_]+)\s*\(", txt)))}


def fn_record(ops, name, by_address):
    """the function object rfx_host_fn(name) answers: [type code, attribute byte, exported symbol] or None"""
    f = ops.rfx_host_fn(name.encode())
    if not f:
        return None
    h = H.header(f)
    rec = [h.type, h.attrs, by_address.get(C.c_int64.from_address(f + 8).value & (2**64 - 1))]
    ops.rfx_host_drop(f)
    return rec
