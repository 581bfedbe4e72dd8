"""ctypes view of the operator-level C ABI (include/rfx_ops.h) and of the standalone host object model (rfx_host.c).

Used by the tests to drive ``rfx_select`` & friends exactly as the reference's evaluator would: with obj_p arguments
laid out like RayforceDB objects (include/rfx_abi.h).  Nothing here computes anything.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np

from . import _lib as L

T_LIST, T_B8, T_I64, T_SYMBOL, T_F64, T_TABLE, T_DICT, T_ERR = 0, 1, 5, 6, 10, 98, 99, 127
NP_OF = {T_B8: np.int8, T_I64: np.int64, T_SYMBOL: np.int64, T_F64: np.float64, 9: np.int64, 4: np.int32, 7: np.int32, 8: np.int32, 2: np.uint8, 3: np.int16}
TYPE_OF = {np.dtype(np.int8): T_B8, np.dtype(np.bool_): T_B8, np.dtype(np.int64): T_I64, np.dtype(np.float64): T_F64}

OPS_PROTOTYPES = {
    "rfx_host_bind": (C.c_int, []),
    "rfx_ops_set_device": (C.c_int, [C.c_int]),
    "rfx_ops_last_error": (C.c_char_p, []),
    "rfx_ops_set_shards": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int]),
    "rfx_ops_shards": (C.c_int, []),
    "rfx_ops_set_validation": (C.c_int, [C.c_int]),
    "rfx_ops_set_deterministic": (C.c_int, [C.c_int]),
    "rfx_ops_set_rank_slices": (C.c_int, [C.c_int]),
    "rfx_ops_dist_init": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "rfx_ops_dist_finalize": (C.c_int, []),
    "rfx_ops_exec": (C.c_void_p, []),
    "rfx_host_device_vector": (C.c_void_p, [C.c_int8, C.c_int64, C.POINTER(C.c_void_p), C.c_int]),
    "rfx_select": (C.c_void_p, [C.c_void_p]),
    "rfx_update": (C.c_void_p, [C.c_void_p]),
    **{f"rfx_{n}": (C.c_void_p, [C.c_void_p, C.c_void_p]) for n in ("eq", "ne", "lt", "gt", "le", "ge", "at", "add", "sub", "mul", "div", "floordiv", "mod")},
    "rfx_and": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_or": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_and_sf": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_or_sf": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_left_join": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_inner_join": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    **{f"rfx_{n}": (C.c_void_p, [C.c_void_p]) for n in ("where", "sum", "avg", "min", "max", "count", "first", "last", "dev", "pin", "unpin", "invalidate", "stats", "group", "med", "iasc", "idesc", "asc", "desc", "rank")},
    "rfx_xasc": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_xdesc": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_last_sort_on_gpu": (C.c_int, []),
    "rfx_asof_join": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_bin": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_binr": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_last_asof_on_gpu": (C.c_int, []),
    "rfx_window_join": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_window_join1": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_last_window_on_gpu": (C.c_int, []),
    "rfx_distinct": (C.c_void_p, [C.c_void_p]),
    **{f"rfx_{n}": (C.c_void_p, [C.c_void_p, C.c_void_p]) for n in ("find", "in", "sect", "except", "union")},
    "rfx_last_set_on_gpu": (C.c_int, []),
    "rfx_last_set_route": (C.c_int, []),
    "rfx_set_stats": (C.c_void_p, [C.c_void_p]),
    **{f"rfx_{n}": (C.c_void_p, [C.c_void_p, C.c_void_p]) for n in ("xrank", "xbar", "within")},
    **{f"rfx_{n}": (C.c_void_p, [C.c_void_p]) for n in ("floor", "ceil", "round", "neg")},
    "rfx_last_bucket_on_gpu": (C.c_int, []),
    "rfx_filter": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_take": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_reverse": (C.c_void_p, [C.c_void_p]),
    "rfx_last_rows_on_gpu": (C.c_int, []),
    "rfx_as": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_last_cast_on_gpu": (C.c_int, []),
    "rfx_concat": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_raze": (C.c_void_p, [C.c_void_p]),
    "rfx_last_concat_on_gpu": (C.c_int, []),
    "rfx_upsert": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_insert": (C.c_void_p, [C.POINTER(C.c_void_p), C.c_int64]),
    "rfx_last_upsert_on_gpu": (C.c_int, []),
    "rfx_row": (C.c_void_p, [C.c_void_p]),
    "rfx_collect": (C.c_void_p, [C.c_void_p]),
    "rfx_last_collect_on_gpu": (C.c_int, []),
    "rfx_cache_clear": (None, []),
    "rfx_cache_bytes": (C.c_int64, []),
    "rfx_last_select_on_gpu": (C.c_int, []),
    "rfx_host_vector": (C.c_void_p, [C.c_int8, C.c_int64]),
    "rfx_host_i64": (C.c_void_p, [C.c_int64]),
    "rfx_host_f64": (C.c_void_p, [C.c_double]),
    "rfx_host_symbol": (C.c_void_p, [C.c_char_p]),
    "rfx_host_list": (C.c_void_p, [C.c_int64]),
    "rfx_host_table": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_host_dict": (C.c_void_p, [C.c_void_p, C.c_void_p]),
    "rfx_host_fn": (C.c_void_p, [C.c_char_p]),
    "rfx_host_clone": (C.c_void_p, [C.c_void_p]),
    "rfx_host_drop": (None, [C.c_void_p]),
    "rfx_host_intern": (C.c_int64, [C.c_char_p, C.c_int64]),
    "rfx_host_symbol_name": (C.c_char_p, [C.c_int64]),
    "rfx_host_error_text": (C.c_char_p, [C.c_void_p]),
}


class Header(C.Structure):
    _fields_ = [("mmod", C.c_uint8), ("order", C.c_uint8), ("type", C.c_int8), ("attrs", C.c_uint8), ("rc", C.c_uint32), ("len", C.c_int64)]


_bound = None


def lib() -> C.CDLL:
    global _bound
    if _bound is None:
        l = L.load_library()
        for name, (res, args) in OPS_PROTOTYPES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _bound = l
    return _bound


def header(o: int) -> Header:
    return Header.from_address(o)


def payload(o: int) -> int:
    return o + 16


def vector(a: np.ndarray) -> int:
    a = np.ascontiguousarray(a)
    t = TYPE_OF[a.dtype]
    o = lib().rfx_host_vector(t, a.size)
    if a.size:
        C.memmove(payload(o), a.ctypes.data, a.nbytes)
    return o


T_U8, T_I16, T_I32, T_DATE, T_TIME, T_TIMESTAMP, T_MAPFILTER, T_MAPGROUP, T_NULL = 2, 3, 4, 7, 8, 9, 71, 72, 126
TYPE_NAMES = {"b8": T_B8, "u8": T_U8, "i16": T_I16, "i32": T_I32, "i64": T_I64, "symbol": T_SYMBOL, "date": T_DATE, "time": T_TIME, "timestamp": T_TIMESTAMP,
              "f64": T_F64}


def typed_vector(a: np.ndarray, t) -> int:
    """A vector of the reference's type code `t` (or its name in TYPE_NAMES) over the cells of `a`, whose dtype must be that type's cell: the narrow
    types (U8, I16, I32 / DATE / TIME) and the 8-byte ones that share int64 cells (SYMBOL, TIMESTAMP)."""
    t = TYPE_NAMES[t] if isinstance(t, str) else int(t)
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.int8)
    if np.dtype(NP_OF[t]) != a.dtype:
        raise TypeError(f"type {t} holds {np.dtype(NP_OF[t])} cells, not {a.dtype}")
    o = lib().rfx_host_vector(t, a.size)
    if a.size:
        C.memmove(payload(o), a.ctypes.data, a.nbytes)
    return o


def group_index(itype: int, groups: int, group_ids: np.ndarray, shift=None, source=None, filt=None, firsts=None) -> int:
    """The reference's 7-slot group index (index_group_build): [type, groups, ids | key table, shift, source column, filter ids, first rows]; slots that
    are not given stay the null object."""
    ix = lib().rfx_host_list(7)
    arr = (C.c_void_p * 7).from_address(payload(ix))
    arr[0], arr[1] = atom(int(itype)), atom(int(groups))
    arr[2] = vector(np.asarray(group_ids, dtype=np.int64))
    arr[3] = atom(int(shift) if itype == 1 else -(2 ** 63))
    if source is not None:
        arr[4] = vector(np.asarray(source, dtype=np.int64))
    if filt is not None:
        arr[5] = vector(np.asarray(filt, dtype=np.int64))
    if firsts is not None:
        arr[6] = vector(np.asarray(firsts, dtype=np.int64))
    return ix


def pair(val: int, index: int, t: int = T_MAPGROUP) -> int:
    """A lazy (val, index) pair as an FN_AGGR built-in receives it: MAPGROUP (a group index) or MAPFILTER (row ids)."""
    p = list_of([val, index])
    header(p).type = t
    return p


def list_to_numpy(o: int):
    """A LIST of vectors -> [(type code, attribute byte, cells)] per item"""
    return [(header(i).type, header(i).attrs, to_numpy(i)) for i in list_items(o)]


def to_numpy(o: int) -> np.ndarray:
    h = header(o)
    dt = NP_OF[h.type]
    return np.frombuffer((C.c_char * (h.len * np.dtype(dt).itemsize)).from_address(payload(o)), dtype=dt).copy() if h.len else np.empty(0, dt)


def list_of(items: Sequence[int]) -> int:
    o = lib().rfx_host_list(len(items))
    arr = (C.c_void_p * len(items)).from_address(payload(o))
    for i, it in enumerate(items):
        arr[i] = it
    return o


def list_items(o: int):
    h = header(o)
    return list((C.c_void_p * h.len).from_address(payload(o)))


def symbols(names: Sequence[str]) -> int:
    l = lib()
    o = l.rfx_host_vector(T_SYMBOL, len(names))
    arr = (C.c_int64 * len(names)).from_address(payload(o))
    for i, n in enumerate(names):
        arr[i] = l.rfx_host_intern(n.encode(), len(n))
    return o


def table(cols: Dict[str, np.ndarray]) -> int:
    return lib().rfx_host_table(symbols(list(cols)), list_of([vector(v) for v in cols.values()]))


def device_vector(t, ptrs=None) -> int:
    """A DEVICE column handle (rfx_host_device_vector): a torch CUDA tensor's cells handed to the operators where they are.  `ptrs`: one
    device address per shard (columns kept shard by shard on several devices); default: the tensor's one allocation."""
    import torch
    tp = {torch.int64: T_I64, torch.float64: T_F64, torch.int8: T_B8}[t.dtype]
    ps = [t.data_ptr()] if ptrs is None else list(ptrs)
    return lib().rfx_host_device_vector(tp, t.numel(), (C.c_void_p * len(ps))(*ps), len(ps))


def device_table(cols) -> int:
    """dict name -> CUDA tensor as a table object whose columns are device handles (the tensors must outlive the table)."""
    return lib().rfx_host_table(symbols(list(cols)), list_of([device_vector(v) for v in cols.values()]))


def atom(x) -> int:
    l = lib()
    if isinstance(x, str):
        return l.rfx_host_symbol(x.encode())
    if isinstance(x, (int, np.integer)):
        return l.rfx_host_i64(int(x))
    return l.rfx_host_f64(float(x))


def expr(e) -> int:
    """('<', 'a', 5) / ('and', e1, e2) / ('sum', 'v') -> LIST [function object, args...] as the reference's parser builds it."""
    if isinstance(e, tuple):
        return list_of([lib().rfx_host_fn(e[0].encode())] + [expr(x) for x in e[1:]])
    return atom(e)


def select_dict(query: Dict, tab: int) -> int:
    """{name: ('sum', 'v'), 'where': (...), 'by': 'k'} + table object -> the select DICT."""
    keys, vals = [], []
    for k, v in query.items():
        keys.append(k)
        if k == "by" and isinstance(v, dict):  # by: {name: column ...} -> DICT of SYMBOL keys, LIST of symbol atoms
            vals.append(lib().rfx_host_dict(symbols(list(v.keys())), list_of([expr(c) for c in v.values()])))  # column symbol or (xbar col w)
        else:
            vals.append(atom(v) if k == "by" else expr(v))
    keys.append("from")
    vals.append(lib().rfx_host_clone(tab))
    return lib().rfx_host_dict(symbols(keys), list_of(vals))


def table_to_numpy(o: int) -> Dict[str, np.ndarray]:
    l = lib()
    keys, vals = list_items(o)
    names = [l.rfx_host_symbol_name(int(i)).decode() for i in to_numpy(keys)]
    return {n: to_numpy(c) for n, c in zip(names, list_items(vals))}


def is_error(o: int) -> bool:
    return header(o).type == T_ERR


def error_text(o: int) -> str:
    return lib().rfx_host_error_text(o).decode(errors="replace")
