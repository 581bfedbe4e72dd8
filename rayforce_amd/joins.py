"""lj / ij over device columns (ray_left_join / ray_inner_join, core/join.c:158-298): the join INDEX is the planner's
(rfx_exec_join_index); what is here is the reference's column rule for the result -- keys, then the other left columns, then the
right-only ones -- assembled with one gather per column."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib as L
from ._lib import RfxError

def join_index(eng, keys, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Per LEFT row the FIRST right row with an equal key tuple, or null (index_left_join_obj, core/index.c:2886-2928): the planner's
    rfx_exec_join_index (dense / hashed build side, composite key or row hash + tuple check)."""
    keys = [keys] if isinstance(keys, str) else list(keys)
    lk = [eng._check_col(eng._resolve(k, left)) for k in keys]
    rk = [eng._check_col(eng._resolve(k, right)) for k in keys]
    if any(c.dtype != torch.int64 for c in lk + rk):
        raise RfxError("join keys must be i64-like columns on this path")
    nl, nr = lk[0].numel(), rk[0].numel()
    ids = eng.empty(nl)
    k = len(keys)
    col = C.c_int(0)
    rc = eng.lib.rfx_exec_join_index(eng._x, (C.c_void_p * k)(*[c.data_ptr() for c in lk]), (C.c_void_p * k)(*[c.data_ptr() for c in rk]), k, nl, nr,
                                      ids.data_ptr(), C.byref(col))
    if rc != L.RFX_OK and col.value:
        raise RfxError("join: two key tuples share one 64-bit row hash (collision); not answered on this path")
    eng._xcheck(rc, "join_index")
    return ids

def left_join(eng, keys, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``(lj [keys] left right)`` -- ray_left_join, core/join.c:158-198: every left row; a non-key column that the right table has takes
    the matched right row's value, else the left row's own (null when the left table lacks the column); columns: keys, then the other
    left columns, then the right-only ones.  Empty side -> the left table."""
    keys = [keys] if isinstance(keys, str) else list(keys)
    nl = next(iter(left.values())).numel() if left else 0
    nr = next(iter(right.values())).numel() if right else 0
    if nl == 0 or nr == 0:
        return dict(left)
    ids = join_index(eng, keys, left, right)
    out = {k: left[k] for k in keys}
    for name in [c for c in left if c not in keys] + [c for c in right if c not in keys and c not in left]:
        if name not in right:
            out[name] = left[name]
            continue
        rc, lc = right[name], left.get(name)
        if lc is not None and lc.dtype != rc.dtype:
            raise RfxError(f"join: column {name} has different types in the two tables")
        o = torch.empty(nl, dtype=rc.dtype, device=eng.device)
        fill = 0x7FF8000000000000 if rc.dtype == torch.float64 else (1 << 63)  # NaN / NULL_I64 bit patterns
        L.check(eng.lib.rfx_hip_gather_or(eng._ctx, rc.data_ptr(), lc.data_ptr() if lc is not None else None, ids.data_ptr(), nl, fill, o.data_ptr()), "gather_or")
        out[name] = o
    eng.sync()
    return out

def inner_join(eng, keys, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``(ij [keys] left right)`` -- ray_inner_join, core/join.c:200-298: the left rows that have a match, in left order, paired with
    their first matching right row; a column the right table has comes from the right row."""
    keys = [keys] if isinstance(keys, str) else list(keys)
    nl = next(iter(left.values())).numel() if left else 0
    nr = next(iter(right.values())).numel() if right else 0
    if nl == 0 or nr == 0:
        return dict(left)
    ids = join_index(eng, keys, left, right)
    lids = eng.where(("!=", ids, None))  # ascending left rows with a match
    rids = eng.at_ids(ids, lids)
    out = {}
    for name in keys + [c for c in left if c not in keys] + [c for c in right if c not in keys and c not in left]:
        if name in right:
            if name in left and left[name].dtype != right[name].dtype:
                raise RfxError(f"join: column {name} has different types in the two tables")
            out[name] = eng.at_ids(right[name], rids)
        else:
            out[name] = eng.at_ids(left[name], lids)
    return out


def asof_index(eng, keys, time, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Per LEFT row the right row of the same ``keys`` tuple that the reference's binary search by ``time`` over the tuple's rows (in row
    order) lands on, or null (index_asof_join_obj, core/index.c:3194-3267): the planner's rfx_exec_asof_index.  i64 columns throughout."""
    keys = [keys] if isinstance(keys, str) else list(keys)
    if not keys:
        raise RfxError("asof_index needs at least one equality key")
    lk = [eng._check_col(eng._resolve(k, left)) for k in keys]
    rk = [eng._check_col(eng._resolve(k, right)) for k in keys]
    nl, nr = lk[0].numel(), rk[0].numel()
    lt, rt = eng._check_col(eng._resolve(time, left), nl), eng._check_col(eng._resolve(time, right), nr)
    if any(c.dtype != torch.int64 for c in lk + rk + [lt, rt]):
        raise RfxError("asof keys and times must be i64-like columns on this path")
    ids = eng.empty(nl)
    k = len(keys)
    col = C.c_int(0)
    rc = eng.lib.rfx_exec_asof_index(eng._x, (C.c_void_p * k)(*[c.data_ptr() for c in lk]), (C.c_void_p * k)(*[c.data_ptr() for c in rk]), k,
                                      lt.data_ptr(), rt.data_ptr(), nl, nr, ids.data_ptr(), C.byref(col))
    if rc != L.RFX_OK and col.value:
        raise RfxError("asof join: two key tuples share one 64-bit row hash (collision); not answered on this path")
    eng._xcheck(rc, "asof_index")
    return ids

def asof_join(eng, keys, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``(asof-join [k1 .. kn t] left right)`` -- ray_asof_join, core/join.c:300-356: ``keys`` names the equality columns and, last, the asof
    column; the result is the left join's (all key columns are the left table's own; no empty-table short-cut)."""
    keys = list(keys)
    if len(keys) < 2:
        raise RfxError("asof_join needs at least one equality key and the asof column")
    nl = next(iter(left.values())).numel() if left else 0
    ids = asof_index(eng, keys[:-1], keys[-1], left, right)
    out = {k: left[k] for k in keys}
    for name in [c for c in left if c not in keys] + [c for c in right if c not in keys and c not in left]:
        if name not in right:
            out[name] = left[name]
            continue
        rc, lc = right[name], left.get(name)
        if lc is not None and lc.dtype != rc.dtype:
            raise RfxError(f"join: column {name} has different types in the two tables")
        o = torch.empty(nl, dtype=rc.dtype, device=eng.device)
        fill = 0x7FF8000000000000 if rc.dtype == torch.float64 else (1 << 63)  # NaN / NULL_I64 bit patterns
        if rc.numel() == 0:  # (nothing to read from: every id is null)
            rc = torch.empty(1, dtype=rc.dtype, device=eng.device)
        L.check(eng.lib.rfx_hip_gather_or(eng._ctx, rc.data_ptr(), lc.data_ptr() if lc is not None else None, ids.data_ptr(), nl, fill, o.data_ptr()), "gather_or")
        out[name] = o
    eng.sync()
    return out

def bin_search(eng, x: torch.Tensor, y: torch.Tensor, right: bool) -> torch.Tensor:
    """bin (right = False) / binr (True) of two i64 device columns: rfx_exec_bin."""
    eng._check_col(x)
    eng._check_col(y)
    if x.dtype != torch.int64 or y.dtype != torch.int64:
        raise RfxError("bin / binr take i64-like columns on this path")
    out = eng.empty(y.numel())
    eng._xcheck(eng.lib.rfx_exec_bin(eng._x, x.data_ptr(), x.numel(), y.data_ptr(), y.numel(), int(bool(right)), out.data_ptr()), "bin")
    eng.sync()
    return out


def window_ranges(eng, keys, time, windows, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor], closed: bool = False):
    """The window join's build and probe (rfx_exec_window_ranges): (perm, li, ri, long_windows, longest) -- the right rows in the stable order of
    (key tuple, ``time``), and per left row the first and last position of its window in that order, (-1, -2) for the null row.  i64 columns
    throughout; the times and the bounds hold 32-bit values (the reference compares them as such)."""
    keys = [keys] if isinstance(keys, str) else list(keys)
    if not keys:
        raise RfxError("window_join needs at least one equality key")
    lk = [eng._check_col(eng._resolve(k, left)) for k in keys]
    rk = [eng._check_col(eng._resolve(k, right)) for k in keys]
    nl, nr = lk[0].numel(), rk[0].numel()
    rt = eng._check_col(eng._resolve(time, right), nr)
    lo, hi = (eng._check_col(w, nl) for w in windows)
    if any(c.dtype != torch.int64 for c in lk + rk + [rt, lo, hi]):
        raise RfxError("window join keys, times and bounds must be i64-like columns on this path")
    perm, li, ri = eng.empty(nr), eng.empty(nl), eng.empty(nl)
    k = len(keys)
    col, stats = C.c_int(0), (C.c_int64 * 2)()
    rc = eng.lib.rfx_exec_window_ranges(eng._x, (C.c_void_p * k)(*[c.data_ptr() for c in lk]), (C.c_void_p * k)(*[c.data_ptr() for c in rk]), k, lo.data_ptr(),
                                         hi.data_ptr(), rt.data_ptr(), nl, nr, int(bool(closed)), perm.data_ptr(), li.data_ptr(), ri.data_ptr(), stats, C.byref(col))
    if rc != L.RFX_OK and col.value:
        raise RfxError("window join: two key tuples share one 64-bit row hash (collision); not answered on this path")
    eng._xcheck(rc, "window_ranges")
    return perm, li, ri, int(stats[0]), int(stats[1])

def window_fold(eng, vals: torch.Tensor, perm, li: torch.Tensor, ri: torch.Tensor, long_windows: int, aggs) -> Dict[str, torch.Tensor]:
    """Every aggregate of ``aggs`` (names of RFX_WAGG) of ONE right column over the windows, in one launch (rfx_exec_window_fold); ``perm`` None:
    ``vals`` is in the sorted order already."""
    eng._check_col(vals)
    if vals.dtype not in (torch.int64, torch.float64):
        raise RfxError("window join aggregates take I64 or F64 columns on this path")
    nl = li.numel()
    outs, ptrs = {}, (C.c_void_p * len(L.RFX_WAGG))()
    for a in aggs:
        if a not in L.RFX_WAGG:
            raise RfxError(f"window join: {a} is not one of {', '.join(L.RFX_WAGG)}")
        dt = torch.int64 if a == "count" else torch.float64 if a == "avg" else vals.dtype
        outs[a] = torch.empty(nl, dtype=dt, device=eng.device)
        ptrs[L.RFX_WAGG[a]] = outs[a].data_ptr()
    eng._xcheck(eng.lib.rfx_exec_window_fold(eng._x, vals.data_ptr(), L.RFX_F64 if vals.dtype == torch.float64 else L.RFX_I64, perm.data_ptr() if perm is not None else None,
                                             li.data_ptr(), ri.data_ptr(), nl, vals.numel(), long_windows, ptrs), "window_fold")
    return outs

def window_join(eng, keys, windows, left: Dict[str, torch.Tensor], right: Dict[str, torch.Tensor], aggs, closed: bool = False) -> Dict[str, torch.Tensor]:
    """``(window-join [k1 .. kn t] windows left right {name: (agg col) ...})`` -- ray_window_join / ray_window_join1 (``closed``), core/join.c:358-489:
    the left table's columns, then one column per entry of ``aggs`` = {name: (agg, right column)}."""
    keys = list(keys)
    if len(keys) < 2:
        raise RfxError("window_join needs at least one equality key and the window column")
    perm, li, ri, nlong, _ = window_ranges(eng, keys[:-1], keys[-1], windows, left, right, closed)
    out = dict(left)
    by_col: Dict[str, list] = {}
    for name, (agg, col) in aggs.items():
        if col not in right:
            raise RfxError(f"window join: the right table has no column {col}")
        by_col.setdefault(col, []).append(agg)
    folded = {col: window_fold(eng, right[col], perm, li, ri, nlong, sorted(set(a))) for col, a in by_col.items()}
    for name, (agg, col) in aggs.items():
        out[name] = folded[col][agg]
    return out
