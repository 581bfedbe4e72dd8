"""The set verbs over i64-like device columns -- distinct / isin / find / sect / except / union -- through the planner (include/rfx_exec.h):
marshalling only, every route decision is rfx_exec_set.c's.  A shape the reference's own tables cannot answer raises RfxUndefined."""
from __future__ import annotations

import ctypes as C
import numbers
from typing import Optional

import torch

from . import _lib as L
from ._lib import RfxError

ROUTE_NAMES = {L.RFX_SET_ROUTE_NONE: "none", L.RFX_SET_ROUTE_DENSE: "dense", L.RFX_SET_ROUTE_HASH: "hash", L.RFX_SET_ROUTE_DISJOINT: "disjoint",
               L.RFX_SET_ROUTE_ATOM: "atom"}


class RfxUndefined(RfxError):
    """The reference has no defined answer for these cells (its table would be indexed outside itself): the device declines."""


def _cols(eng, *cols):
    for c in cols:
        eng._check_col(c)
        if c.dtype != torch.int64:
            raise RfxError("the set verbs take i64-like columns on this path")


def _check(eng, rc: int, route: C.c_int, what: str) -> None:
    eng.last_set_route = ROUTE_NAMES.get(route.value, "undefined")
    if rc == L.RFX_ESTATE and route.value == L.RFX_SET_ROUTE_UNDEFINED:
        raise RfxUndefined(eng.lib.rfx_exec_last_error(eng._x).decode(errors="replace"))
    eng._xcheck(rc, what)


def distinct(eng, x: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """distinct x (y None) / union x y: rfx_exec_distinct.  The result is a view of a buffer of len x + len y cells."""
    _cols(eng, *([x] if y is None else [x, y]))
    nb = 0 if y is None else y.numel()
    out = eng.empty(x.numel() + nb)
    nout, route = C.c_int64(0), C.c_int(0)
    rc = eng.lib.rfx_exec_distinct(eng._x, x.data_ptr(), x.numel(), y.data_ptr() if nb else None, nb, out.data_ptr(), C.byref(nout), C.byref(route))
    _check(eng, rc, route, "union" if y is not None else "distinct")
    return out[:nout.value]


def member(eng, x: torch.Tensor, y: torch.Tensor, want_first: bool) -> torch.Tensor:
    """in x y (int8 0 / 1 per cell of x) / find x y (per cell of y the first row of x holding it, or null): rfx_exec_member."""
    _cols(eng, x, y)
    if want_first:
        out = eng.empty(y.numel() if x.numel() else 0)
    else:
        out = eng.empty(x.numel(), torch.int8)
    route = C.c_int(0)
    rc = eng.lib.rfx_exec_member(eng._x, x.data_ptr(), x.numel(), y.data_ptr(), y.numel(), int(bool(want_first)), out.data_ptr(), C.byref(route))
    _check(eng, rc, route, "find" if want_first else "in")
    return out


def set_filter(eng, x: torch.Tensor, y, keep_members: bool) -> torch.Tensor:
    """sect x y (keep_members) / except x y; y a column, or -- except only -- an integer: rfx_exec_set_filter."""
    atom = isinstance(y, numbers.Integral)  # (a numpy integer too)
    if atom and keep_members:
        raise RfxError("sect takes two columns")
    _cols(eng, *([x] if atom else [x, y]))
    out = eng.empty(x.numel())
    nout, route = C.c_int64(0), C.c_int(0)
    rc = eng.lib.rfx_exec_set_filter(eng._x, x.data_ptr(), x.numel(), None if atom else y.data_ptr(), 0 if atom else y.numel(), int(atom), int(y) if atom else 0,
                                     int(bool(keep_members)), out.data_ptr(), C.byref(nout), C.byref(route))
    _check(eng, rc, route, "sect" if keep_members else "except")
    return out[:nout.value]
