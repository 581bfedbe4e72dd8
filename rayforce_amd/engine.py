"""Python host of librfx.so for the tests and bench.py: the reference's select / where / by surface over HBM-resident columns.

There is NO planning here.  Every query goes to the library's planner (include/rfx_exec.h: rfx_exec_filter_aggr / rfx_exec_where /
rfx_exec_group_by / rfx_exec_join_index) or, for `select`, through the C operator door itself (rfx_select on device-column handles);
this file only marshals: tuples -> rfx_pred_t / rfx_agg_t descriptors, torch tensors -> device addresses, result blocks -> tensors.
Columns are 1-D ``torch.int64`` / ``torch.float64`` CUDA tensors (torch owns memory and the stream); there is no CPU fallback.

Predicates are tuples ``(op, lhs, rhs)`` with op in ``== != < > <= >=``, lhs a column (tensor or table column name) or an element-wise
expression ``(+|-|*|div|/|% x y)``, rhs a Python int / float atom, a column or an expression; ``("and", ...)`` / ``("or", ...)`` nest
freely: up to eight comparisons in four levels run fused in the query's one pass (rfx_pred_t's tree form), anything wider is evaluated
into a B8 mask first (mask_of) and handed to the planner as the selection.  Names follow RayforceDB (core/env.c:135-225).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L
from . import marshal as M
from ._lib import RfxError
from .marshal import NotFused as _NotFused, ctype_of as _ctype_of

Column = torch.Tensor
_NARROW_SORT_TYPES = {torch.int32: L.RFX_I32, torch.int16: L.RFX_I16, torch.uint8: L.RFX_U8, torch.bool: L.RFX_B8}


def _sort_type_of(t: torch.Tensor) -> int:
    """A sort key column's type code: the 8-byte ones, or a narrow one as its raw cells."""
    narrow = _NARROW_SORT_TYPES.get(t.dtype)
    return narrow if narrow is not None else _ctype_of(t)


def _no_narrow_over_shards(cols) -> None:
    if any(c.dtype in _NARROW_SORT_TYPES for c in cols):
        raise RfxError("sort: 1-, 2- and 4-byte key columns do not sort over shards (rfx_exec_sort_shards takes i64 / f64 pieces)")


class _Owner:
    """Holds a result struct of the planner (rfx_groups_t / rfx_ids_t) until no tensor views its device blocks any more."""

    def __init__(self, eng, struct, free):
        self.eng, self.struct, self.free = eng, struct, free

    def __del__(self):
        try:
            if self.eng._x:
                self.free(self.eng._x, C.byref(self.struct))
        except Exception:  # pragma: no cover -- interpreter shutdown
            pass


class _View:
    def __init__(self, owner, ptr: int, n: int, typestr: str):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class Engine:
    """One GPU.  ``shards=k`` splits every query row-range over k contexts on that GPU (each on its own stream and host thread, merged by
    the planner's device kernels): the logic one evaluator process runs over the GPUs of a node, testable on one.

    An Engine is driven by ONE Python thread at a time (the planner and its contexts are not re-entrant).  Results hold their device blocks
    through an owner object whose finaliser may run on whatever thread the garbage collector picks: that is safe -- it only hands blocks
    back to the contexts' pools, which share one process-wide lock (rfx_ctx.hip) -- but it is the only cross-thread call that is."""

    def __init__(self, device: Union[int, torch.device, None] = None, shards: int = 1):
        self.lib = L.load_library()
        if not torch.cuda.is_available():
            raise RfxError("no GPU visible to torch: the MI355X engine has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index)
        torch.cuda.set_device(self.device)
        self.shards = int(shards)
        self._ctxs = (C.c_void_p * self.shards)()
        # shard 0 runs on torch's current stream (tensor ops and librfx kernels are ordered without extra syncs); further shards own theirs
        stream = torch.cuda.current_stream(self.device).cuda_stream or 1  # 0 = legacy default stream -> RFX_STREAM_LEGACY
        for s in range(self.shards):
            c = C.c_void_p()
            L.check(self.lib.rfx_hip_ctx_create(self.device.index, C.c_void_p(stream if s == 0 else 0), C.byref(c)), "ctx_create")
            self._ctxs[s] = c.value
        self._ctx = C.c_void_p(self._ctxs[0])
        self._x = C.c_void_p()
        L.check(self.lib.rfx_exec_create(self._ctxs, self.shards, C.byref(self._x)), "exec_create")
        self._keep: List = []
        self.last_set_route = "none"  # the route of the last set verb (rayforce_amd/sets.py): none / dense / hash / disjoint / atom / undefined

    def close(self) -> None:
        if self._x:
            self.lib.rfx_exec_destroy(self._x)
            self._x = C.c_void_p()
            for s in range(self.shards):
                self.lib.rfx_hip_ctx_destroy(C.c_void_p(self._ctxs[s]))
            self._ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _xcheck(self, rc: int, what: str) -> None:
        if rc != L.RFX_OK:
            raise RfxError(f"{what} failed with code {rc}: {self.lib.rfx_exec_last_error(self._x).decode(errors='replace')}")

    def sync(self) -> None:
        L.check(self.lib.rfx_hip_ctx_sync(self._ctx), "sync")

    def trim(self) -> None:
        """Give the blocks the contexts keep for reuse back to the device (before a phase that needs the memory for columns)."""
        for s in range(self.shards):
            L.check(self.lib.rfx_hip_ctx_trim(C.c_void_p(self._ctxs[s])), "ctx_trim")

    def tune(self, blocks_per_cu: int = 0, flags: int = 0) -> None:
        for s in range(self.shards):
            L.check(self.lib.rfx_hip_ctx_tune(C.c_void_p(self._ctxs[s]), blocks_per_cu, flags), "tune")

    def stat(self, which: int) -> int:
        """Path counters (include/rfx_hip.h RFX_STAT_*), summed over the shards."""
        return sum(int(self.lib.rfx_hip_ctx_stat(C.c_void_p(self._ctxs[s]), which)) for s in range(self.shards))

    def xstat(self, which: int) -> int:
        """The planner's counters (include/rfx_exec.h RFX_XSTAT_*)."""
        return int(self.lib.rfx_exec_stat(self._x, which))

    @property
    def spec_retries(self) -> int:
        return self.xstat(L.RFX_XSTAT_SCOPE_RETRIED)

    def forget_scopes(self) -> None:
        self.lib.rfx_exec_forget_scopes(self._x)

    def timer_start(self) -> None:
        L.check(self.lib.rfx_hip_timer_start(self._ctx), "timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        L.check(self.lib.rfx_hip_timer_stop(self._ctx, C.byref(ms)), "timer_stop")
        return float(ms.value)

    def profile(self, enable: bool = True) -> None:
        L.check(self.lib.rfx_hip_ctx_profile(self._ctx, int(enable)), "ctx_profile")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        L.check(self.lib.rfx_hip_last_kernel_ms(self._ctx, C.byref(ms)), "last_kernel_ms")
        return float(ms.value)

    def empty(self, n: int, dtype=torch.int64) -> torch.Tensor:
        return torch.empty(int(n), dtype=dtype, device=self.device)

    def column(self, host_array) -> torch.Tensor:
        """Upload a numpy int64 / float64 / int8 / bool array (host -> HBM over PCIe; not part of any timed region)."""
        t = torch.as_tensor(host_array)
        if t.dtype not in (torch.int64, torch.float64, torch.int8, torch.bool):
            raise RfxError(f"unsupported dtype {t.dtype}")
        return (t.to(torch.int8) if t.dtype == torch.bool else t).contiguous().to(self.device)

    def upload(self, host_array) -> torch.Tensor:
        """Host numpy array (i64 / f64) -> device column through the pipelined path (what rfx_ops.c's residency cache uses)."""
        import numpy as np
        a = np.ascontiguousarray(host_array)
        if a.ndim != 1 or a.dtype not in (np.int64, np.float64):
            raise RfxError(f"upload: a 1-d int64 / float64 array is expected, not {a.dtype} with shape {a.shape}")
        out = torch.empty(a.shape[0], dtype=torch.float64 if a.dtype == np.float64 else torch.int64, device=self.device)
        L.check(self.lib.rfx_hip_h2d_pipelined(self._ctx, out.data_ptr(), a.ctypes.data, a.nbytes), "h2d_pipelined")
        return out

    def gen_i64(self, n: int, seed: int, modulus: int, row0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = self.empty(n, torch.int64) if out is None else out
        L.check(self.lib.rfx_hip_gen_i64(self._ctx, out.data_ptr(), n, seed, row0, modulus), "gen_i64")
        return out

    def gen_f64(self, n: int, seed: int, row0: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = self.empty(n, torch.float64) if out is None else out
        L.check(self.lib.rfx_hip_gen_f64(self._ctx, out.data_ptr(), n, seed, row0), "gen_f64")
        return out

    # on-disk columns: rayforce_amd/colfiles.py
    def load_column(self, path: str) -> torch.Tensor:
        from . import colfiles
        return colfiles.load_column(self, path)

    def load_splayed(self, directory: str, columns: Optional[Sequence[str]] = None) -> Dict[str, torch.Tensor]:
        from . import colfiles
        return colfiles.load_splayed(self, directory, columns)

    def load_parted(self, root: str, table: str, columns: Optional[Sequence[str]] = None, where=None) -> Dict[str, torch.Tensor]:
        from . import colfiles
        return colfiles.load_parted(self, root, table, columns, where)

    # ------------------------------------------------------------------ marshalling: tuples -> descriptors (rayforce_amd/marshal.py)
    def _check_col(self, t, n=None):
        return M.check_col(self, t, n)

    def _resolve(self, x, table):
        return M.resolve(self, x, table)

    def _query(self, where, aggs, table, nrows: Optional[int], keys=None, flags: int = 0) -> Tuple[L.Query, int]:
        """The planner's query over this engine's shards: descriptors in shard 0's addresses + every column's address per shard."""
        self._keep.clear()
        q = L.Query()
        n = nrows
        if isinstance(where, torch.Tensor):  # a B8 mask as the selection
            m = self._check_col(where.view(torch.int8) if where.dtype == torch.bool else where, n)
            if m.dtype != torch.int8:
                raise RfxError("where expects a B8 mask")  # reference: err_type (core/items.c:1395)
            q.d_mask, n = m.data_ptr(), m.numel()
            self._keep.append(m)
        else:
            try:
                logic, leaves, more = M.tree_leaves(self, where)
            except _NotFused:
                return self._query(self.mask_of(where, table), aggs, table, nrows, keys, flags)
            parr, n = M.preds(self, leaves, more, table, n)
            q.preds, q.npred, q.logic = parr, len(leaves), logic
            self._keep.append(parr)
        aarr, n = M.aggs(self, aggs or [], table, n)
        q.aggs, q.nagg = aarr, len(aggs or [])
        self._keep.append(aarr)
        if keys:
            kx = (C.c_int64 * len(keys))()
            kp = (C.c_void_p * len(keys))()
            for i, k in enumerate(keys):
                if isinstance(k, tuple) and len(k) == 3 and k[0] == "xbar":  # bucketed key: evaluated by the planner (ray_xbar, core/math.c:1635)
                    if int(k[2]) <= 0:
                        raise RfxError("xbar: width must be positive")
                    col, kx[i] = self._check_col(self._resolve(k[1], table), n), int(k[2])
                else:
                    col = self._check_col(self._resolve(k, table), n)
                if col.dtype != torch.int64:
                    raise RfxError("group key must be i64 on this path (f64 keys group on their bit pattern: view as int64)")
                n = col.numel() if n is None else n
                kp[i] = col.data_ptr()
                self._keep.append(col)
            q.d_keys, q.kxbar, q.nkeys = kp, kx, len(keys)
            self._keep += [kp, kx]
        if n is None:
            raise RfxError("cannot infer the row count (count without column and without predicate needs nrows=)")
        q.nrows, q.flags = n, flags
        if self.shards > 1:  # shards of one device: every column's slice by the planner's own split rule
            ptrs = {}
            for t in self._keep:
                if isinstance(t, torch.Tensor) and t.numel() == n:
                    ptrs[t.data_ptr()] = t.element_size()
            cols = (L.QCol * max(1, len(ptrs)))()
            r0 = C.c_int64()
            for i, (p, esz) in enumerate(ptrs.items()):
                for s in range(self.shards):
                    self.lib.rfx_exec_split(n, self.shards, s, C.byref(r0), None)
                    cols[i].d[s] = p + r0.value * esz
            q.cols, q.ncols = cols, len(ptrs)
            self._keep.append(cols)
            torch.cuda.current_stream(self.device).synchronize()  # the other shards run on their own streams
        return q, n

    @staticmethod
    def _value(v: L.Value):
        if v.type == L.RFX_F64:
            return float("nan") if v.is_null else float(v.f)
        return None if v.is_null else int(v.i)

    def _view(self, owner, d_src: int, n: int, dtype) -> torch.Tensor:
        """A planner-owned device column as a torch tensor WITHOUT a copy: torch aliases the memory through __cuda_array_interface__ and keeps
        `owner` alive; the planner's blocks are released when the last tensor over them dies."""
        if not n or not d_src:
            return self.empty(0, dtype)
        return torch.as_tensor(_View(owner, d_src, n, "<f8" if dtype == torch.float64 else "<i8"), device=self.device)

    # ------------------------------------------------------------------ scalar aggregates (K1/K5)
    def filter_aggr(self, aggs, where=None, table=None, nrows: Optional[int] = None):
        """``select {aggs} from t where p`` without ``by:`` -> ([values], selected_rows).  (syncs)"""
        q, _ = self._query(where, aggs, table, nrows)
        vals = (L.Value * max(1, len(aggs)))()
        sel = C.c_int64()
        self._xcheck(self.lib.rfx_exec_filter_aggr(self._x, C.byref(q), vals, C.byref(sel)), "filter_aggr")
        return [self._value(vals[i]) for i in range(len(aggs))], int(sel.value)

    # scalar verbs of the reference (core/math.c:2388-2526, core/misc.c:43-60)
    def sum(self, col, where=None, table=None): return self.filter_aggr([("sum", col)], where, table)[0][0]
    def min(self, col, where=None, table=None): return self.filter_aggr([("min", col)], where, table)[0][0]
    def max(self, col, where=None, table=None): return self.filter_aggr([("max", col)], where, table)[0][0]
    def avg(self, col, where=None, table=None): return self.filter_aggr([("avg", col)], where, table)[0][0]
    def count(self, col, where=None, table=None): return self.filter_aggr([("count", col)], where, table)[0][0]
    def first(self, col, where=None, table=None): return self.filter_aggr([("first", col)], where, table)[0][0]
    def last(self, col, where=None, table=None): return self.filter_aggr([("last", col)], where, table)[0][0]

    def dev(self, col, where=None, table=None) -> float:
        """``(dev col)`` over the selection: ray_dev's two passes (core/math.c:2628-2699) -- NaN for no non-null cell, 0.0 for one.  (syncs)"""
        c = self._check_col(self._resolve(col, table))
        q, _ = self._query(where, [], table, c.numel())
        v = L.Value()
        self._xcheck(self.lib.rfx_exec_dev(self._x, C.byref(q), c.data_ptr(), _ctype_of(c), C.byref(v)), "dev")
        return self._value(v)

    # ------------------------------------------------------------------ K2: masks (API parity with the reference's B8 results)
    def cmp(self, op: str, lhs, rhs, table=None) -> torch.Tensor:
        """ray_eq .. ray_ge on a column: B8 byte mask (int8 tensor of 0/1)."""
        self._keep.clear()
        parr, n = M.preds(self, [(op, lhs, rhs)], [0], table, None)
        out = torch.empty(n, dtype=torch.int8, device=self.device)
        L.check(self.lib.rfx_hip_cmp_mask(self._ctx, parr, n, out.data_ptr()), "cmp_mask")
        return out

    def eq(self, a, b): return self.cmp("==", a, b)
    def ne(self, a, b): return self.cmp("!=", a, b)
    def lt(self, a, b): return self.cmp("<", a, b)
    def gt(self, a, b): return self.cmp(">", a, b)
    def le(self, a, b): return self.cmp("<=", a, b)
    def ge(self, a, b): return self.cmp(">=", a, b)

    def _logic(self, logic: int, masks) -> torch.Tensor:
        if not masks:
            raise RfxError("and/or need at least one argument")
        acc = masks[0].clone()
        for m in masks[1:]:
            if isinstance(m, (bool, int)):
                L.check(self.lib.rfx_hip_mask_logic(self._ctx, logic, acc.data_ptr(), None, int(bool(m)), acc.numel()), "mask_logic")
                continue
            if m.numel() != acc.numel():
                raise RfxError("length mismatch")  # reference: err_type on unequal lengths (core/logic.c:122-126)
            L.check(self.lib.rfx_hip_mask_logic(self._ctx, logic, acc.data_ptr(), m.data_ptr(), 0, acc.numel()), "mask_logic")
        return acc

    def and_(self, *masks) -> torch.Tensor: return self._logic(L.RFX_AND, masks)
    def or_(self, *masks) -> torch.Tensor: return self._logic(L.RFX_OR, masks)

    def mask_of(self, where, table=None) -> torch.Tensor:
        """Materialise any predicate tree as a byte mask (the reference's own evaluation order, on the GPU)."""
        head = where[0]
        if head in L.OPS:
            return self.cmp(head, where[1], where[2], table)
        subs = [self.mask_of(w, table) for w in where[1:]]
        return self.and_(*subs) if head == "and" else self.or_(*subs)

    # ------------------------------------------------------------------ K3: where, K4: gather
    def where(self, where, table=None, row0: int = 0) -> torch.Tensor:
        """Ascending row ids (row0 + row) of the selected rows.  `where` = int8/bool mask tensor or a predicate tree.  (syncs)"""
        q, _ = self._query(where, [], table, None)
        q.row0 = row0
        ids = L.Ids()
        self._xcheck(self.lib.rfx_exec_where(self._x, C.byref(q), C.byref(ids)), "where")
        owner = _Owner(self, ids, self.lib.rfx_exec_ids_free)
        if ids.nshards == 1:
            return self._view(owner, ids.d_ids[0], int(ids.total), torch.int64)
        out, at = self.empty(int(ids.total)), 0
        for s in range(ids.nshards):  # shard order = row order
            if ids.count[s]:
                L.check(self.lib.rfx_hip_d2d(self._ctx, out.data_ptr() + at * 8, C.c_void_p(ids.d_ids[s]), ids.count[s] * 8), "d2d")
                at += ids.count[s]
        self.sync()
        return out

    def at_ids(self, col: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        self._check_col(col)
        self._check_col(ids)
        if ids.dtype != torch.int64:
            raise RfxError("ids must be i64")
        _ctype_of(col)
        out = torch.empty(ids.numel(), dtype=col.dtype, device=self.device)
        L.check(self.lib.rfx_hip_gather(self._ctx, col.data_ptr(), ids.data_ptr(), ids.numel(), out.data_ptr()), "gather")
        return out

    def sort_index(self, columns, descending: bool = False, over_shards: bool = False) -> torch.Tensor:
        """The stable order of the rows by ``columns`` (one device column or a sequence, the first most significant; all ascending or all
        descending) as an i64 device column: iasc / idesc, and the permutation behind xasc / xdesc (rfx_exec_sort).  Columns are int64 /
        float64, or the narrow key types int32 (INT32_MIN is the null: first ascending), int16, uint8 and bool (ordered as bytes), which sort
        as packed 8-byte records; a sequence may mix them.
        ``over_shards`` on an engine of several shards: every shard sorts its rows, one stable multiway merge (rfx_exec_sort_shards) -- the
        same answer bit for bit, int64 / float64 columns only; without it a sharded engine refuses ("sort over a sharded table")."""
        cols = [columns] if isinstance(columns, torch.Tensor) else list(columns)
        if not cols:
            raise RfxError("sort_index needs at least one column")
        n = cols[0].numel()
        for c in cols:
            self._check_col(c, n)
        types = (C.c_int32 * len(cols))(*[_sort_type_of(c) for c in cols])
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        if over_shards and self.shards > 1:
            _no_narrow_over_shards(cols)
            self._sort_shards(cols, types, descending, n, out.data_ptr(), None)
            return out
        ptrs = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
        self._xcheck(self.lib.rfx_exec_sort(self._x, ptrs, types, len(cols), int(bool(descending)), n, out.data_ptr()), "sort")
        return out

    def sort_values(self, col: torch.Tensor, descending: bool = False, over_shards: bool = False) -> torch.Tensor:
        """asc / desc: the column's own cells in sorted order, in the column's dtype (rfx_exec_sort_values; column types and ``over_shards``
        as for sort_index)."""
        self._check_col(col)
        out = torch.empty_like(col)
        if over_shards and self.shards > 1:
            _no_narrow_over_shards([col])
            self._sort_shards([col], (C.c_int32 * 1)(_ctype_of(col)), descending, col.numel(), None, out.data_ptr())
            return out
        self._xcheck(self.lib.rfx_exec_sort_values(self._x, col.data_ptr(), _sort_type_of(col), int(bool(descending)), col.numel(), out.data_ptr(), None), "sort")
        return out

    def _sort_shards(self, cols, types, descending, n, d_perm, d_values):
        qcols = (L.QCol * len(cols))()
        for k, c in enumerate(cols):
            pieces = self._pieces(c)
            for s in range(self.shards):
                qcols[k].d[s] = pieces[s]
        self._operands_written()
        self._xcheck(self.lib.rfx_exec_sort_shards(self._x, qcols, types, len(cols), int(bool(descending)), n, d_perm, d_values), "sort")

    def merge_runs(self, runs, types, descending: bool = False, tile: int = 0, want_perm: bool = True, want_values: bool = False):
        """The flat merge kernel (rfx_hip_merge_runs): ``runs`` = [(key columns in the run's sorted order, rows or None, row0)], ``types`` the key
        columns' RFX_I64 / RFX_F64.  Returns (permutation or None, merged cells of the one key column or None)."""
        arr = (L.MergeRun * len(runs))()
        n = 0
        for r, (keys, rows, row0) in enumerate(runs):
            for k, col in enumerate(keys):
                arr[r].d_keys[k] = col.data_ptr() if col.numel() else None
            arr[r].d_rows = rows.data_ptr() if rows is not None and rows.numel() else None
            arr[r].len = keys[0].numel()
            arr[r].row0 = int(row0)
            n += keys[0].numel()
        perm = torch.empty(n, dtype=torch.int64, device=self.device) if want_perm else None
        vals = torch.empty(n, dtype=torch.int64, device=self.device) if want_values else None
        self._operands_written()
        L.check(self.lib.rfx_hip_merge_runs(self._ctx, arr, len(runs), (C.c_int32 * len(types))(*types), len(types), int(bool(descending)), int(tile),
                                            perm.data_ptr() if want_perm else None, vals.data_ptr() if want_values else None), "merge_runs")
        self.sync()
        return perm, vals

    # ------------------------------------------------------------------ bucket verbs (rfx_bucket.hip through rfx_exec_bucket.c)
    _BK_TYPES = {"i32": 4, "i64": 5, "date": 7, "time": 8, "timestamp": 9, "f64": 10}  # the reference's type codes
    _BK_DTYPE = {4: torch.int32, 7: torch.int32, 8: torch.int32, 5: torch.int64, 9: torch.int64, 10: torch.float64}

    def _pieces(self, t: torch.Tensor):
        """Per shard the address of its rows (rfx_exec_split) of a whole device tensor."""
        out = (C.c_void_p * L.RFX_MAX_SHARDS)()
        for s in range(self.shards):
            r0 = C.c_int64()
            self.lib.rfx_exec_split(t.numel(), self.shards, s, C.byref(r0), None)
            out[s] = t.data_ptr() + r0.value * t.element_size()
        return out

    def _operands_written(self):
        """Before an element-wise map over more than one shard: shards 1.. run on streams of their own, which do not wait for torch's stream, so what
        torch enqueued there -- the kernels that made the operands -- has to have finished (as in _query)."""
        if self.shards > 1:
            torch.cuda.current_stream(self.device).synchronize()

    def xrank(self, col: torch.Tensor, n: int, attr: Optional[str] = None) -> torch.Tensor:
        """(xrank col n): per cell the bucket in [0, n) of its rank under the stable ascending sort, (rank * n) // len (rfx_exec_xrank).  ``attr`` =
        "asc" / "desc": the column carries that attribute, the index formula alone runs.  One shard."""
        self._check_col(col)
        out = torch.empty(col.numel(), dtype=torch.int64, device=self.device)
        attrs = {None: 0, "asc": L.RFX_XRANK_ASC, "desc": L.RFX_XRANK_DESC}[attr]
        self._xcheck(self.lib.rfx_exec_xrank(self._x, col.data_ptr(), _ctype_of(col), attrs, col.numel(), int(n), out.data_ptr()), "xrank")
        return out

    def xbar(self, x, y, xtype: Optional[str] = None, ytype: Optional[str] = None) -> torch.Tensor:
        """(xbar x y), ray_xbar_partial's arms: an operand is a device column (int32 / int64 / float64) or a Python atom; ``xtype`` / ``ytype`` name
        the reference's type where the dtype does not ("date", "time", "timestamp"; an int atom is "i64", or "i32" / "time" ... when said so)."""
        import struct
        d = L.XbarDesc()
        codes, tens = [], []
        for v, name in ((x, xtype), (y, ytype)):
            if isinstance(v, torch.Tensor):
                self._check_col(v)
                code = self._BK_TYPES[name] if name else {torch.int32: 4, torch.int64: 5, torch.float64: 10}.get(v.dtype)
                if code is None or self._BK_DTYPE[code] != v.dtype:
                    raise RfxError(f"xbar: a {v.dtype} column cannot be {name or 'an operand'}")
                tens.append(v)
            else:
                code = self._BK_TYPES[name] if name else (10 if isinstance(v, float) else 5)
                tens.append(None)
            codes.append(code)
        if tens[0] is None and tens[1] is None:
            raise RfxError("xbar: at least one operand is a column")
        if tens[0] is not None and tens[1] is not None and tens[0].numel() != tens[1].numel():
            raise RfxError("length")
        ot = C.c_int()
        if self.lib.rfx_exec_xbar_plan(codes[0], codes[1], C.byref(d), C.byref(ot)) != L.RFX_OK:
            raise RfxError(f"xbar: the reference has no arm for the types {codes[0]} and {codes[1]}")
        bits = []
        for v, code in zip((x, y), codes):
            if isinstance(v, torch.Tensor):
                bits.append(0)
            elif code == 10:
                bits.append(struct.unpack("<Q", struct.pack("<d", float(v)))[0])
            else:
                bits.append(int(v) & (0xFFFFFFFF if self._BK_DTYPE[code] == torch.int32 else 0xFFFFFFFFFFFFFFFF))
        d.x_atom, d.y_atom = bits
        n = (tens[0] if tens[0] is not None else tens[1]).numel()
        out = torch.empty(n, dtype=self._BK_DTYPE[ot.value], device=self.device)
        xs = self._pieces(tens[0]) if tens[0] is not None else None
        ys = self._pieces(tens[1]) if tens[1] is not None else None
        self._operands_written()
        self._xcheck(self.lib.rfx_exec_xbar(self._x, C.byref(d), xs, ys, n, self._pieces(out), -1), "xbar")
        return out

    def within(self, col: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
        """(within col [lo hi]) over an i64 column: a B8 mask (int8 tensor of 0 / 1), lo <= x <= hi as plain signed compares."""
        self._check_col(col)
        if col.dtype != torch.int64:
            raise RfxError("within: an i64 column is expected")
        out = torch.empty(col.numel(), dtype=torch.int8, device=self.device)
        self._operands_written()
        self._xcheck(self.lib.rfx_exec_within(self._x, self._pieces(col), int(lo), int(hi), col.numel(), self._pieces(out), -1), "within")
        return out

    def _round(self, op: int, col: torch.Tensor, what: str) -> torch.Tensor:
        self._check_col(col)
        if col.dtype != torch.float64:
            raise RfxError(f"{what}: an f64 column is expected")
        out = torch.empty_like(col)
        self._operands_written()
        self._xcheck(self.lib.rfx_exec_round(self._x, op, self._pieces(col), col.numel(), self._pieces(out), -1), what)
        return out

    def floor(self, col: torch.Tensor) -> torch.Tensor: return self._round(L.RFX_ROUND_FLOOR, col, "floor")
    def ceil(self, col: torch.Tensor) -> torch.Tensor: return self._round(L.RFX_ROUND_CEIL, col, "ceil")
    def round(self, col: torch.Tensor) -> torch.Tensor: return self._round(L.RFX_ROUND_ROUND, col, "round")

    def neg(self, col: torch.Tensor) -> torch.Tensor:
        """(neg col): int32 / int64 columns answer i64, float64 answers f64 (ray_neg's vector arms)."""
        self._check_col(col)
        t = {torch.int32: L.RFX_I32, torch.int64: L.RFX_I64, torch.float64: L.RFX_F64}.get(col.dtype)
        if t is None:
            raise RfxError(f"neg: unsupported dtype {col.dtype}")
        out = torch.empty(col.numel(), dtype=torch.float64 if t == L.RFX_F64 else torch.int64, device=self.device)
        self._operands_written()
        self._xcheck(self.lib.rfx_exec_neg(self._x, t, self._pieces(col), col.numel(), self._pieces(out), -1), "neg")
        return out

    # ------------------------------------------------------------------ cast (rfx_cast.hip through rfx_exec_cast.c)
    _CAST_DTYPE = {1: torch.int8, 2: torch.uint8, 3: torch.int16, 4: torch.int32, 5: torch.int64, 7: torch.int32, 8: torch.int32, 9: torch.int64, 10: torch.float64}
    _CAST_OF_DTYPE = {torch.int8: 1, torch.bool: 1, torch.uint8: 2, torch.int16: 3, torch.int32: 4, torch.int64: 5, torch.float64: 10}

    def cast(self, col: torch.Tensor, to: str, frm: Optional[str] = None) -> torch.Tensor:
        """(as 'to col): a uint8 / int8 / int16 / int32 / int64 / float64 device column cast to the type ``to`` names ("b8" "u8" "i16" "i32" "i64" "f64"
        "date" "time" "timestamp", either case), one C cast per cell as the reference does it, nulls not carried.  ``frm`` names the column's reference
        type where the dtype does not (an int32 column is "i32" unless it is "date" / "time", an int64 one "i64" unless "timestamp", int8 "b8", uint8
        "u8").  -> a tensor of the target's storage dtype (b8 int8, u8 uint8); the same type answers ``col`` itself."""
        if isinstance(col, torch.Tensor) and col.dtype == torch.bool:
            col = col.view(torch.int8)
        self._check_col(col)
        dst = L.RFX_CAST.get(str(to).lower())
        if dst is None:
            raise RfxError(f"cast: {to!r} names none of the nine numeric and temporal types")
        src = L.RFX_CAST.get(str(frm).lower()) if frm is not None else self._CAST_OF_DTYPE.get(col.dtype)
        if src is None or self._CAST_DTYPE[src] != col.dtype:
            raise RfxError(f"cast: a {col.dtype} column cannot be {frm or 'cast'}")
        if src == dst:
            return col
        out = torch.empty(col.numel(), dtype=self._CAST_DTYPE[dst], device=self.device)
        if col.numel() == 0:
            return out
        if not self.lib.rfx_hip_cast_arm(src, dst):
            raise RfxError(f"cast: the reference has no cast from type {src} to type {dst}")
        if col.data_ptr() % 16:  # (a view into a larger tensor: the kernel moves 16-byte accesses)
            col = col.clone()
        self._operands_written()
        self._xcheck(self.lib.rfx_exec_cast(self._x, src, dst, self._pieces(col), col.numel(), self._pieces(out), -1), "cast")
        return out

    # ------------------------------------------------------------------ row verbs (rfx_rows.hip through rfx_exec_rows.c)
    _ROW_TYPESTR = {torch.int64: "<i8", torch.float64: "<f8", torch.int32: "<i4", torch.int8: "|i1"}

    def _row_source(self, t: torch.Tensor, n: Optional[int] = None):
        """A column of a row verb -> (the tensor the kernels read, its cell kind, the result's dtype): i64 / f64 cells as they are, int8 (bool) bytes,
        an int32 column through its widened 8-byte copy (rfx_hip_widen_i32), answered in 4-byte cells again."""
        if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
            t = t.view(torch.int8)
        self._check_col(t, n)
        if t.dtype in (torch.int64, torch.float64):
            return t, L.RFX_ROWS_8, t.dtype
        if t.dtype == torch.int8:
            return t, L.RFX_ROWS_1, t.dtype
        if t.dtype == torch.int32:
            wide = torch.empty(t.numel(), dtype=torch.int64, device=self.device)
            L.check(self.lib.rfx_hip_widen_i32(self._ctx, t.data_ptr(), t.numel(), wide.data_ptr()), "widen_i32")
            return wide, L.RFX_ROWS_4W, t.dtype
        raise RfxError(f"unsupported column dtype {t.dtype} (the row verbs take int64, float64, int32 and int8 / bool columns)")

    def _row_view(self, owner, ptr, n: int, dtype) -> torch.Tensor:
        if not n or not ptr:
            return self.empty(0, dtype)
        return torch.as_tensor(_View(owner, ptr, n, self._ROW_TYPESTR[dtype]), device=self.device)

    def filter(self, columns, where, table=None, form: Optional[str] = None):
        """(filter x mask) / the rows a where: selects: ``columns`` is one device column or a dict of them, ``where`` a B8 mask tensor or a predicate
        tree exactly as Engine.where takes it -- the fused pass feeds the ordered compaction with no mask and no ids in between (rfx_exec_filter).
        Runs over every shard's rows.  ``form``: None (what ships), "direct" or "ring" -- the compaction's write-out (measurements).  (syncs)"""
        single = isinstance(columns, torch.Tensor)
        cols = {"": columns} if single else dict(columns)
        if not cols:
            raise RfxError("filter: no columns")
        n = next(iter(cols.values())).numel()
        if form not in (None, "direct", "ring"):
            raise RfxError(f"filter: unknown write-out form {form!r}")
        flags = {None: 0, "direct": L.RFX_Q_ROWS_DIRECT, "ring": L.RFX_Q_ROWS_RING}[form]
        q, _ = self._query(where, [], table, n, flags=flags)
        srcs = [self._row_source(t, n) for t in cols.values()]
        self._operands_written()
        pieces = (L.QCol * len(srcs))()
        kinds = (C.c_int32 * len(srcs))()
        for k, (t, kind, _dt) in enumerate(srcs):
            addr = self._pieces(t)
            for s in range(self.shards):
                pieces[k].d[s] = addr[s]
            kinds[k] = kind
        rows = L.Rows()
        self._xcheck(self.lib.rfx_exec_filter(self._x, C.byref(q), pieces, kinds, len(srcs), C.byref(rows)), "filter")
        owner = _Owner(self, rows, self.lib.rfx_exec_rows_free)
        total, out = int(rows.total), []
        for k, (_t, kind, dt) in enumerate(srcs):
            if rows.nshards == 1:
                out.append(self._row_view(owner, self.lib.rfx_exec_rows_piece(C.byref(rows), 0, k), total, dt))
                continue
            o, at = self.empty(total, dt), 0
            for s in range(rows.nshards):  # shard order = row order
                if rows.count[s]:
                    L.check(self.lib.rfx_hip_d2d(self._ctx, o.data_ptr() + at, C.c_void_p(self.lib.rfx_exec_rows_piece(C.byref(rows), s, k)), rows.count[s] * kind), "d2d")
                    at += rows.count[s] * kind
            out.append(o)
        if rows.nshards > 1:
            self.sync()
        return out[0] if single else dict(zip(cols.keys(), out))

    @staticmethod
    def _take_window(l: int, count):
        """ray_take's count (core/items.c:405-445) -> (first cell, cells): an int takes |count| cells cyclically, from the end when negative; a
        (start, amount) pair takes a range clamped to the cells there are, a negative start counting from the end."""
        if isinstance(count, (tuple, list)):
            if len(count) != 2 or int(count[1]) < 0:
                raise RfxError("take: a range is (start, amount) with amount >= 0")  # reference: err_length
            start, m = int(count[0]), int(count[1])
            if start < 0:
                start += l
            start = min(max(start, 0), l)
            m = min(m, l - start)
            return (start if m else 0), m
        c = int(count)
        if l == 0:
            raise RfxError("take from an empty column")  # (the reference divides by the length)
        m = abs(c)
        return ((l - m % l) % l if c < 0 else 0), m

    def take(self, columns, count, dtype=None):
        """(take from count): ``columns`` is one device column, a dict of them, or a Python number (an atom, broadcast as ``dtype``: int64 / float64 /
        int32 / int8); ``count`` an int or a (start, amount) pair.  One shard (rfx_exec_take)."""
        if isinstance(columns, (int, float, bool)):
            import struct
            dt = dtype or (torch.float64 if isinstance(columns, float) else torch.int64)
            if isinstance(count, (tuple, list)) and len(count) != 2:
                raise RfxError("take: a range is (start, amount) with amount >= 0")
            m = abs(int(count)) if not isinstance(count, (tuple, list)) else int(count[1])
            if dt not in self._ROW_TYPESTR or m < 0:
                raise RfxError("take: an atom is broadcast as int64, float64, int32 or int8, a non-negative number of times")
            out = self.empty(m, dt)
            fmt = {torch.int64: "<q", torch.float64: "<d", torch.int32: "<i", torch.int8: "<b"}[dt]
            bits = int.from_bytes(struct.pack(fmt, float(columns) if dt == torch.float64 else int(columns)), "little")
            if m:
                self._xcheck(self.lib.rfx_exec_take_atom(self._x, out.element_size(), bits, m, out.data_ptr()), "take")
            return out
        single = isinstance(columns, torch.Tensor)
        cols = {"": columns} if single else dict(columns)
        if not cols:
            raise RfxError("take: no columns")
        l = next(iter(cols.values())).numel()
        j0, m = self._take_window(l, count)
        srcs = [self._row_source(t, l) for t in cols.values()]
        outs = [self.empty(m, dt) for _t, _k, dt in srcs]
        if m:
            ptrs = (C.c_void_p * len(srcs))(*[t.data_ptr() for t, _k, _d in srcs])
            kinds = (C.c_int32 * len(srcs))(*[k for _t, k, _d in srcs])
            optrs = (C.c_void_p * len(srcs))(*[o.data_ptr() for o in outs])
            self._xcheck(self.lib.rfx_exec_take(self._x, ptrs, kinds, len(srcs), l, j0, m, optrs), "take")
        return outs[0] if single else dict(zip(cols.keys(), outs))

    def reverse(self, col: torch.Tensor) -> torch.Tensor:
        """(reverse col): the column's cells last to first (rfx_exec_reverse).  One shard."""
        t, kind, dt = self._row_source(col)
        out = self.empty(t.numel(), dt)
        if t.numel():
            self._xcheck(self.lib.rfx_exec_reverse(self._x, t.data_ptr(), kind, t.numel(), out.data_ptr()), "reverse")
        return out

    # ------------------------------------------------------------------ concat, raze (rfx_concat.hip through rfx_exec_concat.c)
    _CONCAT_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float64)

    def _concat_cols(self, columns):
        """columns: per result column a list of parts (device tensors of one dtype, or Python numbers: atoms) -> one fresh tensor per column, every column
        ONE multi-span copy, RFX_MAX_COLS columns to a launch (rfx_exec_concat_cols).  One shard."""
        import struct
        descs = (L.ConcatCol * len(columns))()
        outs, keep = [], []
        for k, parts in enumerate(columns):
            tens = [p.view(torch.int8) if isinstance(p, torch.Tensor) and p.dtype == torch.bool else p for p in parts]
            dts = {p.dtype for p in tens if isinstance(p, torch.Tensor)}
            if len(dts) != 1 or next(iter(dts)) not in self._CONCAT_DTYPES:
                raise RfxError("concat / raze: the parts of a column are tensors of one dtype among int8 (bool), uint8, int16, int32, int64, float64")
            dt = next(iter(dts))
            spans = (L.Span * len(tens))()
            total = 0
            for i, p in enumerate(tens):
                if isinstance(p, torch.Tensor):
                    self._check_col(p)  # (a view t[j:] is contiguous: its cells are cell-aligned, which is all the kernel asks)
                    spans[i].d_ptr, spans[i].cells = (p.data_ptr() if p.numel() else None), p.numel()
                else:
                    fmt = {torch.int64: "<q", torch.float64: "<d", torch.int32: "<i", torch.int16: "<h", torch.int8: "<b", torch.uint8: "<B"}[dt]
                    spans[i].d_ptr, spans[i].cells = None, 1
                    spans[i].bits = int.from_bytes(struct.pack(fmt, float(p) if dt == torch.float64 else int(p)), "little")
                total += spans[i].cells
            out = self.empty(total, dt)
            descs[k].spans, descs[k].nspans, descs[k].width, descs[k].d_out = spans, len(tens), out.element_size(), (out.data_ptr() if total else None)
            outs.append(out)
            keep.append(spans)
        if any(o.numel() for o in outs):
            self._xcheck(self.lib.rfx_exec_concat_cols(self._x, descs, len(columns)), "concat")
        return outs

    def concat(self, a, b):
        """(concat a b): two device columns of one dtype, a column and a Python number (an atom of the column's type, on either side), or two dicts of
        columns with the same names as tables -- b's columns are taken in a's name order, the result carries a's names.  -> fresh tensors."""
        if isinstance(a, dict) or isinstance(b, dict):
            if not (isinstance(a, dict) and isinstance(b, dict)) or not a or set(a) != set(b):
                raise RfxError("concat: tables whose name sets differ")  # reference: err_value
            return dict(zip(a.keys(), self._concat_cols([[a[n], b[n]] for n in a])))
        if not isinstance(a, torch.Tensor) and not isinstance(b, torch.Tensor):
            raise RfxError("concat: an atom with an atom")
        return self._concat_cols([[a, b]])[0]

    def raze(self, parts):
        """(raze (list v1 v2 ...)): one or more device columns of one dtype, empties among them included, end to end.  -> a fresh tensor."""
        parts = list(parts)
        if not parts or not all(isinstance(p, torch.Tensor) for p in parts):
            raise RfxError("raze: a non-empty list of device columns")
        return self._concat_cols([parts])[0]

    # ------------------------------------------------------------------ upsert, insert (rfx_upsert.hip through rfx_exec_upsert.c)
    def _upsert(self, table, nkeys, batch, verb):
        names = list(table)
        if not names:
            raise RfxError(f"{verb}: a table with no columns")
        tcols = [self._check_col(table[k].view(torch.int8) if table[k].dtype == torch.bool else table[k]) for k in names]
        n = tcols[0].numel()
        if any(c.numel() != n for c in tcols) or any(c.dtype not in self._CONCAT_DTYPES for c in tcols):
            raise RfxError(f"{verb}: table columns are equally long tensors of int8 (bool), uint8, int16, int32, int64 or float64")
        by_name = isinstance(batch, dict)
        if by_name:  # the DICT / TABLE form: any name order, a missing column is a null vector (matched rows take it too)
            if not batch or any(k not in table for k in batch):
                raise RfxError(f"{verb}: a batch name the table does not have")  # reference: err_value
            given = [batch.get(k) for k in names]
        else:  # the LIST form: the first l columns; the others keep their matched rows and append their null
            given = list(batch) + [None] * (len(names) - len(batch))
            if not batch or len(batch) > len(names) or (not nkeys and len(batch) < len(names)):
                raise RfxError(f"{verb}: a LIST batch has 1 .. p columns (insert: all p)")  # reference: err_length / a ragged table
        given = [self._check_col(b.view(torch.int8) if b.dtype == torch.bool else b) if b is not None else None for b in given]
        lens = {b.numel() for b in given if b is not None}
        if len(lens) != 1 or 0 in lens:
            raise RfxError(f"{verb}: batch columns of one length >= 1")
        m = lens.pop()
        if nkeys and any(c.dtype == torch.uint8 for c in tcols):
            raise RfxError("upsert: a uint8 column (the reference answers a LIST column)")
        if nkeys > min(len(names), L.RFX_MAX_KEYS) or (nkeys < 1 and verb == "upsert"):
            raise RfxError("upsert: 1 .. 8 keys, no more than the table has columns")
        descs = (L.UpsertXCol * len(names))()
        keep = []
        for i, (t, b) in enumerate(zip(tcols, given)):
            if b is not None and b.dtype != t.dtype:
                raise RfxError(f"{verb}: a batch column that is not of its column's dtype")
            if i < nkeys and (b is None or t.dtype != torch.int64):
                raise RfxError("upsert: key columns are int64 and the batch provides them")
            null = {torch.int64: 1 << 63, torch.float64: 0x7FF8000000000000}.get(t.dtype, 0)
            if b is None and not by_name and t.dtype in (torch.uint8, torch.int16, torch.int32):
                raise RfxError(f"{verb}: a column not provided whose null is not a cell of its type")  # (the reference answers a LIST column)
            if b is None and by_name and nkeys:
                b = torch.full((m,), 0, dtype=t.dtype, device=self.device)
                L.check(self.lib.rfx_hip_upsert_fill(self._ctx, b.data_ptr(), b.element_size(), null, m), "upsert_fill")
            keep.append(b)
            descs[i].d_table, descs[i].d_batch = (t.data_ptr() if n else None), (b.data_ptr() if b is not None else None)
            descs[i].width, descs[i].null_bits = t.element_size(), null
            descs[i].role = L.RFX_UPSERT_KEY if i < nkeys else (L.RFX_UPSERT_VALUE if b is not None else L.RFX_UPSERT_ABSENT)
        a, dest = m, None
        if nkeys:
            idx, dest = self.empty(m, torch.int64), self.empty(m, torch.int64)
            tk = (C.c_void_p * nkeys)(*[descs[i].d_table for i in range(nkeys)])
            bk = (C.c_void_p * nkeys)(*[descs[i].d_batch for i in range(nkeys)])
            undefined, appended = C.c_int(0), C.c_int64(0)
            self._xcheck(self.lib.rfx_exec_upsert_index(self._x, tk, bk, nkeys, n, m, idx.data_ptr(), C.byref(undefined)), "upsert index")
            self._xcheck(self.lib.rfx_exec_upsert_plan(self._x, idx.data_ptr(), m, n, dest.data_ptr(), C.byref(appended)), "upsert plan")
            a = int(appended.value)
            if a < m and any(d.role == L.RFX_UPSERT_VALUE and d.width != 8 for d in descs):
                raise RfxError("upsert: a matched row for a 1-, 2- or 4-byte value column (the reference answers a LIST column)")
        outs = [self.empty(n + a, t.dtype) for t in tcols]
        for i, o in enumerate(outs):
            descs[i].d_out = o.data_ptr()
        if nkeys:
            self._xcheck(self.lib.rfx_exec_upsert_cols(self._x, descs, len(names), dest.data_ptr(), m, n, a), "upsert")
        else:
            self._xcheck(self.lib.rfx_exec_insert_cols(self._x, descs, len(names), m, n), "insert")
        return dict(zip(names, outs))

    def upsert(self, table_columns, nkeys: int, batch_columns) -> Dict[str, torch.Tensor]:
        """``(upsert t nkeys batch)``: ``table_columns`` a dict of equally long device columns whose first ``nkeys`` are the int64 key; ``batch_columns`` a
        list of the first l columns' tensors (the others keep their matched rows and append their null) or a dict by name in any order (a missing
        column is a null vector: matched rows take the null too).  A batch row whose key tuple equals a table row overwrites the FIRST such row's
        value columns, the last such batch row winning; every other batch row is appended in order.  -> a dict of fresh tensors, the table's names."""
        return self._upsert(table_columns, int(nkeys), batch_columns, "upsert")

    def insert(self, table_columns, batch_columns) -> Dict[str, torch.Tensor]:
        """``(insert t batch)``: every batch row appended; the batch as for upsert, a list giving every column.  -> a dict of fresh tensors."""
        return self._upsert(table_columns, 0, batch_columns, "insert")

    # ------------------------------------------------------------------ row, collect (rfx_collect.hip through rfx_exec_collect.c)
    def _partition(self, gid: torch.Tensor, groups: int):
        gid = self._check_col(gid)
        if gid.dtype != torch.int64:
            raise RfxError("partition: group ids are int64")
        part = L.Partition()
        m = gid.numel()
        self._xcheck(self.lib.rfx_exec_group_partition(self._x, gid.data_ptr() if m else None, m, int(groups), C.byref(part)), "partition")
        return part, _Owner(self, part, self.lib.rfx_exec_group_partition_free)

    def partition(self, gid: torch.Tensor, groups: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The stable partition of the positions 0 .. m-1 by their dense group id ``gid[i]`` in [0, groups) -> (offsets, perm): ``perm`` the positions
        ordered by (group, position), group g's at ``perm[offsets[g]:offsets[g + 1]]`` (rfx_exec_group_partition).  An id outside [0, groups) is refused
        before anything is placed.  One shard.  (syncs)"""
        part, own = self._partition(gid, groups)
        return self._view(own, part.d_offsets, int(groups) + 1, torch.int64), self._view(own, part.d_perm, int(part.m), torch.int64)

    _COLLECT_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float64)

    def partition_collect(self, gid: torch.Tensor, groups: int, columns, rows: Optional[torch.Tensor] = None, outs=None, want_rows: bool = False,
                          col_len: Optional[int] = None):
        """The two primitives over the caller's own group ids: partition ``gid`` (one id per element), then ``outs[k][j] = columns[k][src(j)]`` with
        ``src(j) = rows[perm[j]]`` under a filter's row ids, else ``perm[j]`` -> (offsets, [cells per column], rows or None).  ``outs``: the caller's
        own result tensors (cell-aligned views included), else fresh ones.  (syncs)"""
        cols = [self._check_col(c.view(torch.int8) if c.dtype == torch.bool else c) for c in columns]
        if any(c.dtype not in self._COLLECT_DTYPES for c in cols) or len({c.numel() for c in cols}) > 1:
            raise RfxError("collect: columns are equally long tensors of int8 (bool), uint8, int16, int32, int64 or float64")
        part, own = self._partition(gid, groups)
        m = int(part.m)
        if rows is not None and (self._check_col(rows, m).dtype != torch.int64):
            raise RfxError("collect: row ids are int64")
        n = cols[0].numel() if cols else (m if col_len is None else int(col_len))  # (the cells a row id may name)
        outs = [self.empty(m, c.dtype) for c in cols] if outs is None else [self._check_col(o, m) for o in outs]
        if len(outs) != len(cols) or any(o.dtype != c.dtype for o, c in zip(outs, cols)):
            raise RfxError("collect: one result of its column's dtype per column")
        rows_out = self.empty(m) if want_rows else None
        nc = len(cols)
        self._xcheck(self.lib.rfx_exec_group_collect(self._x, C.byref(part), rows.data_ptr() if rows is not None and m else None, n,
                                                     (C.c_void_p * max(1, nc))(*[c.data_ptr() for c in cols]), (C.c_int32 * max(1, nc))(*[c.element_size() for c in cols]),
                                                     nc, (C.c_void_p * max(1, nc))(*[o.data_ptr() for o in outs]), int(want_rows),
                                                     rows_out.data_ptr() if want_rows and m else None), "collect")
        self.sync()
        return self._view(own, part.d_offsets, int(groups) + 1, torch.int64), outs, rows_out

    def _group_members(self, key, columns, where, table, want_rows: bool):
        if self.shards > 1:  # (the planner's own refusal, before anything else runs)
            self._xcheck(self.lib.rfx_exec_group_partition(self._x, None, 0, 0, C.byref(L.Partition())), "partition")
        from . import joins
        k = self._check_col(self._resolve(key, table))
        if k.dtype != torch.int64:
            raise RfxError("group key must be i64 on this path")
        n = k.numel()
        names = list(columns)
        cols = [self._resolve(columns[c] if isinstance(columns, dict) else c, table) for c in names]
        cols = [self._check_col(c.view(torch.int8) if c.dtype == torch.bool else c, n) for c in cols]
        if any(c.dtype not in self._COLLECT_DTYPES for c in cols):
            raise RfxError("collect: columns are tensors of int8 (bool), uint8, int16, int32, int64 or float64")
        rows = self.where(where, table) if where is not None else None
        m = rows.numel() if rows is not None else n
        if m == 0:
            keys, gid = self.empty(0), self.empty(0)
        else:  # the groups in first-occurrence order, then every selected row's place among them: its key looked up in the groups' keys
            keys = self.group_by(key, [], where, table)["keys"]
            gid = joins.join_index(self, ["k"], {"k": self.at_ids(k, rows) if rows is not None else k}, {"k": keys})
        part, own = self._partition(gid, keys.numel())
        outs = [self.empty(m, c.dtype) for c in cols]
        rows_out = self.empty(m) if want_rows else None
        nc = len(cols)
        self._xcheck(self.lib.rfx_exec_group_collect(self._x, C.byref(part), rows.data_ptr() if rows is not None and m else None, n,
                                                     (C.c_void_p * max(1, nc))(*[c.data_ptr() for c in cols]), (C.c_int32 * max(1, nc))(*[c.element_size() for c in cols]),
                                                     nc, (C.c_void_p * max(1, nc))(*[o.data_ptr() for o in outs]), int(want_rows),
                                                     rows_out.data_ptr() if want_rows and m else None), "collect")
        self.sync()  # (the partition's blocks go back to the pool with `own`: nothing may still read them)
        return keys, self._view(own, part.d_offsets, keys.numel() + 1, torch.int64), dict(zip(names, outs)), rows_out

    def group_rows(self, key, where=None, table=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``select {r: (row c) by: key from: t [where: p]}`` in its device-resident form -> (keys, offsets, rows): the groups' keys in first-occurrence
        order, and group g's row numbers, ascending, at ``rows[offsets[g]:offsets[g + 1]]`` (aggr_row, core/aggr.c:3118-3136).  One shard.  (syncs)"""
        keys, offsets, _, rows = self._group_members(key, {}, where, table, True)
        return keys, offsets, rows

    def group_collect(self, key, columns, where=None, table=None):
        """``select {c: c ... by: key from: t [where: p]}``: every group's cells -> (keys, offsets, {name: cells}); ``columns`` a dict name -> device
        column, or a list of ``table``'s names; group g's cells of a column, in row order, at ``cells[offsets[g]:offsets[g + 1]]``, in the column's own
        dtype (aggr_collect, core/aggr.c:3021-3116).  Any number of columns: eight to a launch over one partition.  One shard.  (syncs)"""
        if not columns:
            raise RfxError("collect: at least one column")
        keys, offsets, cells, _ = self._group_members(key, columns, where, table, False)
        return keys, offsets, cells

    def eval_expr(self, expr, table=None) -> torch.Tensor:
        """``(op x y)`` / an expression tree over columns and atoms as a device column: ray_add .. ray_mod (binop_map,
        core/math.c:2280-2345) in ONE pass whatever the depth."""
        a = L.Agg()
        keep, self._keep = self._keep, []
        n = M.agg_expr(self, a, expr, table, None)
        out = torch.empty(n, dtype=torch.float64 if L.agg_input_type(a) == L.RFX_F64 else torch.int64, device=self.device)
        t = C.c_int32()
        L.check(self.lib.rfx_hip_eval_expr(self._ctx, C.byref(a), n, out.data_ptr(), C.byref(t)), "eval_expr")
        self._keep = keep
        return out

    def scope(self, key: torch.Tensor, where=None, table=None) -> Tuple[int, int, int]:
        """index_scope_i64 (core/index.c:376-435): (min, max, rows seen) of a key column through the predicates.  (syncs)"""
        self._keep.clear()
        logic, leaves, more = M.tree_leaves(self, where)
        parr, n = M.preds(self, leaves, more, table, self._check_col(key).numel())
        mn, mx, cnt = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.rfx_hip_scope_i64(self._ctx, key.data_ptr(), parr, len(leaves), logic, n, C.byref(mn), C.byref(mx), C.byref(cnt)), "scope_i64")
        return int(mn.value), int(mx.value), int(cnt.value)

    def row_hash(self, kcols, value_first: bool = False) -> torch.Tensor:
        """The reference's row hash of the key tuples (__index_list_precalc_hash, core/index.c:274-309) as one i64 column."""
        k, n = len(kcols), kcols[0].numel()
        out = self.empty(n)
        ptrs = (C.c_void_p * k)(*[kc.data_ptr() for kc in kcols])
        L.check(self.lib.rfx_hip_row_hash(self._ctx, ptrs, k, n, int(value_first), out.data_ptr()), "row_hash")
        return out

    # ------------------------------------------------------------------ group-by (K6-K10): the planner's
    def group_by(self, key, aggs, where=None, table=None, order: str = "first", flags: int = 0, probe_first: bool = False):
        """``select {aggs} from t [where p] by key`` -> dict(groups=, keys=, first=, results=[...], dense=, cap=, path=[, key_columns=]) of
        device tensors, groups in first-occurrence order (`order="radix"`, key tuples on the row-hash path only: the order of the
        reference's multi-threaded radix grouping -- hash & 1023, then first occurrence, core/index.c:2465-2729).  (syncs)"""
        keys = list(key) if isinstance(key, (list, tuple)) and not (isinstance(key, tuple) and len(key) == 3 and key[0] == "xbar") else [key]
        q, n = self._query(where, aggs, table, None, keys, flags | L.RFX_Q_WANT_FIRST | (L.RFX_Q_PROBE_FIRST if probe_first else 0))
        g = L.Groups()
        self._xcheck(self.lib.rfx_exec_group_by(self._x, C.byref(q), C.byref(g)), "group_by")
        own = _Owner(self, g, self.lib.rfx_exec_groups_free)
        ng = int(g.groups)
        res = [self._view(own, g.d_results[a], ng, torch.float64 if g.result_type[a] == L.RFX_F64 else torch.int64) for a in range(len(aggs))] if ng else \
              [self.empty(0, torch.float64 if (fn == "avg" or (fn != "count" and col is not None and self._arg_f64(col, table))) else torch.int64) for fn, col in aggs]
        r = dict(groups=ng, keys=self._view(own, g.d_keys, ng, torch.int64), first=self._view(own, g.d_first, ng, torch.int64), results=res,
                 dense=g.path in (L.RFX_PATH_DENSE, L.RFX_PATH_DENSE_SMALL), cap=int(g.capacity), path=int(g.path))
        if len(keys) > 1:
            r["key_columns"] = [self._view(own, g.d_keycols[i], ng, torch.int64) for i in range(len(keys))]
        if probe_first and g.d_probe:
            r["probe"] = self._view(own, g.d_probe, n, torch.int64)
        if order == "radix" and r["groups"] > 1 and r["path"] == L.RFX_PATH_ROWHASH:  # a different ORDER of the same groups, for the golden sets of that arm
            perm = torch.argsort((r["keys"] & 1023) * (1 << 40) + torch.argsort(torch.argsort(r["first"])), stable=True)
            r["keys"], r["first"] = r["keys"][perm], r["first"][perm]
            r["results"] = [x[perm] for x in r["results"]]
            r["key_columns"] = [x[perm] for x in r["key_columns"]]
        return r

    def group_dev(self, key, col, where=None, table=None, flags: int = 0):
        """``(dev col)`` per group of ``select ... from t [where p] by key`` -> dict(groups=, keys=, dev=) of device tensors, groups in
        first-occurrence order: aggr_dev's rule (core/aggr.c:2250-2350,2864-2929) -- NaN for a group without a non-null cell, 0.0 for one
        cell, else sqrt(max(0, sq/n - (s/n)^2)) (rfx_exec_group_dev).  One shard.  (syncs)"""
        keys = list(key) if isinstance(key, (list, tuple)) and not (isinstance(key, tuple) and len(key) == 3 and key[0] == "xbar") else [key]
        c = self._resolve(col, table)
        q, n = self._query(where, [], table, None, keys, flags)
        c = self._check_col(c, n)
        self._keep.append(c)
        g = L.Groups()
        self._xcheck(self.lib.rfx_exec_group_by(self._x, C.byref(q), C.byref(g)), "group_by")
        own = _Owner(self, g, self.lib.rfx_exec_groups_free)
        ng = int(g.groups)
        out = torch.empty(ng, dtype=torch.float64, device=self.device)
        self._xcheck(self.lib.rfx_exec_group_dev(self._x, C.byref(q), C.byref(g), c.data_ptr(), _ctype_of(c), out.data_ptr()), "group_dev")
        return dict(groups=ng, keys=self._view(own, g.d_keys, ng, torch.int64), dev=out, path=int(g.path))

    def _arg_f64(self, col, table) -> bool:
        """Element type of an aggregate's argument: a column, or (op lhs rhs) with the reference's promotion (the library's own rule)."""
        if isinstance(col, tuple):
            a = L.Agg()
            keep, self._keep = self._keep, []
            M.agg_expr(self, a, col, table, None)
            self._keep = keep
            return L.agg_input_type(a) == L.RFX_F64
        return self._resolve(col, table).dtype == torch.float64

    # ------------------------------------------------------------------ equi-joins: rayforce_amd/joins.py
    def join_index(self, keys, left, right) -> torch.Tensor:
        from . import joins
        return joins.join_index(self, keys, left, right)

    def left_join(self, keys, left, right) -> Dict[str, torch.Tensor]:
        from . import joins
        return joins.left_join(self, keys, left, right)

    def inner_join(self, keys, left, right) -> Dict[str, torch.Tensor]:
        from . import joins
        return joins.inner_join(self, keys, left, right)

    def asof_index(self, keys, time, left, right) -> torch.Tensor:
        """Per left row the right row an asof join pairs it with, or null (rfx_exec_asof_index)."""
        from . import joins
        return joins.asof_index(self, keys, time, left, right)

    def asof_join(self, keys, left, right) -> Dict[str, torch.Tensor]:
        """``(asof-join keys left right)``: the last of ``keys`` is the asof column."""
        from . import joins
        return joins.asof_join(self, keys, left, right)

    def window_join(self, keys, windows, left, right, aggs, closed: bool = False) -> Dict[str, torch.Tensor]:
        """``(window-join keys windows left right aggs)`` (``closed``: window-join1): the last of ``keys`` is the window column, ``windows``
        the pair (lower, upper) of bounds per left row, ``aggs`` maps a result name to (aggregate, right column)."""
        from . import joins
        return joins.window_join(self, keys, windows, left, right, aggs, closed)

    def bin(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``(bin x y)``: per cell of y the last probe position of the reference's binary search with x[mid] <= y, else -1."""
        from . import joins
        return joins.bin_search(self, x, y, False)

    def binr(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``(binr x y)``: the first probe position with x[mid] >= y, else len x."""
        from . import joins
        return joins.bin_search(self, x, y, True)

    # ------------------------------------------------------------------ the set verbs (rfx_set.hip): rayforce_amd/sets.py
    def distinct(self, x: torch.Tensor) -> torch.Tensor:
        """``(distinct x)``: ascending on the reference's dense route, in its table's slot order on the hash route (``last_set_route``)."""
        from . import sets
        return sets.distinct(self, x)

    def union(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``(union x y)``: distinct of x followed by y; the concatenation is never made."""
        from . import sets
        return sets.distinct(self, x, y)

    def isin(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``(in x y)``: int8 0 / 1 per cell of x."""
        from . import sets
        return sets.member(self, x, y, False)

    def find(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``(find x y)``: per cell of y the first row of x holding it, or null; empty when x is empty."""
        from . import sets
        return sets.member(self, x, y, True)

    def sect(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """``(sect x y)``: the cells of x that occur in y, in x's order."""
        from . import sets
        return sets.set_filter(self, x, y, True)

    def except_(self, x: torch.Tensor, y) -> torch.Tensor:
        """``(except x y)``: the cells of x that do not occur in y (a column, or one int)."""
        from . import sets
        return sets.set_filter(self, x, y, False)

    # ------------------------------------------------------------------ the select surface (core/query.c:607-654)
    def select(self, query: Dict) -> Dict[str, torch.Tensor]:
        """``(select {name: (fn col) ... from: t where: p by: k})`` with t a dict of equally long device columns -- answered by the planner
        through this engine's shards (the same entry points rfx_select plans through; `select_door` asks the C operator itself).
        Keys ``from`` (required), ``where``, ``by`` (column name, or {name: column | ("xbar", column, width)}) are clauses; every other key is
        an output column ``(fn, column | expression)``.  Without outputs the filtered columns come back (select_collect_fields,
        core/query.c:474-557).  Result: dict name -> device tensor, group key(s) first."""
        if "from" not in query:
            raise RfxError("'select' expects 'from' param")  # core/query.c:281
        table = query["from"]
        where, by = query.get("where"), query.get("by")
        outs = [(k, v) for k, v in query.items() if k not in ("from", "where", "by", "take", "order")]
        if len({int(c.numel()) for c in table.values()}) > 1:
            raise RfxError("table columns differ in length")
        n = next(iter(table.values())).numel() if table else 0
        aggs = [(fn, col) for _, (fn, col) in outs]
        if by is not None:
            r = self.group_by(list(by.values()) if isinstance(by, dict) else by, aggs, where, table, order=query.get("order", "first"))
            if isinstance(by, dict):
                res = dict(zip(by.keys(), r["key_columns"])) if len(by) > 1 else {next(iter(by)): r["keys"]}
            else:
                res = {by if isinstance(by, str) else "by": r["keys"]}
            res.update({name: col for (name, _), col in zip(outs, r["results"])})
            return res
        if outs:
            vals, _ = self.filter_aggr(aggs, where, table, nrows=n)
            res = {}
            for (name, (fn, col)), v in zip(outs, vals):
                f64 = fn == "avg" or (col is not None and fn != "count" and self._arg_f64(col, table))
                if v is None:
                    v = float("nan") if f64 else L.NULL_I64
                res[name] = torch.tensor([v], dtype=torch.float64 if f64 else torch.int64, device=self.device)
            return res
        if where is None:
            return dict(table)
        ids = self.where(where, table)
        return {name: self.at_ids(col, ids) for name, col in table.items()}
