"""The reference's asof join, bin and binr restated in numpy: index_asof_join_obj / index_bin_i64 (core/index.c:3121-3137,3194-3267),
__left_join_inner (core/join.c:38-156), ray_bin / ray_binr (core/items.c:1399-1644).  Cells are int64 (a 4-byte TIME cell sign-extended, F64 cells
as their bit patterns); tests/test_asof_cpu.py holds this restatement to the fixture written from the compiled reference, which is what lets
the GPU tests use inputs far larger than the fixture."""
import numpy as np

T_LIST, T_I64, T_SYMBOL, T_TIME, T_TIMESTAMP, T_F64 = 0, 5, 6, 8, 9, 10
NULL = -(2**63)
NAN_BITS = 0x7FF8000000000000


def search(t, base, length, q, right=False):
    """Per query i the reference's loop over t[base[i] : base[i] + length[i]], every query at once:
        left = 0, right = len - 1, idx = none; while (left <= right) { mid = left + (right - left) / 2;
        if (t[mid] <= q) { idx = mid; left = mid + 1; } else right = mid - 1; }                     (right=False: asof, bin; none = -1)
        if (t[mid] >= q) { idx = mid; right = mid - 1; } else left = mid + 1;                       (right=True: binr; none = len)
    -> idx, a position inside the segment."""
    t, q = np.asarray(t, np.int64), np.asarray(q, np.int64)
    base = np.broadcast_to(np.asarray(base, np.int64), q.shape)
    length = np.broadcast_to(np.asarray(length, np.int64), q.shape)
    lo, hi = np.zeros(q.shape, np.int64), length - 1
    idx = length.copy() if right else np.full(q.shape, -1, np.int64)
    live = lo <= hi
    while live.any():
        mid = lo + (hi - lo) // 2
        v = t[np.where(live, base + mid, 0)] if t.size else np.zeros(q.shape, np.int64)
        hit = live & ((v >= q) if right else (v <= q))
        miss = live & ~hit
        idx = np.where(hit, mid, idx)
        if right:
            hi = np.where(hit, mid - 1, hi)
            lo = np.where(miss, mid + 1, lo)
        else:
            lo = np.where(hit, mid + 1, lo)
            hi = np.where(miss, mid - 1, hi)
        live = lo <= hi
    return idx


def bin_(x, y):
    return search(x, 0, len(x), y, False)


def binr(x, y):
    return search(x, 0, len(x), y, True)


def groups(lkeys, rkeys):
    """One id per distinct key tuple of either side (cells compared as raw integers: null equals null) -> (ids of the left rows, of the right rows, count)"""
    nl = len(lkeys[0])
    both = [np.concatenate([np.asarray(a, np.int64), np.asarray(b, np.int64)]) for a, b in zip(lkeys, rkeys)]
    if len(both) == 1:
        _, inv = np.unique(both[0], return_inverse=True)
    else:
        order = np.lexsort(both[::-1])
        new = np.zeros(order.size, bool)
        for c in both:
            s = c[order]
            new[1:] |= s[1:] != s[:-1]
        inv = np.empty(order.size, np.int64)
        inv[order] = np.cumsum(new)
    inv = inv.reshape(-1).astype(np.int64)
    return inv[:nl], inv[nl:], (int(inv.max()) + 1 if inv.size else 0)


def asof_index(lkeys, lt, rkeys, rt):
    """ids[i] = the right row left row i is paired with, or NULL: the right rows of i's key tuple in ascending ROW order (not time order), searched
    by time with the loop above; the answer is the row at the position it lands on"""
    lt, rt = np.asarray(lt, np.int64), np.asarray(rt, np.int64)
    gl, gr, ng = groups(lkeys, rkeys)
    rows = np.argsort(gr, kind="stable")  # every group's rows adjacent, ascending inside the group
    counts = np.bincount(gr, minlength=ng).astype(np.int64)
    starts = np.cumsum(counts) - counts
    base, length = starts[gl], counts[gl]  # (a tuple the right side lacks: length 0)
    idx = search(rt[rows], base, length, lt, False)
    if rows.size == 0:
        return np.full(lt.shape, NULL, np.int64)
    return np.where(idx >= 0, rows[np.where(idx >= 0, base + idx, 0)], NULL)


def asof_join(keys, left, right):
    """left / right: {name: (cells, type)}; keys: the equality columns and, last, the asof column.  -> {name: (cells, null flags, type)} in the
    reference's column order: the key columns (the LEFT table's own, the asof column included), the other left columns, the right-only ones; a
    column the right table has takes the matched right row's cell, else the left row's own; a right-only column has no cell for an unmatched row
    (flag 1: the reference holds a Null object there, this engine the typed null)."""
    ids = asof_index([left[k][0] for k in keys[:-1]], left[keys[-1]][0], [right[k][0] for k in keys[:-1]], right[keys[-1]][0])
    hit = ids != NULL
    at = np.where(hit, ids, 0)
    out = {}
    for name in list(keys) + [c for c in left if c not in keys] + [c for c in right if c not in keys and c not in left]:
        if name in keys or name not in right:
            out[name] = (left[name][0], np.zeros(len(ids), np.int8), left[name][1])
            continue
        rv, rtype = right[name]
        got = rv[at] if len(rv) else np.zeros(len(ids), np.int64)
        if name in left:
            out[name] = (np.where(hit, got, left[name][0]), np.zeros(len(ids), np.int8), rtype)
        else:
            out[name] = (np.where(hit, got, 0), (~hit).astype(np.int8), rtype)
    return out


def typed_null(t):
    return np.int64(NAN_BITS) if t == T_F64 else np.int64(NULL)
