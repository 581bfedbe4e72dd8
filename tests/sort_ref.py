"""numpy restatement of the sort verbs' contract (include/rfx_hip.h "stable radix sort", include/rfx_ops.h rfx_iasc ..): the sort key u(x), stable
orders in both directions, the attribute short-cuts.  Values travel as int64 bit patterns of their cells ('f64' says how to read them)."""
import numpy as np

ATTR_DISTINCT, ATTR_ASC, ATTR_DESC = 1, 2, 4
T_I64, T_SYMBOL, T_TIMESTAMP, T_F64 = 5, 6, 9, 10
TOP = np.uint64(1 << 63)


def u(bits, f64):
    """the sort key of 8-byte cells given as int64 bit patterns"""
    b = np.ascontiguousarray(bits).view(np.uint64)
    if not f64:
        return b ^ TOP
    nan = (b & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)
    return np.where(nan, np.uint64(0), np.where((b & TOP) != 0, ~b, b | TOP))


def order(bits, f64, descending=False, attrs=0):
    """(iasc / idesc, attrs of the result)"""
    n = len(bits)
    if n == 0:
        return np.empty(0, np.int64), 0
    if attrs & (ATTR_ASC | ATTR_DESC):  # the attribute is trusted, not the data
        up = bool(attrs & ATTR_ASC) != bool(descending)
        return (np.arange(n, dtype=np.int64) if up else np.arange(n - 1, -1, -1, dtype=np.int64)), (ATTR_ASC if up else ATTR_DESC) | ATTR_DISTINCT
    k = u(bits, f64)
    return np.argsort(~k if descending else k, kind="stable").astype(np.int64), 0


def values(bits, f64, descending=False, attrs=0):
    """(asc / desc cells, attrs of the result)"""
    same, other = (ATTR_DESC, ATTR_ASC) if descending else (ATTR_ASC, ATTR_DESC)
    if attrs & same:
        return np.array(bits, np.int64), attrs
    if attrs & other:
        return np.array(bits[::-1], np.int64), (attrs & ~(ATTR_ASC | ATTR_DESC)) | same  # (ray_reverse swaps the two attributes)
    return np.asarray(bits, np.int64)[order(bits, f64, descending)[0]], same | (attrs & ATTR_DISTINCT)


def rank(bits, f64, attrs=0):
    n = len(bits)
    if attrs & ATTR_ASC:
        return np.arange(n, dtype=np.int64), ATTR_ASC | ATTR_DISTINCT
    if attrs & ATTR_DESC:
        return np.arange(n - 1, -1, -1, dtype=np.int64), 0
    out = np.empty(n, np.int64)
    out[order(bits, f64)[0]] = np.arange(n, dtype=np.int64)
    return out, 0


def lex_order(cols, f64s, descending=False):
    """rows ordered by cols[0] (most significant) .. cols[-1], stable, one direction for all"""
    keys = [(~u(c, f) if descending else u(c, f)) for c, f in zip(cols, f64s)]
    return np.lexsort(keys[::-1]).astype(np.int64)
