"""numpy restatement of the sort verbs over 1-, 2- and 4-byte keys (include/rfx_hip.h "stable radix sort", keys of at most 32 bits): a stable argsort
of the 32-bit key, its complement within the key's width for descending, the attribute short-cuts of the 8-byte verbs (tests/sort_ref.py).  Cells
travel in their own dtype: uint8 (B8, U8), int16 (I16), int32 (I32, DATE, TIME)."""
import numpy as np

ATTR_DISTINCT, ATTR_ASC, ATTR_DESC = 1, 2, 4
T_B8, T_U8, T_I16, T_I32, T_I64, T_DATE, T_TIME, T_ERR = 1, 2, 3, 4, 5, 7, 8, 127
DTYPE = {T_B8: np.uint8, T_U8: np.uint8, T_I16: np.int16, T_I32: np.int32, T_DATE: np.int32, T_TIME: np.int32}
NULL_I32, NULL_I64 = -(2**31), -(2**63)


def key_bytes(cells):
    return np.asarray(cells).dtype.itemsize


def key32(cells, descending=False):
    """the 32-bit sort key: the byte itself; (u16)x ^ 0x8000; (u32)x ^ 0x80000000 (INT32_MIN, the null, is 0).  Descending: the complement
    within the key's width."""
    c = np.ascontiguousarray(cells)
    w = c.dtype.itemsize
    if w == 1:
        k = c.view(np.uint8).astype(np.uint32)
    elif w == 2:
        k = c.view(np.uint16).astype(np.uint32) ^ np.uint32(0x8000)
    else:
        assert w == 4, c.dtype
        k = c.view(np.uint32) ^ np.uint32(0x80000000)
    return k ^ np.uint32((1 << (8 * w)) - 1) if descending else k


def key32_of_widened(image, descending=False):
    """the same key from an I32-family column's widened 8-byte image (NULL_I32 -> NULL_I64, else sign-extended)"""
    im = np.ascontiguousarray(image, dtype=np.int64)
    k = np.where(im == NULL_I64, np.uint32(0), im.view(np.uint64).astype(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint32)
    return ~k if descending else k


def widen(cells):
    c = np.asarray(cells, np.int32)
    return np.where(c == NULL_I32, np.int64(NULL_I64), c.astype(np.int64))


def varying_digits(cells):
    k = key32(cells)
    return sum(1 for d in range(key_bytes(cells)) if len(np.unique((k >> np.uint32(8 * d)) & np.uint32(255))) > 1)


def order(cells, descending=False, attrs=0):
    """(iasc / idesc, attrs of the result)"""
    n = len(cells)
    if n == 0:
        return np.empty(0, np.int64), 0
    if attrs & (ATTR_ASC | ATTR_DESC):  # the attribute is trusted, not the data
        up = bool(attrs & ATTR_ASC) != bool(descending)
        return (np.arange(n, dtype=np.int64) if up else np.arange(n - 1, -1, -1, dtype=np.int64)), (ATTR_ASC if up else ATTR_DESC) | ATTR_DISTINCT
    return np.argsort(key32(cells, descending), kind="stable").astype(np.int64), 0


def values(cells, descending=False, attrs=0):
    """(asc / desc cells in the input's dtype, attrs of the result); None where the reference answers an error: an I16 vector whose attribute asks
    for a reverse (ray_reverse has no I16 arm)"""
    cells = np.asarray(cells)
    same, other = (ATTR_DESC, ATTR_ASC) if descending else (ATTR_ASC, ATTR_DESC)
    if attrs & same:
        return cells.copy(), attrs
    if attrs & other:
        if cells.dtype == np.int16:
            return None, 0
        return cells[::-1].copy(), (attrs & ~(ATTR_ASC | ATTR_DESC)) | same  # (ray_reverse swaps the two attributes)
    return cells[order(cells, descending)[0]], same | (attrs & ATTR_DISTINCT)


def rank(cells, attrs=0):
    n = len(cells)
    if attrs & ATTR_ASC:
        return np.arange(n, dtype=np.int64), ATTR_ASC | ATTR_DISTINCT
    if attrs & ATTR_DESC:
        return np.arange(n - 1, -1, -1, dtype=np.int64), 0
    out = np.empty(n, np.int64)
    out[order(cells)[0]] = np.arange(n, dtype=np.int64)
    return out, 0


def restated(verb, cells, attrs=0):
    if verb in ("iasc", "idesc"):
        return order(cells, verb == "idesc", attrs)
    if verb in ("asc", "desc"):
        return values(cells, verb == "desc", attrs)
    return rank(cells, attrs)
