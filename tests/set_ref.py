"""A numpy restatement of the reference's set verbs over 8-byte keys -- distinct, in, find, sect, except, union -- with its ROUTES.

What is restated (paths in the RayforceDB tree):
  index_distinct_i64   core/index.c:551-607    scope over every cell; dense when range <= len or range <= 2^20 (the values ascending), else a
                                               linear-probing table of next_prime(ceil(len / 0.75)) cells filled in row order, read in slot order
  index_in_i64_i64     core/index.c:1291-1361  dense over the intersection of the two scopes when it spans <= 2^20, else a table; membership
  index_find_i64       core/index.c:1507-1574  the same two routes, the first row of x per cell of y
  ray_sect / ray_except / ray_union  core/items.c:898-1029   filter(x, in(x, y)), filter(x, not in(x, y)), distinct(concat(x, y))
  ht_oa_create / ht_oa_tab_next / ht_oa_tab_get  core/hash.c:35-127,207-225    home cell = (i64)key % size

Every function returns (answer, route) with route one of "none", "dense", "hash", "disjoint", "atom" -- or (UNDEFINED, reason) for the shapes where
the reference indexes outside its own table (a negative key on a hash route, for find a null too; a range that does not fit 64 bits): there is
nothing to restate there.  Test infrastructure only."""
import numpy as np

NULL = -(2**63)
I64_MAX = 2**63 - 1
MAX_RANGE = 1 << 20
UNDEFINED = "undefined"


def is_prime(v: int) -> bool:
    if v <= 1:
        return False
    if v <= 3:
        return True
    if v % 2 == 0 or v % 3 == 0:
        return False
    i = 5
    while i * i <= v:
        if v % i == 0 or v % (i + 2) == 0:
            return False
        i += 6
    return True


def table_cells(n: int) -> int:
    """ht_oa_create(n): the first prime >= ceil(n / 0.75), computed in doubles as the reference does"""
    want = float(n) / 0.75
    p = int(want)
    if float(p) < want:
        p += 1
    while not is_prime(p):
        p += 1
    return p


def _arr(a):
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _scope(a):
    """(min, max, min over the non-null cells or None, null cells) as Python ints"""
    nn = a[a != NULL]
    return int(a.min()), int(a.max()), (int(nn.min()) if nn.size else None), int(a.size - nn.size)


def sequential_table(keys_in_row_order, P: int):
    """The reference's insert loop: distinct non-negative keys in the order of their first rows -> the table's cells (None = empty)"""
    cells = [None] * P
    for k in keys_in_row_order:
        s = k % P
        while cells[s] is not None:
            s = s + 1 if s + 1 < P else 0
        cells[s] = k
    return cells


def priority_table(first_rows, keys, P: int, order):
    """The device's construction: items (first row, key) inserted in ANY order; a cell keeps the smaller first row, the larger one walks on.
    Returns the cells as first rows (None = empty)."""
    cells = [None] * P
    for j in order:
        mine, s = int(first_rows[j]), int(keys[j]) % P
        while True:
            old = cells[s]
            if old is None or old > mine:
                cells[s] = mine
                if old is None:
                    break
                mine = old
            s = s + 1 if s + 1 < P else 0
    return cells


def distinct(a, b=None):
    a = _arr(a)
    if b is not None:
        a = np.concatenate([a, _arr(b)])
    n = a.size
    if n == 0:
        return np.empty(0, np.int64), "none"
    mn, mx, mnn, _ = _scope(a)
    rng = mx - mn + 1
    if rng > I64_MAX:
        return UNDEFINED, "max - min + 1 does not fit 64 bits"
    if rng <= n or rng <= MAX_RANGE:
        return np.unique(a), "dense"
    if mnn is not None and mnn < 0:
        return UNDEFINED, "hash route over a negative key"
    u, first = np.unique(a[a != NULL], return_index=True)
    keys = u[np.argsort(first, kind="stable")]
    cells = sequential_table([int(k) for k in keys], table_cells(n))
    return np.array([c for c in cells if c is not None], np.int64), "hash"


def _member_route(x, y, want_first):
    """x: the cells looked up, y: the set.  -> route or (UNDEFINED, reason)"""
    if y.size == 0:
        return "disjoint"
    ymn, ymx, ymnn, ynull = _scope(y)
    xmn, xmx, xmnn, xnull = _scope(x)
    mn, mx = max(xmn, ymn), min(xmx, ymx)
    if mn > mx:
        return "disjoint"
    rng = mx - mn + 1
    if want_first and rng > I64_MAX:
        return (UNDEFINED, "max - min + 1 does not fit 64 bits")
    if rng <= MAX_RANGE:
        return "dense"
    if (xmnn is not None and xmnn < 0) or (ymnn is not None and ymnn < 0):
        return (UNDEFINED, "hash route over a negative key")
    if want_first and (xnull or ynull):
        return (UNDEFINED, "hash route over a null")
    return "hash"


def isin(x, y):
    x, y = _arr(x), _arr(y)
    if x.size == 0:
        return np.empty(0, np.int8), "none"
    r = _member_route(x, y, False)
    if isinstance(r, tuple):
        return r
    return np.isin(x, y).astype(np.int8), r


def find(x, y):
    """per cell of y the first row of x holding it, else null; I64(0) when x is empty"""
    x, y = _arr(x), _arr(y)
    if x.size == 0 or y.size == 0:
        return np.empty(0, np.int64), "none"
    r = _member_route(y, x, True)
    if isinstance(r, tuple):
        return r
    u, first = np.unique(x, return_index=True)
    pos = np.minimum(np.searchsorted(u, y), u.size - 1)
    return np.where(u[pos] == y, first[pos], NULL).astype(np.int64), r


def _filter(x, y, keep):
    x = _arr(x)
    if x.size == 0:
        return np.empty(0, np.int64), "none"
    if isinstance(y, (int, np.integer)):
        assert not keep
        return x[x != int(y)], "atom"
    m, r = isin(x, y)
    if isinstance(m, str):
        return m, r
    return x[(m != 0) == keep], r


def sect(x, y):
    return _filter(x, y, True)


def except_(x, y):
    return _filter(x, y, False)


def union(x, y):
    return distinct(x, y)


VERBS = {"distinct": distinct, "in": isin, "find": find, "sect": sect, "except": except_, "union": union}
