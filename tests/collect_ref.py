"""numpy restatement of `row` and the collected column of select ... by: (aggr_row / aggr_collect, core/aggr.c:3021-3136).

AGGR_ITER (core/aggr.c:73-125) visits the elements i = 0 .. l-1 in order on one thread: the row is x = filter[i] under a filter, else i; the group is
y = ids[i] (INDEX_TYPE_IDS, aligned with the filter's positions) or table[source[x] - shift] (INDEX_TYPE_SHIFT); aggr_collect appends val[x] to group
y's vector, aggr_row appends x.  So the answer is the stable partition of the elements by group: a stable argsort of the ids plus a bincount."""
import numpy as np

NULL_I64 = -(2 ** 63)


def partition(gid, groups):
    """(offsets[groups + 1], perm[m]): the elements ordered by (group, element); ids outside [0, groups) are an error"""
    gid = np.asarray(gid, dtype=np.int64)
    if gid.size and (gid.min() < 0 or gid.max() >= groups):
        raise ValueError("a group id outside [0, groups)")
    perm = np.argsort(gid, kind="stable").astype(np.int64)
    offsets = np.zeros(groups + 1, dtype=np.int64)
    np.cumsum(np.bincount(gid, minlength=groups), out=offsets[1:])
    return offsets, perm


def ids_of_index(kind, l, ids=None, source=None, table=None, shift=0, rows=None):
    """the group of every element i < l under the two index flavours; `rows` = the filter's row ids or None"""
    x = np.arange(l, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)[:l]
    if kind == "ids":
        return np.asarray(ids, dtype=np.int64)[:l]
    slot = np.asarray(source, dtype=np.int64)[x] - shift
    if slot.size and (slot.min() < 0 or slot.max() >= len(table)):
        raise ValueError("a source cell outside the SHIFT table")
    return np.asarray(table, dtype=np.int64)[slot]


def collect(gid, groups, cols, rows=None):
    """(offsets, [cells of every column in group order], rows in group order): the cells in the column's own dtype"""
    offsets, perm = partition(gid, groups)
    src = perm if rows is None else np.asarray(rows, dtype=np.int64)[perm]
    return offsets, [np.asarray(c)[src] for c in cols], src.astype(np.int64)


def first_occurrence_ids(keys):
    """(distinct keys in first-occurrence order, every element's place among them): the group order of select ... by:"""
    keys = np.asarray(keys, dtype=np.int64)
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    return uniq[order], rank[inv.reshape(-1)]


def group_collect(key, cols, mask=None):
    """select {c: c ... by: key from: t where: mask} -> (keys, offsets, [cells], rows)"""
    key = np.asarray(key, dtype=np.int64)
    rows = None if mask is None else np.flatnonzero(mask).astype(np.int64)
    keys, gid = first_occurrence_ids(key if rows is None else key[rows])
    offsets, cells, src = collect(gid, len(keys), cols, rows)
    return keys, offsets, cells, src


def lists(offsets, cells):
    """the LIST the reference answers: one vector per group"""
    return [cells[offsets[g]:offsets[g + 1]] for g in range(len(offsets) - 1)]


# ---- inputs: arithmetic in the row number, never stored ----
DTYPES = {"b8": np.int8, "u8": np.uint8, "i16": np.int16, "i32": np.int32, "date": np.int32, "time": np.int32, "i64": np.int64, "symbol": np.int64,
          "timestamp": np.int64, "f64": np.float64}


def value_column(kind, n, seed=0):
    """a value column of one of the ten types whose every cell tells its row (modulo the type's range)"""
    i = np.arange(n, dtype=np.int64)
    x = (i * 2654435761 + seed * 40503) & 0x7FFFFFFF
    if kind == "b8":
        return ((x >> 7) & 1).astype(np.int8)
    if kind == "u8":
        return (x % 251).astype(np.uint8)
    if kind == "i16":
        return ((x % 65521) - 32760).astype(np.int16)
    if kind in ("i32", "date", "time"):
        return (x - (1 << 30)).astype(np.int32)
    if kind == "f64":
        return (x.astype(np.float64) - 1e9) / 1024.0
    return x * 1000003 - (1 << 40) + i


def key_column(n, groups, shape="cycle", base=0, stride=1):
    """n keys over `groups` distinct values base + stride * g.  cycle: g = i mod groups; heavy: every row group 0 but the last; own: every row its own"""
    i = np.arange(n, dtype=np.int64)
    if shape == "cycle":
        g = (i * 7919) % groups if groups > 1 else np.zeros(n, dtype=np.int64)
        g[:min(n, groups)] = np.arange(min(n, groups))  # (every group occurs)
    elif shape == "heavy":
        g = np.zeros(n, dtype=np.int64)
        if n:
            g[-1] = 1 if groups > 1 else 0
    else:
        g = i.copy()
    return base + stride * g


# ---- the golden cases: what tests/golden/make_collect_golden.py runs through the compiled reference, and what the tests replay ----
TYPE_CODE = {"b8": 1, "u8": 2, "i16": 3, "i32": 4, "i64": 5, "symbol": 6, "date": 7, "time": 8, "timestamp": 9, "f64": 10}
RECORDED = ["b8", "u8", "i16", "i32", "date", "time", "i64", "timestamp", "f64"]  # (SYMBOL cells are interned ids: the tests run the I64 case under its code)
ROUTES = {"shift": dict(base=-40, stride=1),                    # range <= 524 288 and <= rows: rfx_group's key table (INDEX_TYPE_SHIFT)
          "dense": dict(base=1000, stride=1),                   # range > 524 288, still <= rows: dense per-row ids (INDEX_TYPE_IDS)
          "sparse": dict(base=-(1 << 50), stride=(1 << 40) + 12345)}  # range > rows: the hashed route's per-row ids
WHERES = {None: None, "none": "(< i 0)", "one": "(== i 0)", "all": "(>= i 0)", "some": "(< a 37)"}


def _case(name, n, groups, shape="cycle", route="shift", where=None, kinds=("i64",), row=True, aggs=True):
    return dict(name=name, n=n, groups=groups, shape=shape, route=route, where=where, kinds=list(kinds), row=row, aggs=aggs)


def cases():
    out = []
    for n in (0, 1, 63, 64, 65, 4097):
        out.append(_case(f"rows{n}", n, min(n, 7), kinds=("i64", "f64")))
    for g in (1, 2, 255, 256, 257):
        out.append(_case(f"groups{g}", 4097, g, kinds=("i64",)))
    out.append(_case("groups65537", 70001, 65537, kinds=("i64", "i32")))
    out.append(_case("heavy", 4097, 2, shape="heavy", kinds=("i64", "u8")))
    out.append(_case("own", 4097, 4097, shape="own", kinds=("f64", "i16")))
    out.append(_case("types", 4097, 257, kinds=RECORDED))
    out.append(_case("bare_only", 4097, 257, kinds=("i64",), row=False, aggs=False))
    out.append(_case("row_only", 4097, 257, kinds=(), aggs=False))
    for w in ("none", "one", "all", "some"):
        out.append(_case(f"where_{w}", 4097, 257, where=w, kinds=("i64", "f64", "b8")))
    out.append(_case("where_some_65537", 70001, 65537, where="some", kinds=("i64", "date")))
    out.append(_case("where_types", 4097, 257, where="some", kinds=RECORDED))
    out.append(_case("sparse", 4097, 257, route="sparse", kinds=("i64", "time")))
    out.append(_case("sparse_where", 70001, 65537, route="sparse", where="some", kinds=("timestamp",)))
    out.append(_case("dense_ids", 600011, 590000, route="dense", kinds=("i64",)))
    out.append(_case("dense_ids_where", 600011, 590000, route="dense", where="some", kinds=("f64",)))
    return out


def case_table(c):
    """the case's table: k the key, i the row number, a the filter column, vi the aggregates' column, v_<kind> the value columns"""
    n = c["n"]
    t = {"k": key_column(n, c["groups"], c["shape"], **ROUTES[c["route"]]), "i": np.arange(n, dtype=np.int64), "a": value_column("i64", n, 9) % 100,
         "vi": value_column("i64", n, 1) % 1000003}
    for s, kind in enumerate(c["kinds"]):
        t[f"v_{kind}"] = value_column(kind, n, s + 2)
    return t


def case_mask(c, t):
    w = c["where"]
    return None if w is None else {"none": t["i"] < 0, "one": t["i"] == 0, "all": t["i"] >= 0, "some": t["a"] < 37}[w]


def case_mappings(c):
    """[(result name, expression as text, as a tuple for the host object model)] in the query's order: aggregates and nested columns interleaved"""
    m = []
    if c["aggs"]:
        m.append(("s", "(sum vi)", ("sum", "vi")))
    for kind in c["kinds"]:
        m.append((f"p_{kind}", f"v_{kind}", f"v_{kind}"))
    if c["aggs"]:
        m.append(("c", "(count vi)", ("count", "vi")))
    if c["row"]:
        m.append(("r", "(row vi)", ("row", "vi")))
    if c["aggs"]:
        m.append(("f", "(first vi)", ("first", "vi")))
    return m


def case_expected(c, t=None):
    """the restatement's answer: {k, n (the groups' lengths), s, c, f, r (razed), p_<kind> (razed)}"""
    t = case_table(c) if t is None else t
    keys, offsets, cells, rows = group_collect(t["k"], [t[f"v_{kind}"] for kind in c["kinds"]], case_mask(c, t))
    want = {"k": keys, "n": np.diff(offsets)}
    for kind, cc in zip(c["kinds"], cells):
        want[f"p_{kind}"] = cc
    if c["row"]:
        want["r"] = rows
    if c["aggs"]:
        vi = t["vi"][rows]
        want["c"] = np.diff(offsets)
        want["s"] = np.add.reduceat(vi, offsets[:-1]).astype(np.int64) if len(keys) else np.empty(0, np.int64)
        want["f"] = vi[offsets[:-1]] if len(keys) else np.empty(0, np.int64)
    return want


def digest(a):
    """what the fixture keeps of an answer column: its dtype, length and the sha-256 of its cells"""
    import hashlib
    a = np.ascontiguousarray(a)
    return f"{a.dtype.name}|{a.size}|{hashlib.sha256(a.tobytes()).hexdigest()}"


# ---- shapes the door hands to the host's own verb (without a host: refused with this reason) ----
HOST_SHAPES = {"mapfilter": "a MAPFILTER pair", "plain_vector": "not a MAPGROUP pair", "index_type": "parted / window index",
               "c8_value": "value column type", "list_value": "value column type", "device_i32": "a device column that is not I64 / F64 / TIMESTAMP / B8"}
