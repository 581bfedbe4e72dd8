"""upsert (ray_upsert, core/update.c:556-750) and insert (ray_insert, :414-542) restated in numpy, the inputs of the fixture's cases, and the loader of
tests/golden/upsert_golden.npz, the compiled reference's own answers.  These are copies: cells, type code and attribute byte must agree bit for bit.
Test infrastructure only.

A case is a small description -- its inputs are ARITHMETIC in the row number and are made here (inputs), by the recorder and by the tests alike, so the
fixture holds descriptions and recorded answers only:
  name, verb ("upsert" | "insert"), keys, form ("list" | "record" | "dict" | "table" | "dict_record"), types (the table's column type codes; the first
  `keys` are the key), n (table rows), m (batch rows), pattern (which table row each batch row's key names: PATTERNS), given (the table column indices the
  batch provides, in the batch's own order), sparse (keys far apart: find's hash route), tdup (table row 10 carries row 3's key).
  out -- per result column (type, attrs, cells) as the reference answered.
A `host_` case has `shape` (what to build: HOST_SHAPES) and `host`, the reason the device path names when it hands the shape to the host.

The semantics, where the code surprises:
  * the index is taken once, against the table as it was: the FIRST table row with the key tuple; two batch rows with one new key are both appended;
  * several batch rows matching one row: the last in batch order wins;
  * a LIST of l < p columns appends null(type) for the others and leaves their matched rows alone; a DICT / TABLE is reordered first and a column it misses
    is a null VECTOR (nullv): matched rows are overwritten with it.  nullv is 0 for the 1-, 2- and 4-byte types, the null for the 8-byte ones;
  * a matched row is written by set_idx, which knows I64 / SYMBOL / TIMESTAMP / F64 cells only: it turns a B8 / U8 / I16 / I32 / DATE / TIME value column into
    a LIST; appends keep B8 / I16 / I32 vectors, never DATE / TIME ones, U8 ones under insert's vector forms only.  Those answers are the host's;
  * one record under two or more keys does not find its row in the reference (it indexes a LIST of atoms): the host's;
  * every column of the answer is a fresh vector of the column's type, attribute byte 0.

Further down: the three device calls of include/rfx_hip.h restated (winners, plan, plan_loop, place, fill), a case's answer composed from them as the
planner composes it (rebuilt), and find's route from the key columns' ranges (find_route) -- the reference of tests/test_upsert_edges_gpu.py."""
import json
import os

import numpy as np

from concat_ref import B8, U8, I16, I32, I64, SYMBOL, DATE, TIME, TS, F64, GUID, C8, ENUM, MAPLIST, DTYPE, as_bits, planes, unplanes  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upsert_golden.npz")
BIG = 2**20 + 5
NULL_I64 = -2**63
ADOPTED = (I64, SYMBOL, TS, F64, B8)


def nullv(tp):
    """what the reference's nullv() fills a vector of this type with (core/rayforce.c:104-148)"""
    if tp in (I64, SYMBOL, TS):
        return np.int64(NULL_I64)
    return np.float64(np.nan) if tp == F64 else DTYPE[tp](0)


def value_cells(tp, rows, salt):
    """a value column's cells for the row numbers `rows`: arithmetic, every 16th a null (NaN), periodic so that the planes compress"""
    i = (np.asarray(rows, dtype=np.int64) + salt * 1009) % 4093
    if tp == B8:
        return (i % 3 == 0).astype(np.int8)
    if tp == U8:
        return ((i * 7 + 3) % 251).astype(np.uint8)
    if tp == F64:
        return np.where(i % 16 == 5, np.nan, i * 0.5 - 1000.0)
    null = {2: -2**15, 4: -2**31, 8: -2**63}[np.dtype(DTYPE[tp]).itemsize]
    return np.where(i % 16 == 5, null, i * 7 - 3000).astype(DTYPE[tp])


def key_cells(r, nkeys, sparse):
    """the key tuple of "row reference" r (>= 0; one tuple per r): one key r * 3 + 7 (sparse: r * 1000003), two (r // 5, r % 5), three (r // 25, r // 5 % 5, r % 5)"""
    r = np.asarray(r, dtype=np.int64)
    if nkeys == 1:
        return [r * 1000003 + 11 if sparse else r * 3 + 7]
    if nkeys == 2:
        return [r // 5, r % 5 + 100]
    return [r // 25, (r // 5) % 5 + 100, r % 5]


def batch_refs(pattern, n, m):
    """which row reference each batch row's key names: < n a table row, >= n a new key"""
    j = np.arange(m, dtype=np.int64)
    hit = j * 7 % n if n else j + n
    if pattern == "all":
        return hit
    if pattern == "none":
        return n + j
    if pattern == "alt":  # matched, new, matched, new ...
        return np.where(j % 2 == 0, hit, n + j) if n else n + j
    if pattern == "runs":  # a matched run and an unmatched run, each longer than a block
        return np.where(j < m // 2, hit, n + j)
    if pattern == "dups":  # one matched key within a wavefront, across wavefronts, across blocks, last in the final partial block
        r = np.where(j % 2 == 0, hit, n + j)
        r[[3, 40, 300, 2100, m - 1]] = 5
        return r
    if pattern == "newdups":  # the same NEW key several times: all appended
        r = np.where(j % 2 == 0, hit, n + j)
        r[[1, 2, 70, m - 1]] = n + 1
        return r
    if pattern == "hot":  # every batch row on one of 1 000 table rows, every 64th a new key: the contended atomicMax
        return np.where(j % 64 == 63, n + j, (j * 7919 % 1000) * (n // 1000)) if n else n + j
    if pattern == "one":  # one address: every even batch row names table row 5, every odd one is new
        return np.where(j % 2 == 0, 5, n + j) if n > 5 else n + j
    raise KeyError(pattern)


PATTERNS = ("all", "none", "alt", "runs", "dups", "newdups")
SCALE_PATTERNS = ("hot", "one")  # of the tests at scale (tests/test_upsert_edges_gpu.py): not in the fixture, not in its census


def inputs(c):
    """-> (table columns [cells], batch columns [cells] in the order of c["given"])"""
    n, m, keys, types = c["n"], c["m"], c["keys"], c["types"]
    nk = max(keys, 1)
    tr = np.arange(n, dtype=np.int64)
    if c.get("tdup") and n > 10:
        tr[10] = 3
    tk = key_cells(tr, nk, c.get("sparse"))
    bk = key_cells(batch_refs(c["pattern"], n, m), nk, c.get("sparse"))
    table = [tk[i].astype(DTYPE[tp]) if i < nk else value_cells(tp, np.arange(n), i) for i, tp in enumerate(types)]
    batch = [bk[i].astype(DTYPE[types[i]]) if i < nk else value_cells(types[i], np.arange(m) + 77, i + 31) for i in c["given"]]
    return table, batch


def index(table, batch, keys):
    """idx[j] = the first table row whose key tuple equals batch row j's, else -1 (index_upsert_obj, core/index.c:3001-3065)"""
    n, m = len(table[0]), len(batch[0])
    code = np.zeros(n + m, dtype=np.int64)
    for k in range(keys):  # the tuples as one integer: every column's cells numbered densely
        u, inv = np.unique(np.concatenate([table[k], batch[k]]), return_inverse=True)
        code = code * len(u) + inv.reshape(-1)
    tc, bc = code[:n], code[n:]
    order = np.argsort(tc, kind="stable")  # (stable: the first row of equal tuples comes first)
    at = np.searchsorted(tc[order], bc, side="left")
    hit = (at < n) & (tc[order][np.minimum(at, max(n - 1, 0))] == bc) if n else np.zeros(m, dtype=bool)
    return np.where(hit, order[np.minimum(at, max(n - 1, 0))] if n else -1, -1).astype(np.int64).reshape(m)


def ordered(c, batch):
    """the batch in the table's column order: per table column its cells or None, and whether a missing column is a null vector (DICT / TABLE)"""
    p = len(c["types"])
    cols = [None] * p
    for cells, i in zip(batch, c["given"]):
        cols[i] = cells
    return cols, c["form"] in ("dict", "table", "dict_record")


def answer(c, counts=None):
    """a case -> the answer's columns [(type, attrs, cells)], vectorised: dest by last-writer-wins + ordered append"""
    table, batch = inputs(c)
    cols, nulled = ordered(c, batch)
    n, m, keys = c["n"], c["m"], c["keys"]
    idx = index(table, [cols[k] for k in range(keys)], keys) if keys else np.full(m, -1, dtype=np.int64)
    miss = idx < 0
    a = int(miss.sum())
    if counts is not None:
        counts.update(matched=m - a, appended=a)
    out = []
    for i, tp in enumerate(c["types"]):
        o = np.concatenate([table[i], np.full(a, nullv(tp), dtype=DTYPE[tp])])
        b = cols[i] if cols[i] is not None else (np.full(m, nullv(tp), dtype=DTYPE[tp]) if nulled else None)
        if b is not None:
            o[n:] = b[miss]
            if i >= keys:
                hit = np.flatnonzero(~miss)
                o[idx[hit]] = b[hit]  # (numpy assigns in order: the last of several batch rows for one row stays)
        out.append((tp, 0, o))
    return out


def replay(c):
    """the reference's loop, cell by cell (core/update.c:717-739; insert: every row appended)"""
    table, batch = inputs(c)
    cols, nulled = ordered(c, batch)
    keys, m = c["keys"], c["m"]
    first = {}
    for i in range(c["n"] - 1, -1, -1):  # the first row of every key tuple, literally
        first[tuple(int(table[k][i]) for k in range(keys))] = i
    rows = [first.get(tuple(int(cols[k][j]) for k in range(keys)), -1) if keys else -1 for j in range(m)]
    out = []
    for i, tp in enumerate(c["types"]):
        col = list(table[i])
        b = cols[i] if cols[i] is not None else ([nullv(tp)] * m if nulled else None)
        for j in range(m):
            if rows[j] < 0:
                col.append(b[j] if b is not None else nullv(tp))
            elif keys <= i and b is not None:
                col[rows[j]] = b[j]
        out.append((tp, 0, np.array(col, dtype=DTYPE[tp])))
    return out


# ---- the three device calls of include/rfx_hip.h, restated: rfx_hip_upsert_plan, _place, _fill ----
HOSTILE = (NULL_I64, -1, -7)  # "none" beside a row >= n: the null and two negatives


def winners(idx, n):
    """per table row the largest batch row that matched it, -1 where none did: what the scratch W holds at the matched rows after k_up_max"""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    hit = idx.view(np.uint64) < np.uint64(n)
    w = np.full(n, -1, dtype=np.int64)
    np.maximum.at(w, idx[hit], np.flatnonzero(hit))
    return w


def plan(idx, n):
    """rfx_hip_upsert_plan -> (dest, appended): a row is matched iff (uint64)idx[j] < n; dest[j] = idx[j] when j is the largest batch row with that idx, -1
    when a later one has it, n + (the unmatched rows before j) otherwise"""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    j = np.arange(len(idx), dtype=np.int64)
    hit = idx.view(np.uint64) < np.uint64(n)
    w = winners(idx, n)
    miss = (~hit).astype(np.int64)
    dest = n + np.cumsum(miss) - miss  # (the exclusive count)
    dest[hit] = np.where(w[idx[hit]] == j[hit], idx[hit], -1)
    return dest, int(miss.sum())


def plan_loop(idx, n):
    """the same, row by row (small m)"""
    last, dest, a = {}, [], 0
    for j, r in enumerate(idx):
        if 0 <= int(r) < n:
            last[int(r)] = j
    for j, r in enumerate(idx):
        if 0 <= int(r) < n:
            dest.append(int(r) if last[int(r)] == j else -1)
        else:
            dest.append(n + a)
            a += 1
    return np.array(dest, dtype=np.int64).reshape(len(idx)), a


def place(outs, batch, dest, n, total, appends_only):
    """rfx_hip_upsert_place, in batch order and in place: outs[k][dest[j]] = batch[k][j] where 0 <= dest[j] < total (appends_only[k]: n <= dest[j]);
    dest None: every row appended in order"""
    d = n + np.arange(len(batch[0]), dtype=np.int64) if dest is None else np.asarray(dest, dtype=np.int64)
    for o, b, ao in zip(outs, batch, appends_only):
        ok = (d >= (n if ao else 0)) & (d < total)
        o[d[ok]] = b[ok]


def fill(width, bits, cells):
    """rfx_hip_upsert_fill: `cells` cells of the low `width` bytes of `bits`"""
    return np.full(cells, bits & ((1 << (8 * width)) - 1), dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width])


def null_bits(tp):
    """the cell the planner fills for a column the batch does not provide (Engine._upsert), as the bits handed to the fill"""
    return int(as_bits(np.array([nullv(tp)], dtype=DTYPE[tp]))[0])


def rebuilt(c, counts=None):
    """a case's answer as the planner composes it (rfx_exec_upsert.c upsert_cols): index -> plan -> the table's cells, the fill of the columns not
    provided, the place -- key columns appends only; a DICT's missing column a filled null vector that is placed as a value column"""
    table, batch = inputs(c)
    cols, nulled = ordered(c, batch)
    n, m, keys = c["n"], c["m"], c["keys"]
    dest, a = (None, m)
    if keys:
        dest, a = plan(index(table, [cols[k] for k in range(keys)], keys), n)
    if counts is not None:
        counts.update(matched=m - a, appended=a)
    outs, placed, given, ao = [], [], [], []
    for i, tp in enumerate(c["types"]):
        width = np.dtype(DTYPE[tp]).itemsize
        o = np.concatenate([table[i], np.zeros(a, dtype=DTYPE[tp])])
        b = cols[i]
        if b is None and nulled and keys:
            b = fill(width, null_bits(tp), m).view(DTYPE[tp])
        if b is None:
            o[n:] = fill(width, null_bits(tp), a).view(DTYPE[tp])
        else:
            placed.append(o)
            given.append(b)
            ao.append(i < keys)
        outs.append(o)
    place(placed, given, dest, n, n + a, ao)
    return [(tp, 0, o) for tp, o in zip(c["types"], outs)]


def find_route(table_key, batch_key):
    """the route rfx_exec_set.c takes for find over one key column: the two scopes' intersection empty -> "disjoint", at most 2^20 wide -> "dense", else "hash" """
    lo, hi = max(int(table_key.min()), int(batch_key.min())), min(int(table_key.max()), int(batch_key.max()))
    return "disjoint" if lo > hi else ("dense" if hi - lo + 1 <= 2**20 else "hash")


# what a `host_` case builds (tests/upsert_door.py host_call), by name -> (verb, the reason the door gives)
HOST_SHAPES = {
    "quoted_symbol": ("upsert", "a quoted symbol"), "insert_quoted_symbol": ("insert", "a quoted symbol"),
    "arity": ("upsert", "not three arguments"), "keys_not_i64": ("upsert", "keys is not an I64 atom"), "keys_zero": ("upsert", "keys < 1"),
    "keys_nine": ("upsert", "more than 8 keys"), "keys_beyond_table": ("upsert", "more keys than the table has columns"),
    "key_f64": ("upsert", "a key column that is not I64 / SYMBOL / TIMESTAMP"), "key_i32": ("upsert", "a key column that is not I64 / SYMBOL / TIMESTAMP"),
    "negative_key_hash": ("upsert", "hash route over a negative key"), "null_key_hash": ("upsert", "hash route over a null"),
    "f64_into_i64": ("upsert", "an F64 cell for an integer column"), "f64_atom_into_i64": ("upsert", "an F64 cell for an integer column"),
    "list_column": ("upsert", "not a vector of a concat type"), "c8_column": ("upsert", "not a vector of a concat type"),
    "guid_column": ("upsert", "not a vector of a concat type"), "enum_column": ("upsert", "not a vector of a concat type"),
    "maplist_column": ("upsert", "not a vector of a concat type"), "parted": ("upsert", "a parted table"),
    "matched_i32": ("upsert", "a matched row for a 1-, 2- or 4-byte value column"), "matched_b8_dict_missing": ("upsert", "a matched row for a 1-, 2- or 4-byte value column"),
    "date_column": ("upsert", "a DATE / TIME column"), "insert_time_column": ("insert", "a DATE / TIME column"), "u8_column": ("upsert", "a U8 column"),
    "insert_record_u8": ("insert", "one record for a U8 column"),
    "record_keys2": ("upsert", "one record under several keys"),
    "absent_i32": ("upsert", "a column not provided whose null is not a cell of its type"),
    "record_dict_absent_i16": ("upsert", "a column not provided whose null is not a cell of its type"),
    "too_many_columns": ("upsert", "more batch columns than the table has"), "unequal_lengths": ("upsert", "batch columns of unequal lengths"),
    "unknown_name": ("upsert", "a DICT name the table does not have"), "dict_keys_not_symbols": ("upsert", "a DICT whose keys are not symbols"),
    "batch_vector": ("upsert", "a batch that is not a LIST, a DICT or a TABLE"), "empty_batch": ("upsert", "a batch of no rows"),
    "not_a_table": ("upsert", "not a table"),
    "insert_short_list": ("insert", "a ragged table"), "insert_empty": ("insert", "a batch of no rows"), "insert_arity": ("insert", "not two arguments"),
    "insert_type": ("insert", "a batch column that is not a vector or an atom of its column's type"),
}


# ... of which these are decided on the device: by the index's route, or once the matched rows are known
DEVICE_DECIDED = ("negative_key_hash", "null_key_hash", "matched_i32", "matched_b8_dict_missing")


def load_cases():
    npz = np.load(GOLDEN)
    blob = npz["blob"]
    arrays = {}
    for line in npz["index"]:  # "key|dtype|shape|offset|bytes": the arrays, cut out of the one blob
        key, *dt, shape, at, nbytes = str(line).split("|")
        arrays[key] = blob[int(at):int(at) + int(nbytes)].view(np.dtype("|".join(dt))).reshape([int(d) for d in shape.split("x")])
    out = []
    for c in json.loads(bytes(npz["cases"]).decode()):
        if not c.get("host"):
            c["out"] = [(o["tp"], o["attrs"], unplanes(arrays[o["key"]], o["tp"])) for o in c["out"]]
        out.append(c)
    return out


def retyped(c, frm, to):
    """the same cells under another type code of the same width (SYMBOL: an interned id cannot travel in a fixture)"""
    return dict(c, name=c["name"] + f"_as{to}", types=[to if tp == frm else tp for tp in c["types"]], out=[(to if tp == frm else tp, a, cells) for tp, a, cells in c["out"]])
