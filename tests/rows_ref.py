"""The row verbs restated in numpy -- filter (ray_filter, core/items.c:338-396), take (ray_take, core/items.c:398-734), reverse (ray_reverse,
core/compose.c:144-202) -- and the loader of tests/golden/rows_golden.npz, the compiled reference's own answers.  These are copies: cells, type code
and attributes must agree bit for bit.  Test infrastructure only."""
import os

import numpy as np

B8, I16, I32, I64, SYMBOL, DATE, TIME, TS, F64 = 1, 3, 4, 5, 6, 7, 8, 9, 10
DTYPE = {B8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, SYMBOL: np.int64, DATE: np.int32, TIME: np.int32, TS: np.int64, F64: np.float64}
ROW_TYPES = (I64, SYMBOL, TS, F64, I32, DATE, TIME, B8)
ATTR_DISTINCT, ATTR_ASC, ATTR_DESC = 1, 2, 4
NULL32, NULL64 = -(2**31), -(2**63)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_golden.npz")


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the verbs: columns are (type code, attrs, cells) triples ----
def filter_cells(cells, mask):
    """any non-zero mask byte selects its row"""
    return cells[np.asarray(mask).view(np.uint8) != 0]


def take_window(l, count):
    """count: ("atom", type, value) or ("range", start, amount) -> (first cell, cells), as ray_take computes them; None where the reference raises an
    error or divides by the length"""
    if count[0] == "range":
        start, m = int(count[1]), int(count[2])
        if m < 0:
            return None
        if start < 0:
            start += l
        start = min(max(start, 0), l)
        m = min(m, l - start)
        return start, m
    if count[1] not in (I64, I32, I16) or l == 0:
        return None
    c = int(count[2])
    m = abs(c)
    return ((l - m % l) % l if c < 0 else 0), m


def take_cells(cells, count):
    j0, m = take_window(len(cells), count)
    if m == 0:
        return cells[:0].copy()
    if j0 + m <= len(cells):
        return cells[j0:j0 + m].copy()
    return cells[(j0 + np.arange(m, dtype=np.int64)) % len(cells)]


def reverse_attrs(attrs):
    return (attrs & ~(ATTR_ASC | ATTR_DESC)) | (ATTR_DESC if attrs & ATTR_ASC else 0) | (ATTR_ASC if attrs & ATTR_DESC else 0)


def answer(c):
    """a fixture case -> the answer's columns [(type, attrs, cells)]"""
    if c["verb"] == "filter":
        return [(tp, 0, filter_cells(cells, c["mask"])) for tp, _a, cells in c["cols"]]
    if c["verb"] == "take":
        if c["atom"]:
            m = abs(int(c["count"][2])) if c["count"][0] == "atom" else int(c["count"][2])
            return [(tp, 0, np.repeat(cells[:1], m)) for tp, _a, cells in c["cols"]]
        return [(tp, 0, take_cells(cells, c["count"])) for tp, _a, cells in c["cols"]]
    return [(tp, reverse_attrs(a), cells[::-1].copy()) for tp, a, cells in c["cols"]]


# ---- the fixture ----
def planes(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return np.ascontiguousarray(a.view(np.uint8).reshape(-1, a.dtype.itemsize).T)


def unplanes(p, tp):
    return np.ascontiguousarray(p.T).reshape(-1).view(DTYPE[tp]).copy()


def count_text(count):
    return "" if count is None else ":".join(str(x) for x in count)


def count_of(text):
    if not text:
        return None
    kind, a, b = text.split(":")
    return (kind, int(a), int(b))


def load_cases():
    """-> [dict(name, verb, table, atom, names, cols [(type, attrs, cells)], mask, count, out [(type, attrs, cells)] or None, host: the reason a shape is
    handed to the host (the reference's own answer there: `ref_error`), threads)]"""
    npz = np.load(GOLDEN)
    blob, z = npz["blob"], {"cases": npz["cases"]}
    for line in npz["index"]:  # "key|dtype|shape|offset|bytes": the arrays, cut out of the one blob
        key, *dt, shape, at, nbytes = str(line).split("|")  # (a dtype string may itself hold a bar: "|u1")
        dt = "|".join(dt)
        z[key] = blob[int(at):int(at) + int(nbytes)].view(np.dtype(dt)).reshape([int(d) for d in shape.split("x")])
    out = []
    for k, line in enumerate(z["cases"]):
        name, verb, table, atom, names, colmeta, count, outmeta, host, ref_error, threads = str(line).split("|")
        c = dict(name=name, verb=verb, table=table == "1", atom=atom == "1", names=names.split(",") if names else [], count=count_of(count),
                 host=host or None, ref_error=ref_error == "1", threads=threads)
        c["cols"], c["alias"] = [], []
        for j, m in enumerate(colmeta.split(",") if colmeta else []):
            tp, attrs, *alias = (int(v) for v in m.split(":"))
            c["alias"].append(alias[0] if alias else -1)  # (>= 0: the very vector of that column, under another name)
            c["cols"].append((tp, attrs, unplanes(z[f"c{k}_x{j}"], tp) if f"c{k}_x{j}" in z else np.empty(0, DTYPE.get(tp, np.int64))))
        c["mask"] = z[f"c{k}_m"] if f"c{k}_m" in z else None
        c["out"] = None
        if outmeta:
            c["out"] = []
            for j, m in enumerate(outmeta.split(",")):
                tp, attrs = (int(v) for v in m.split(":"))
                c["out"].append((tp, attrs, unplanes(z[f"c{k}_o{j}"], tp)))
        out.append(c)
    return out
