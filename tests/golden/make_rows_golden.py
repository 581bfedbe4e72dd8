#!/usr/bin/env python
"""Golden row verbs from the compiled reference -- build container only.

    python tests/golden/make_rows_golden.py     # writes tests/golden/rows_golden.npz

Every case is a Rayfall script run by the reference BINARY (oracle/ref.py Session): the columns go in as column files carrying their type code (1 B8,
4 I32, 5 I64, 7 DATE, 8 TIME, 9 TIMESTAMP, 10 F64; a SYMBOL column cannot travel as a file: the GPU tests run SYMBOL vectors and atoms through the door against the restatement, and the drop-in
test compares them inside the reference), an
atom is (first v) of a one-cell vector of its type, a table is (table [names] (list columns)), and one of (filter x m) (take x c) (reverse x) is
evaluated; every column of the answer comes back as a column file whose header gives its type code and attributes.  A reverse case with attributes
sorts its column in the reference first ((asc x) / (desc x) carry ATTR_ASC / ATTR_DESC; ATTR_DISTINCT | ATTR_ASC comes with (til n) alone, an I64
vector: the other types and B8 get their attributes set on standalone host vectors by the GPU tests) and keeps the sorted cells as the case's x.  Each case runs
with one thread and with eight, and the maker stops at a case where the two differ.  A `host_` case is a shape the device path hands to the host: the
fixture records the shape, the reason, and whether the reference itself answers it with an error (its script then fails).

The fixture is data only (tests/rows_ref.py load_cases reads it): `cases` lines
"name|verb|table|atom|names|x type:attrs[:alias of column],...|count|out type:attrs,...|host reason|reference errors|threads", and per case k the cells
as byte planes c<k>_x<j> / c<k>_o<j> and the mask bytes c<k>_m, all of them in one `blob` of bytes that `index` lines "key|dtype|shape|offset|bytes" cut up.  The long cases are built so that their byte planes repeat (two columns row // P and
row % P under a mask of period P = 20011 name every row, and compress)."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
from rows_ref import B8, I16, I32, I64, DATE, TIME, TS, F64, DTYPE, NULL32, NULL64, planes, count_text  # noqa: E402

LENS = (0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 4097, 20011)
BIG = 2**20 + 5
P = 20011
TYPES = (I64, TS, F64, I32, DATE, TIME, B8)


def cells(rng, n, tp):
    if n > 130:  # long columns name their rows (and compress): 7 * row - 3 * n, every 16th cell a null
        i = np.arange(n, dtype=np.int64)
        if tp == B8:
            return (i % 3 == 0).astype(np.int8)
        if tp == F64:
            return np.where(i % 16 == 5, np.nan, i * 0.5 - n)
        return np.where(i % 16 == 5, NULL64 if DTYPE[tp] == np.int64 else NULL32, i * 7 - 3 * n).astype(DTYPE[tp])
    if tp == F64:
        a = (rng.random(n) - 0.5) * 1e6
        if n:
            a[rng.integers(0, n, max(1, n // 16))] = np.nan
        return a
    if tp == B8:
        return rng.integers(0, 2, n).astype(np.int8)
    wide = DTYPE[tp] == np.int64
    a = rng.integers(-2**40 if wide else -2**31 + 1, 2**40 if wide else 2**31, n).astype(DTYPE[tp])
    if n:
        a[rng.integers(0, n, max(1, n // 16))] = NULL64 if wide else NULL32
    return a


def masks(rng, n):
    """name -> mask bytes"""
    def only(i):
        m = np.zeros(n, np.uint8)
        if 0 <= i < n:
            m[i] = 1
        return m
    out = {"zero": np.zeros(n, np.uint8), "one": np.ones(n, np.uint8), "first": only(0), "last": only(n - 1), "row511": only(511), "row512": only(512),
           "alternating": (np.arange(n) % 2).astype(np.uint8), "every64th": (np.arange(n) % 64 == 0).astype(np.uint8)}
    for pct in (1, 50, 99):
        out[f"random{pct}"] = (rng.random(n) * 100 < pct).astype(np.uint8)
    r = rng.random(n) < 0.5
    for byte in (2, 0x80, 0xFF):
        out[f"true{byte}"] = np.where(r, byte, 0).astype(np.uint8)
    return out


def cases():
    rng = np.random.default_rng(20261019)
    out = []

    def add(name, verb, cols, mask=None, count=None, table=False, atom=False, names=None, host=None, sort=None):
        out.append(dict(name=name, verb=verb, cols=[(tp, np.ascontiguousarray(a, dtype=DTYPE[tp]), alias) for tp, a, alias in cols], mask=mask, count=count,
                        table=table, atom=atom, names=names or [f"c{j}" for j in range(len(cols))] if table else [], host=host, sort=sort))

    def table_cols(n, ncols):
        kinds = [I64, I32, B8, F64, DATE, TS, TIME, I64, F64]
        return [(kinds[j], cells(rng, n, kinds[j]), -1) for j in range(ncols)]

    # ---- filter: every length under a few masks, every mask at the lengths around the bitmap's groups, the chunk and the wave step
    for n in LENS:
        ms = masks(rng, n)
        pick = ms if n in (0, 1, 129, 513, 1025, 20011) else {k: ms[k] for k in ("one", "last", "random50", "true128")}
        for mname, m in pick.items():
            add(f"filter_i64_len{n}_{mname}", "filter", [(I64, cells(rng, n, I64), -1)], mask=m)
    for tp in TYPES:
        for n in (65, 1025, 4097):
            add(f"filter_type{tp}_len{n}", "filter", [(tp, cells(rng, n, tp), -1)], mask=masks(rng, n)["random50"])
    for ncols in (1, 8, 9):
        for n in (513, 4097):
            ms = masks(rng, n)
            for mname in ("random1", "random50", "random99", "zero", "one") if n == 513 else ("random1", "random50"):
                add(f"filter_table{ncols}_len{n}_{mname}", "filter", table_cols(n, ncols), mask=ms[mname], table=True)
    shared = cells(rng, 1025, I32)
    add("filter_table_one_vector_two_names", "filter", [(I32, shared, -1), (I32, shared, 0), (F64, cells(rng, 1025, F64), -1)], mask=masks(rng, 1025)["random50"],
        table=True)
    rows = np.arange(BIG, dtype=np.int64)
    for pct in (1,):  # two columns name every row; both and the mask repeat with period P (50 % and 99 % at this length: the GPU tests, against the restatement)
        tile = (rng.random(P) * 100 < pct).astype(np.uint8)
        add(f"filter_big_random{pct}", "filter", [(I64, rows // P, -1), (I32, rows % P, -1), (B8, (rows % P) % 2, -1)], mask=np.resize(tile, BIG), table=True)
    for mname in ("one", "last", "alternating"):
        add(f"filter_big_{mname}", "filter", [(I64, rows, -1)], mask=masks(rng, BIG)[mname])

    # ---- take
    for l in (1, 2, 63, 64, 65, 4097):
        x = cells(rng, l, I64)
        for k, m in enumerate((0, 1, l - 1, l, l + 1, 2 * l + 3, 7 * l)):
            for sign in (1, -1):
                for ct in (I64, I32, I16):
                    add(f"take_len{l}_m{k}_{'neg' if sign < 0 else 'pos'}_t{ct}", "take", [(I64, x, -1)], count=("atom", ct, sign * m))
        for start in (0, 1, -1, -l, -l - 5, l, l + 5):
            for amount in (0, 1, l, l + 7):
                add(f"take_len{l}_range_{start}_{amount}", "take", [(I64, x, -1)], count=("range", start, amount))
    for tp in TYPES:
        x = cells(rng, 65, tp)
        for c in (("atom", I64, 200), ("atom", I64, -200), ("atom", I64, 7), ("atom", I64, -7), ("range", 3, 20), ("range", -20, 50), ("range", 2, 17)):
            add(f"take_type{tp}_{count_text(c)}", "take", [(tp, x, -1)], count=c)
        add(f"take_atom_type{tp}", "take", [(tp, x[1:2], -1)], count=("atom", I64, 67), atom=True)
        add(f"take_atom_type{tp}_neg", "take", [(tp, x[1:2], -1)], count=("atom", I32, -5), atom=True)
    add("take_atom_zero", "take", [(I64, [7], -1)], count=("atom", I64, 0), atom=True)
    for ncols in (1, 8, 9):
        for c in (("atom", I64, 1000), ("atom", I64, -1000), ("atom", I64, 9000), ("range", 100, 1000), ("range", 101, 1000), ("range", -5, 9)):
            add(f"take_table{ncols}_{count_text(c)}", "take", table_cols(4097, ncols), count=c, table=True)
    for c in (("atom", I64, -1000), ("range", BIG - 5003, 70000)):
        add(f"take_big_{count_text(c)}", "take", [(I64, rows, -1), (I32, rows % P, -1)], count=c, table=True)

    # ---- reverse
    for tp in TYPES:
        for n in (0, 1, 65, 4097):
            add(f"reverse_type{tp}_len{n}", "reverse", [(tp, cells(rng, n, tp), -1)])
        if tp != B8:
            for sort in ("asc", "desc") + (("distinct_asc",) if tp == I64 else ()):  # ((til n) alone carries ATTR_DISTINCT | ATTR_ASC: an I64 vector)
                add(f"reverse_type{tp}_{sort}", "reverse", [(tp, cells(rng, 129, tp), -1)], sort=sort)
    for n in LENS:
        add(f"reverse_i64_len{n}", "reverse", [(I64, cells(rng, n, I64), -1)])
    add("reverse_big", "reverse", [(I64, rows, -1)])

    # ---- shapes handed to the host (type codes beyond the row types: U8 2, I16 3, GUID 11, C8 12, ENUM 20, MAPLIST 75, LIST 0, DICT 99)
    x = cells(rng, 10, I64)
    m10 = masks(rng, 10)["random50"]
    for verb in ("filter", "take", "reverse"):
        for code, nm in ((2, "u8"), (3, "i16"), (11, "guid"), (12, "c8"), (20, "enum"), (75, "maplist"), (0, "list"), (99, "dict")):
            out.append(dict(name=f"host_{verb}_{nm}", verb=verb, cols=[(code, np.empty(0, np.int64), -1)], mask=m10 if verb == "filter" else None,
                            count=("atom", I64, 3) if verb == "take" else None, table=False, atom=False, names=[], host="not a vector of a row type", sort=None))
        if verb != "reverse":
            out.append(dict(name=f"host_{verb}_parted_table", verb=verb, cols=[(77 + I64, np.empty(0, np.int64), -1)], mask=m10 if verb == "filter" else None,
                            count=("atom", I64, 3) if verb == "take" else None, table=True, atom=False, names=["c0"], host="a parted table", sort=None))
            out.append(dict(name=f"host_{verb}_table_no_columns", verb=verb, cols=[], mask=m10 if verb == "filter" else None,
                            count=("atom", I64, 3) if verb == "take" else None, table=True, atom=False, names=[], host="a table with no columns", sort=None))
    add("host_filter_mask_not_b8", "filter", [(I64, x, -1)], mask=("i64", np.arange(10, dtype=np.int64) % 2), host="a mask that is not a B8 vector")
    add("host_filter_lengths_differ", "filter", [(I64, x, -1)], mask=m10[:9], host="length")
    add("host_take_negative_amount", "take", [(I64, x, -1)], count=("range", 1, -2), host="a negative range amount")
    add("host_take_count_f64", "take", [(I64, x, -1)], count=("atom", F64, 2), host="count type")
    add("host_take_count_b8", "take", [(I64, x, -1)], count=("atom", B8, 1), host="count type")
    add("host_take_empty_vector", "take", [(I64, x[:0], -1)], count=("atom", I64, 3), host="take from an empty vector")
    add("host_take_empty_vector_zero", "take", [(I64, x[:0], -1)], count=("atom", I64, 0), host="take from an empty vector")
    add("host_take_empty_table", "take", [(I64, x[:0], -1), (F64, cells(rng, 0, F64), -1)], count=("atom", I64, -3), table=True, host="take from an empty table")
    add("host_take_int64_min", "take", [(I64, x, -1)], count=("atom", I64, NULL64), host="a count of INT64_MIN")
    add("host_take_range_overflow", "take", [(I64, x, -1)], count=("range", 2**62, 2**62), host="start + amount does not fit 63 bits")
    add("host_reverse_table", "reverse", [(I64, x, -1)], table=True, host="a table")
    return out


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    return np.frombuffer(body, DTYPE[tp], n).copy(), tp, attrs


def script(s, c):
    """the case's objects and call in a Session; -> (expression, the columns' names whose sorted cells come back)"""
    for j, (tp, a, alias) in enumerate(c["cols"]):
        if alias < 0:
            s.put(f"x{j}", a, tp=tp)
        else:
            s.eval(f"(set x{j} x{alias})")
    back = []
    if c["sort"]:
        s.eval({"asc": "(set x0 (asc x0))", "desc": "(set x0 (desc x0))", "distinct_asc": "(set x0 (til 129))"}[c["sort"]])
        s.out("xs", "x0")
        back.append("xs")
    if c["table"]:
        s.eval(f"(set x (table [{' '.join(c['names'])}] (list {' '.join(f'x{j}' for j in range(len(c['cols'])))})))")
        xx = "x"
    else:
        xx = "(first x0)" if c["atom"] else "x0"
    if c["verb"] == "reverse":
        return f"(reverse {xx})", back
    if c["verb"] == "filter":
        m = c["mask"]
        if isinstance(m, tuple):
            s.put("m", m[1])
        else:
            s.put("m", m.view(np.int8), tp=B8)
        return f"(filter {xx} m)", back
    kind, a, b = c["count"]
    if kind == "range":
        return f"(take {xx} [{a} {b}])", back
    if a == F64:
        return f"(take {xx} {float(b)})", back
    s.put("n", np.array([b], dtype=DTYPE[a]), tp=a)
    return f"(take {xx} (first n))", back


def run_case(c, threads):
    with ref.Session() as s:
        expr, back = script(s, c)
        s.eval(f"(set r {expr})")
        if c["table"]:
            for j, nm in enumerate(c["names"]):
                s.out(f"o{j}", f"(at r '{nm})")
        else:
            s.out("o0", "r")
        s.run(threads=threads)
        outs = [read_file(os.path.join(s.dir, f"out_o{j}")) for j in range(max(1, len(c["names"])))]
        xs = read_file(os.path.join(s.dir, "out_xs")) if back else None
        return outs, xs


def reference_errors(c):
    """a host_ case the reference can be asked: does its own verb answer an error?  (its script fails then)"""
    try:
        run_case(c, 1)
        return False
    except RuntimeError:
        return True


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    assert ref.build() or ref.available()
    arrays, lines = {}, []
    for c in cases():
        k = len(lines)
        cols = [(tp, 0, a, alias) for tp, a, alias in c["cols"]]
        outmeta, ref_error = "", 0
        askable = c["host"] in ("a mask that is not a B8 vector", "length", "a negative range amount", "count type", "a table") and c["name"] != "host_take_count_b8"
        if c["host"] is None:
            try:
                one, eight = run_case(c, 1), run_case(c, 8)
            except RuntimeError:
                print("the reference failed at", c["name"])
                raise
            assert len(one[0]) == len(eight[0]) and all(same(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(one[0], eight[0])), f"{c['name']}: 1 and 8 threads differ"
            if c["sort"]:
                assert same(one[1][0], eight[1][0]) and one[1][1:] == eight[1][1:], c["name"]
                cols = [(cols[0][0], one[1][2], one[1][0], -1)]
            for j, (a, tp, attrs) in enumerate(one[0]):
                arrays[f"c{k}_o{j}"] = planes(a)
            outmeta = ",".join(f"{tp}:{attrs}" for _a, tp, attrs in one[0])
        elif askable:
            ref_error = int(reference_errors(c))
            assert ref_error, c["name"]
        for j, (tp, attrs, a, alias) in enumerate(cols):
            if tp in DTYPE and a.size:
                arrays[f"c{k}_x{j}"] = planes(a)
        if c["mask"] is not None:
            arrays[f"c{k}_m"] = c["mask"][1] if isinstance(c["mask"], tuple) else c["mask"]
        colmeta = ",".join(f"{tp}:{attrs}" + (f":{alias}" if alias >= 0 else "") for tp, attrs, _a, alias in cols)
        lines.append(f"{c['name']}|{c['verb']}|{int(c['table'])}|{int(c['atom'])}|{','.join(c['names'])}|{colmeta}|{count_text(c['count'])}|{outmeta}|{c['host'] or ''}|{ref_error}|1,8")
        if k % 100 == 0:
            print(k, c["name"])
    # one blob and an index instead of a few thousand members: the archive's per-member headers would outweigh the cells
    index, parts, at = [], [], 0
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        index.append(f"{key}|{a.dtype.str}|{'x'.join(str(d) for d in a.shape)}|{at}|{a.nbytes}")
        parts.append(a.reshape(-1).view(np.uint8))
        at += a.nbytes
    path = os.path.join(HERE, "rows_golden.npz")
    np.savez_compressed(path, cases=np.array(lines), index=np.array(index), blob=np.concatenate(parts) if parts else np.empty(0, np.uint8))
    print("wrote", len(lines), "cases,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2**20


if __name__ == "__main__":
    main()
