#!/usr/bin/env python
"""Golden bucket verbs from the compiled reference -- build container only.

    python tests/golden/make_bucket_golden.py     # writes tests/golden/bucket_golden.npz

Every case is a Rayfall script run by the reference BINARY (oracle/ref.py Session): the operands go in as column files carrying their type code
(2 U8, 3 I16, 4 I32, 5 I64, 7 DATE, 8 TIME, 9 TIMESTAMP, 10 F64), an atom operand is (first v) of a one-cell vector of its type (a -U8 atom: a cast literal), and one of
(xrank x y) (xbar x y) (within x y) (floor x) (ceil x) (round x) (neg x) is evaluated; the answer comes back as a column file whose header gives its
type code.  An xrank case with an attribute sorts its key in the reference first -- (asc x) / (desc x) carry ATTR_ASC / ATTR_DESC -- and the fixture
keeps the SORTED cells as the case's x.  Each case runs with one thread and with eight (pool_map's chunk boundaries are crossed): the verbs are pure
maps, or a stable sort and a map, so the two runs must agree bit for bit -- the maker stops at a case that does not.

The cells where XBARI32 / XBARI64's `x + 1 - y` overflows its type are kept out (undefined in the reference).

The fixture is data only:
  cases      "name|verb|x type|y type|x atom|y atom|attrs|answer type|threads|tiled"   (y type 0: a unary verb)
  c<k>_x c<k>_y c<k>_out    the cells as byte planes (uint8, shape (cell bytes, cells)).  Long operands are a pattern of 800 cells repeated; where an
                            array IS such a repetition, `tiled` lists it as tag:length and the fixture holds the pattern only"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
from bucket_ref import DTYPE, I32, I64, DATE, TIME, TS, F64, NULL32, NULL64  # noqa: E402

U8, I16 = 2, 3
LENS = (0, 1, 63, 64, 65, 4097, 20011)
BIG = 2**20 + 5
P63 = 2.0**63


def tiled(a):
    """a long operand as a pattern of 800 cells repeated: the answers of a map repeat with it, which keeps the fixture small on disk"""
    return np.resize(a[:800], a.size) if a.size > 2000 else a


def ints(rng, n, tp, lo, hi, nulls=True):
    a = rng.integers(lo, hi, n).astype(DTYPE[tp])
    if nulls and n:
        a[rng.integers(0, n, max(1, n // 16))] = NULL32 if DTYPE[tp] == np.int32 else NULL64
    return tiled(a)


F_EDGE = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.0, -0.0, 0.49999999999999994, -0.49999999999999994, np.nan, -np.nan, np.inf, -np.inf,
                   np.nextafter(P63, 0), P63, np.nextafter(P63, np.inf), -np.nextafter(P63, 0), -P63, np.nextafter(-P63, -np.inf), 1e30, -1e30,
                   4503599627370495.5, -4503599627370495.5, 4503599627370496.0, 9007199254740993.0, 1e-310, -1e-310, 3.0, -3.0])


def floats(rng, n, edge=True, divisor=False):
    a = (rng.random(n) - 0.5) * 10.0 ** rng.integers(-2, 6, n)
    if n:
        a[rng.integers(0, n, max(1, n // 16))] = np.nan
    if edge and n >= 63:
        a[: F_EDGE.size] = F_EDGE
    if divisor and n:  # short decimals, zeros of either sign among them
        a = np.where(np.isnan(a), a, np.round(a, 2))
        a[rng.integers(0, n, max(1, n // 10))] = 0.0
        a[rng.integers(0, n, max(1, n // 20))] = -0.0
    return tiled(a)


def cases():
    rng = np.random.default_rng(20261021)
    out = []

    def add(name, verb, x, xt, y=None, yt=0, xa=False, ya=False, attrs=0):
        out.append(dict(name=name, verb=verb, x=np.ascontiguousarray(x, dtype=DTYPE[xt]), xt=xt, y=None if y is None else np.ascontiguousarray(y, dtype=DTYPE[yt]),
                        yt=yt, xa=xa, ya=ya, attrs=attrs))

    # ---- xrank
    for n in LENS:
        add(f"xrank_ties_len{n}", "xrank", rng.integers(0, 8, n), I64, [10], I64, ya=True)
    n = 4097
    add("xrank_all_equal", "xrank", np.full(n, 7), I64, [10], I64, ya=True)
    add("xrank_nulls_negative", "xrank", ints(rng, n, I64, -50, 50), I64, [4], I64, ya=True)
    add("xrank_wide_negative", "xrank", rng.integers(-2**62, 2**62, n), I64, [10], I64, ya=True)
    add("xrank_timestamp", "xrank", ints(rng, n, TS, 0, 10**15), TS, [10], I64, ya=True)
    f = rng.random(n) * 100 - 50
    f[:8] = [np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 0.0, -0.0]
    f[100:140] = np.nan
    add("xrank_f64_specials", "xrank", f, F64, [10], I64, ya=True)
    for ln in (65, 4097):
        keys = rng.integers(-20, 20, ln)
        for nb in (1, 2, 3, 10, ln - 1, ln, 2 * ln):
            add(f"xrank_len{ln}_n{nb}", "xrank", keys, I64, [nb], I64, ya=True)
    keys = rng.integers(0, 30, 65)
    add("xrank_n_i32", "xrank", keys, I64, [7], I32, ya=True)
    add("xrank_n_i16", "xrank", keys, I64, [7], I16, ya=True)
    add("xrank_n_u8", "xrank", keys, I64, [200], U8, ya=True)
    for ln in (0, 1, 65, 4097):
        for attrs, nm in ((2, "asc"), (4, "desc")):
            add(f"xrank_{nm}_ties_len{ln}", "xrank", rng.integers(0, 8, ln), I64, [10], I64, ya=True, attrs=attrs)
    for attrs, nm in ((2, "asc"), (4, "desc")):
        add(f"xrank_{nm}_f64", "xrank", f[:300], F64, [3], I64, ya=True, attrs=attrs)
        add(f"xrank_{nm}_n2len", "xrank", rng.integers(0, 8, 65), I64, [130], I64, ya=True, attrs=attrs)
    add("xrank_big_descending", "xrank", BIG - 1 - np.arange(BIG, dtype=np.int64), I64, [10], I64, ya=True)  # (byte planes that compress)

    # ---- xbar: every arm, vector (x) atom, atom (x) vector, vector (x) vector
    small = {I32: 2**20, DATE: 2**20, TIME: 2**20, I64: 2**40, TS: 2**40}
    arms = [(I32, I32), (I32, I64), (I32, F64), (I64, I32), (I64, I64), (I64, F64), (F64, I32), (F64, I64), (F64, F64), (DATE, I32), (DATE, I64),
            (TIME, I32), (TIME, I64), (TIME, TIME), (TS, I32), (TS, I64), (TS, TIME)]

    def operand(tp, n, divisor):
        if tp == F64:
            return floats(rng, n, edge=not divisor, divisor=divisor)
        if divisor:
            a = ints(rng, n, tp, -9, 10)
            return a
        return ints(rng, n, tp, -small[tp], small[tp])

    def atoms(tp):
        if tp == F64:
            return [0.25, -2.5, 0.0, np.nan, 1e-300]
        return [7, -3, 0, NULL32 if DTYPE[tp] == np.int32 else NULL64]

    for xt, yt in arms:
        nm = f"xbar_{xt}x{yt}"
        for k, a in enumerate(atoms(yt)):
            add(f"{nm}_va{k}", "xbar", operand(xt, 65, False), xt, [a], yt, ya=True)
        for k, a in enumerate([-1000003, 12345, 0] if xt != F64 else [-1000.75, 1e30, np.nan]):
            add(f"{nm}_av{k}", "xbar", [a], xt, operand(yt, 65, True), yt, xa=True)
        add(f"{nm}_av_null", "xbar", [NULL32 if DTYPE[xt] == np.int32 else (NULL64 if xt != F64 else np.nan)], xt, operand(yt, 65, True), yt, xa=True)
        add(f"{nm}_vv", "xbar", operand(xt, 4097, False), xt, operand(yt, 4097, True), yt)
    add("xbar_date_i64_narrowing", "xbar", ints(rng, 65, DATE, -2**20, 2**20), DATE, [2**33 + 5], I64, ya=True)  # (a negative day floors to -(2^33 + 5): stored truncated)
    add("xbar_time_i64_narrowing", "xbar", ints(rng, 65, TIME, -2**20, 2**20), TIME, [-(2**33) - 5], I64, ya=True)
    big = np.array([1e30, -1e30, 2.0**63, -(2.0**63), 1e19, -1e19, 5.0, -5.0, 0.0, -0.0, np.inf, -np.inf, np.nan])
    add("xbar_f64_beyond_2p63", "xbar", big, F64, [1.0], F64, ya=True)
    add("xbar_f64_beyond_2p63_tiny_y", "xbar", big, F64, [1e-10], F64, ya=True)
    add("xbar_f64_y_zero", "xbar", big, F64, [0.0], F64, ya=True)
    add("xbar_f64_y_negzero", "xbar", big, F64, [-0.0], F64, ya=True)
    add("xbar_f64_y_inf", "xbar", big, F64, [np.inf], F64, ya=True)
    for n in LENS:
        add(f"xbar_ts_i64_len{n}", "xbar", ints(rng, n, TS, -2**40, 2**40), TS, [5000], I64, ya=True)
        add(f"xbar_f64_f64_len{n}", "xbar", floats(rng, n), F64, operand(F64, n, True), F64)
        add(f"xbar_i32_i32_len{n}", "xbar", ints(rng, n, I32, -2**20, 2**20), I32, operand(I32, n, True), I32)
        add(f"xbar_time_i64_len{n}", "xbar", ints(rng, n, TIME, -2**20, 2**20), TIME, [1000], I64, ya=True)
    add("xbar_ts_i64_big", "xbar", ints(rng, BIG, TS, -2**40, 2**40), TS, [5000], I64, ya=True)
    add("xbar_f64_f64_big", "xbar", floats(rng, BIG), F64, [0.25], F64, ya=True)
    add("xbar_date_i32_big", "xbar", ints(rng, BIG, DATE, -2**20, 2**20), DATE, operand(I32, BIG, True), I32)

    # ---- floor / ceil / round
    for verb in ("floor", "ceil", "round"):
        add(f"{verb}_edges", verb, F_EDGE, F64)
        for n in LENS:
            add(f"{verb}_len{n}", verb, floats(rng, n), F64)
        add(f"{verb}_big", verb, floats(rng, BIG), F64)

    # ---- neg
    for n in LENS:
        add(f"neg_i32_len{n}", "neg", ints(rng, n, I32, -2**31 + 1, 2**31), I32)
        add(f"neg_i64_len{n}", "neg", ints(rng, n, I64, -2**62, 2**62), I64)
        add(f"neg_f64_len{n}", "neg", floats(rng, n), F64)
    add("neg_i64_extremes", "neg", [NULL64, NULL64 + 1, 2**63 - 1, 0, -1], I64)
    add("neg_i32_extremes", "neg", [NULL32, NULL32 + 1, 2**31 - 1, 0, -1], I32)
    add("neg_i32_big", "neg", ints(rng, BIG, I32, -2**31 + 1, 2**31), I32)
    add("neg_f64_big", "neg", floats(rng, BIG), F64)

    # ---- within
    for n in LENS:
        add(f"within_len{n}", "within", ints(rng, n, I64, 0, 1000), I64, [10, 500], I64)
    col = ints(rng, 4097, I64, -1000, 1000)
    add("within_lo_gt_hi", "within", col, I64, [500, 10], I64)
    add("within_lo_null", "within", col, I64, [NULL64, 0], I64)
    add("within_hi_null", "within", col, I64, [0, NULL64], I64)
    add("within_both_null", "within", col, I64, [NULL64, NULL64], I64)
    add("within_all", "within", col, I64, [NULL64, 2**63 - 1], I64)
    add("within_negative", "within", col, I64, [-300, -5], I64)
    add("within_big", "within", ints(rng, BIG, I64, 0, 1000), I64, [10, 500], I64)

    # ---- xbar, f64 middle type, by an ATOM whose reciprocal is inexact, at lengths that cross pool_map's chunk edges and leave a vector remainder.
    # Three cells in four are picked (in IEEE arithmetic, here) so that x / y and x * (1 / y) floor to DIFFERENT integers: a true division anywhere
    # in the compiled loop -- a chunk's head, its scalar tail -- would show in the answer (the usual pattern of 800 cells, repeated).
    def splitting(n, y, integers):
        k = rng.integers(-2**40, 2**40, 400000).astype(np.float64)
        c = k if integers else k * y
        if not integers:
            c = np.concatenate([c, np.nextafter(c, np.inf), np.nextafter(c, -np.inf)])
        pick = c[np.floor(c / y) != np.floor(c * (1.0 / y))][:600]
        assert pick.size == 600, (y, pick.size)
        plain = rng.integers(-2**40, 2**40, 200).astype(np.float64) * (1.0 if integers else 0.37)
        if not integers:
            plain[:12] = np.nan
        pat = rng.permutation(np.concatenate([pick, plain]))
        return np.resize(pat, n)

    for n in (4097, 20011, BIG):
        add(f"xbar_f64_atom_i64_7_len{n}", "xbar", splitting(n, 7.0, False), F64, [7], I64, ya=True)
        add(f"xbar_f64_atom_f64_0.7_len{n}", "xbar", splitting(n, 0.7, False), F64, [0.7], F64, ya=True)  # (0.3 and 0.6 split no cell of this kind)
        add(f"xbar_i64_atom_f64_0.7_len{n}", "xbar", splitting(n, 0.7, True), I64, [0.7], F64, ya=True)
    return out


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    return np.frombuffer(body, DTYPE[tp], n).copy(), tp, attrs


def run_case(c, threads):
    with ref.Session() as s:
        s.put("x", c["x"], tp=c["xt"])
        if c["y"] is not None:
            s.put("y", c["y"], tp=c["yt"])
        if c["attrs"]:
            s.eval("(set x (asc x))" if c["attrs"] == 2 else "(set x (desc x))")
            s.out("xs", "x")
        xx = "(first x)" if c["xa"] else "x"
        yy = "(first y)" if c["ya"] else "y"
        if c["ya"] and c["yt"] == U8:  # ((first v) of a U8 vector answers a b8 atom in the reference: the u8 atom is cast from a literal)
            yy = f"(as 'u8 {int(c['y'][0])})"
        s.out("r", f"({c['verb']} {xx})" if c["y"] is None else f"({c['verb']} {xx} {yy})")
        s.run(threads=threads)
        r, rt, _ = read_file(os.path.join(s.dir, "out_r"))
        xs = read_file(os.path.join(s.dir, "out_xs")) if c["attrs"] else None
        return r, rt, xs


def is_tiled(a):
    return a.size > 2000 and same(a, np.resize(a[:800], a.size))


def planes(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return np.ascontiguousarray(a.view(np.uint8).reshape(-1, a.dtype.itemsize).T)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    assert ref.build() or ref.available()
    arrays, names = {}, []
    for c in cases():
        k = len(names)
        one, eight = run_case(c, 1), run_case(c, 8)
        assert same(one[0], eight[0]) and one[1] == eight[1], f"{c['name']}: 1 and 8 threads differ"
        x = c["x"]
        if c["attrs"]:
            assert same(one[2][0], eight[2][0]) and one[2][1] == c["xt"] and (one[2][2] & 6) == c["attrs"], c["name"]
            x = one[2][0]
        tiles = []
        for tag, a in (("x", x), ("y", c["y"]), ("out", one[0])):
            if a is None:
                continue
            if is_tiled(a):  # a pattern of 800 cells repeated (a map's answer repeats with its operands): the pattern and the length
                tiles.append(f"{tag}:{a.size}")
                a = a[:800]
            arrays[f"c{k}_{tag}"] = planes(a)
        names.append(f"{c['name']}|{c['verb']}|{c['xt']}|{c['yt']}|{int(c['xa'])}|{int(c['ya'])}|{c['attrs']}|{one[1]}|1,8|{','.join(tiles)}")
        print(c["name"], x.size, "->", one[0].size, "type", one[1])
    arrays["cases"] = np.array(names)
    path = os.path.join(HERE, "bucket_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
