#!/usr/bin/env python
"""Golden window joins from the compiled reference -- build container only.

    python tests/golden/make_wj_golden.py     # writes tests/golden/wj_golden.npz

Every case is a Rayfall script run by the reference binary (oracle/ref.py Session): both tables and the two window vectors go in as column files
(TIME cells with type code 8), `(window-join [keys t] (list lo hi) L R {...})` and `(window-join1 ...)` are evaluated with all seven aggregates
over an I64 and an F64 value column, and every result column comes back as a column file.  Each case runs with one thread and with eight, and the
two runs must agree bit for bit; the empty-left case runs with one thread only (with more workers the reference divides by zero there).
The fixture is data only:
  cases             "name|number of equality keys|key kind (i64 / sym)|threads it ran with"
  symbols           the strings SYMBOL key cells index
  c<k>_lk<j> c<k>_rk<j>   equality keys of both sides;  c<k>_lt c<k>_rt  the TIME columns;  c<k>_lo c<k>_hi  the window bounds (4-byte cells, sign-extended)
  c<k>_vi c<k>_vf   the right table's I64 value column and the BITS of its F64 one
  c<k>_out          the answers, [verb (window-join, window-join1)][value column (vi, vf)][aggregate (AGGS)][left row], F64 answers as bits
Every array of cells is kept as its eight byte planes (uint8, shape (8, cells): plane b holds byte b of every cell; tests/wj_ref.py unplanes reads
them back): the high bytes of small numbers are constant, and the file stays small.
F64 cells are multiples of 1/8 of small magnitude: their sums are exact in any order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402

NULL = -(2**63)
NULL32 = -(2**31)
AGGS = ("sum", "min", "max", "count", "avg", "first", "last")
SYMS = ["apple", "pear", "fig", "kiwi", "plum", "absent"]  # (the last one never occurs in a right table)


def values(rng, n, pnull=0.05):
    vi = rng.integers(-40, 40, n)
    vf = rng.integers(-40, 40, n) / 8.0
    vi[rng.random(n) < pnull] = NULL
    vf[rng.random(n) < pnull] = np.nan
    return vi, vf


def sides(rng, nl, nr, nkeys=1, krange=5, trange=1000, width=60, sort_right=True, shuffle=False, knulls=0.0, tnulls=0.0, absent=0.0, pnull=0.05, kind="i64", tile=0):
    """tile: the left side is a pattern of that many random rows repeated to nl rows -- the answers repeat with it, which is what keeps the
    fixture's large cases small on disk (an avg is a full-mantissa quotient: 8 bytes of entropy per cell otherwise)"""
    want_nl, nl = nl, (min(nl, tile) if tile else nl)
    lk = [rng.integers(0, krange, nl) for _ in range(nkeys)]
    rk = [rng.integers(0, krange, nr) for _ in range(nkeys)]
    lt, rt = rng.integers(0, trange, nl), rng.integers(0, trange, nr)
    if sort_right:
        rt = np.sort(rt)
    if shuffle and nr:  # rows in no order at all: neither by key nor by time
        p = rng.permutation(nr)
        rk, rt = [k[p] for k in rk], rt[p]
    lo = lt - rng.integers(0, width, nl)
    hi = lt + rng.integers(0, width, nl)
    if absent:
        lk[0] = np.where(rng.random(nl) < absent, krange, lk[0])  # (sym: SYMS[krange] is "absent" when krange = 5)
    if knulls:
        for k in lk + rk:
            k[rng.random(len(k)) < knulls] = NULL
    if tnulls:
        for t in (lo, hi, rt):
            t[rng.random(len(t)) < tnulls] = NULL32
    vi, vf = values(rng, nr, pnull)
    if nl != want_nl:
        lk, lt, lo, hi = [np.resize(k, want_nl) for k in lk], np.resize(lt, want_nl), np.resize(lo, want_nl), np.resize(hi, want_nl)
    return dict(kind=kind, lk=lk, rk=rk, lt=lt, lo=lo, hi=hi, rt=rt, vi=vi, vf=vf)


def cases():
    rng = np.random.default_rng(20261018)
    out = []
    # tests/lang.c:4289-4303: trades at 10:00:01 and 10:00:05, quotes at 10:00:00 / :02 / :04 with bids 99 100 101, windows of +-2 s
    t0 = 36_000_000
    lt = np.array([t0 + 1000, t0 + 5000])
    out.append(("lang_examples", dict(kind="sym", lk=[np.array([0, 0])], rk=[np.array([0, 0, 0])], lt=lt, lo=lt - 2000, hi=lt + 2000,
                                      rt=np.array([t0, t0 + 2000, t0 + 4000]), vi=np.array([99, 100, 101]), vf=np.array([99, 100, 101]) / 8.0)))
    sizes = (0, 1, 63, 64, 65, 4097)
    for n in sizes[1:]:
        for m in sizes:
            if (n in (63, 64) and m in (63, 64, 65)) or (n == 4097 and m not in (0, 1, 65)) or (m == 4097 and n not in (1, 65)):
                continue  # (a sample of the pairs: every size appears on both sides)
            out.append((f"sorted_{n}x{m}", sides(rng, n, m, trange=300, width=40, tile=500)))
    out.append(("empty_left", sides(rng, 0, 65)))
    out.append(("sorted_20011x1000", sides(rng, 20011, 1000, krange=20, trange=4000, width=150, tile=700)))
    out.append(("sorted_1000x20011", sides(rng, 1000, 20011, krange=20, trange=4000, width=12)))
    out.append(("shuffled_4097x1500", sides(rng, 4097, 1500, krange=7, trange=600, shuffle=True, tile=500)))
    out.append(("shuffled_65x4097", sides(rng, 65, 4097, krange=3, trange=900, width=30, shuffle=True)))
    out.append(("unsorted_times_400x800", sides(rng, 400, 800, krange=6, sort_right=False)))
    out.append(("sym_keys_sorted", sides(rng, 400, 800, kind="sym", absent=0.15)))
    out.append(("sym_keys_shuffled", sides(rng, 400, 800, kind="sym", absent=0.15, shuffle=True)))
    out.append(("two_keys", sides(rng, 400, 800, nkeys=2, krange=4, absent=0.1, shuffle=True)))
    out.append(("three_keys", sides(rng, 400, 800, nkeys=3, krange=3, absent=0.1, shuffle=True)))
    c = sides(rng, 400, 800, nkeys=2, krange=3, kind="sym", shuffle=True)
    c["kind"] = "sym+i64"  # (a SYMBOL key beside an I64 key)
    out.append(("sym_and_i64_keys", c))
    out.append(("null_keys", sides(rng, 500, 1000, nkeys=2, krange=3, knulls=0.1, shuffle=True)))
    out.append(("null_times", sides(rng, 500, 1000, krange=4, trange=200, width=30, tnulls=0.08, shuffle=True)))
    out.append(("ties", sides(rng, 500, 1000, krange=3, trange=6, width=3)))
    out.append(("all_equal_times", dict(sides(rng, 500, 700, krange=3), rt=np.full(700, 7), lo=rng.integers(5, 9, 500), hi=rng.integers(6, 10, 500))))
    c = sides(rng, 900, 600, krange=4, trange=100)
    c["rt"] = np.sort(rng.integers(400, 500, 600))  # every group lives in [400, 500)
    kind = rng.integers(0, 6, 900)  # wholly before / wholly after / spanning the group / lo > hi / zero width / ending inside
    c["lo"] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [rng.integers(0, 300, 900), rng.integers(500, 700, 900), np.full(900, 100), rng.integers(440, 520, 900),
                                                                                  rng.integers(390, 510, 900)], rng.integers(300, 460, 900))
    c["hi"] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [c["lo"] + rng.integers(0, 99, 900), c["lo"] + rng.integers(0, 99, 900), np.full(900, 900),
                                                                                  c["lo"] - rng.integers(1, 30, 900), c["lo"]], rng.integers(420, 480, 900))
    out.append(("before_after_spanning_reversed_zero_width", c))
    out.append(("mostly_null_cells", sides(rng, 400, 800, krange=4, trange=400, width=8, pnull=0.85)))
    c = sides(rng, 300, 400, krange=3)
    c["vi"][:], c["vf"][:] = NULL, np.nan
    out.append(("all_null_cells", c))
    lens = [1, 2, 3, 64, 65, 1, 2, 3, 64, 65]
    for shuffled in (False, True):
        rk = np.repeat(np.arange(len(lens)), lens)
        rt = np.sort(rng.integers(0, 400, rk.size))
        if shuffled:
            p = rng.permutation(rk.size)
            rk, rt = rk[p], rt[p]
        else:
            rk = rng.permutation(rk)
        c = sides(rng, 500, rk.size, krange=len(lens) + 1, trange=400, width=200)
        c["rk"], c["rt"] = [rk], rt
        out.append((f"group_lengths_{'shuffled' if shuffled else 'sorted'}", c))
        c = sides(rng, 500, 4097, krange=1, trange=9000, width=300, shuffle=shuffled)
        c["lk"], c["rk"] = [np.full(500, 3)], [np.full(4097, 3)]
        c["lo"][:5], c["hi"][:5] = -50, 9050  # (windows over the whole group)
        out.append((f"one_group_{'shuffled' if shuffled else 'sorted'}", c))
    # window lengths around the fold's boundaries: one row per millisecond, so window-join1's window [lo, hi] holds exactly hi - lo + 1 rows (and
    # window-join's the same unless lo is before the group); lengths 0 .. 40, around 64 / 128 / 192 / 256 / 512, starts of both parities
    nr = 1500
    c = sides(rng, 1, nr, krange=1)
    c["rk"], c["rt"] = [np.zeros(nr, np.int64)], np.arange(nr)
    want = np.concatenate([np.arange(0, 41), np.arange(60, 70), np.arange(124, 134), np.arange(188, 196), np.arange(252, 262), np.arange(508, 518), [1000, 1499, 1500]])
    lo = np.concatenate([rng.integers(0, 400, want.size), rng.integers(0, 400, want.size) | 1, rng.integers(0, 400, want.size) & ~1])
    want = np.tile(want, 3)
    c["lk"], c["lo"], c["hi"], c["lt"] = [np.zeros(want.size, np.int64)], lo, lo + want - 1, lo
    out.append(("window_lengths", c))
    return out


def run_case(name, c, threads):
    nk = len(c["lk"])
    kinds = {"i64": ["i64"] * nk, "sym": ["sym"] * nk, "sym+i64": ["sym"] + ["i64"] * (nk - 1)}[c["kind"]]
    with ref.Session() as s:
        s.eval("(set SY [" + " ".join(SYMS) + "])")
        for side in "lr":
            for j in range(nk):
                s.put(f"{side}k{j}", np.ascontiguousarray(c[f"{side}k"][j], dtype=np.int64))
        for n in ("lt", "lo", "hi", "rt"):
            s.put(n, np.ascontiguousarray(c[n], dtype=np.int64).astype(np.int32), tp=8)
        s.put("vi", np.ascontiguousarray(c["vi"], dtype=np.int64))
        s.put("vf", np.ascontiguousarray(c["vf"], dtype=np.float64))
        knames = " ".join(f"k{j}" for j in range(nk))
        col = lambda side, j: f"(at SY {side}k{j})" if kinds[j] == "sym" else f"{side}k{j}"
        s.eval(f"(set L (table [{knames} t] (list {' '.join(col('l', j) for j in range(nk))} lt)))")
        s.eval(f"(set R (table [{knames} t vi vf] (list {' '.join(col('r', j) for j in range(nk))} rt vi vf)))")
        aggs = " ".join(f"{a}_{x}: ({a} v{x})" for x in "if" for a in AGGS)
        for w, verb in enumerate(("window-join", "window-join1")):
            s.eval(f"(set W{w} ({verb} [{knames} t] (list lo hi) L R {{{aggs}}}))")
            for x in "if":
                for a in AGGS:
                    s.out(f"w{w}_{a}_{x}", f"(at W{w} '{a}_{x})")
        res = s.run(threads=threads)
    out = {}
    for k, v in res.items():
        if k == "_stdout":
            continue
        want = np.float64 if (k.endswith("_f") and "count" not in k) or "_avg_" in k else np.int64
        assert v.dtype == want and v.size == len(c["lt"]), (name, k, v.dtype, v.size)
        out[k] = v.view(np.int64)
    return out


def planes(a):
    return np.ascontiguousarray(np.ascontiguousarray(a, dtype=np.int64).reshape(-1).view(np.uint8).reshape(-1, 8).T)


def main():
    assert ref.build() or ref.available()
    arrays, names = {}, []
    for ci, (name, c) in enumerate(cases()):
        one = run_case(name, c, 1)
        threads = "1"
        if len(c["lt"]):
            eight = run_case(name, c, 8)
            assert one.keys() == eight.keys() and all(np.array_equal(one[k], eight[k]) for k in one), name
            threads = "1,8"
        for j, (a, b) in enumerate(zip(c["lk"], c["rk"])):
            arrays[f"c{ci}_lk{j}"], arrays[f"c{ci}_rk{j}"] = planes(a), planes(b)
        for n in ("lt", "lo", "hi", "rt", "vi"):
            arrays[f"c{ci}_{n}"] = planes(c[n])
        arrays[f"c{ci}_vf"] = planes(np.ascontiguousarray(c["vf"], dtype=np.float64).view(np.int64))
        arrays[f"c{ci}_out"] = planes(np.stack([np.stack([np.stack([one[f"w{w}_{a}_{x}"] for a in AGGS]) for x in "if"]) for w in (0, 1)]))
        names.append(f"{name}|{len(c['lk'])}|{c['kind']}|{threads}")
        print(name, len(c["lt"]), len(c["rt"]), "counts", int(one["w0_count_i"].sum()), int(one["w1_count_i"].sum()), "null rows", int((one["w0_count_i"] == 0).sum()))
    arrays["cases"] = np.array(names)
    arrays["symbols"] = np.array(SYMS)
    path = os.path.join(HERE, "wj_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
