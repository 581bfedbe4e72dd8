"""numpy restatement of the stable multiway merge of sorted runs (include/rfx_hip.h "stable multiway merge", rfx_merge.hip): the merged order is
(sort-key tuple, run, place in run) -- np.lexsort over the runs' keys laid end to end -- and the splitter rule the kernel finds its segments with:
a splitter's co-rank is an upper bound in earlier runs, a lower bound in later ones, its own place in its own run; the sum is its global place.
Cells travel as int64 bit patterns, as in sort_ref.  A run is (key columns in the run's sorted order, local rows, row0)."""
import numpy as np

import sort_ref as R

NULL = -(2**63)


def make_runs(cols, f64s, lens, descending=False):
    """the table `cols` cut into consecutive row ranges of `lens` rows, every range sorted on its own (stable): the runs a sharded sort merges"""
    runs, r0 = [], 0
    for n in lens:
        piece = [np.ascontiguousarray(c[r0:r0 + n], dtype=np.int64) for c in cols]
        rows = R.lex_order(piece, f64s, descending) if n else np.empty(0, np.int64)
        runs.append(([p[rows] for p in piece], rows, r0))
        r0 += n
    return runs


def merge(runs, f64s, descending=False):
    """(global row at every place, raw cell of key column 0 at every place)"""
    nk = len(f64s)
    keys = [np.concatenate([r[0][c] for r in runs]) if runs else np.empty(0, np.int64) for c in range(nk)]
    run = np.concatenate([np.full(len(r[1]), i, np.int64) for i, r in enumerate(runs)])
    pos = np.concatenate([np.arange(len(r[1]), dtype=np.int64) for r in runs])
    glob = np.concatenate([r[1] + r[2] for r in runs]).astype(np.int64)
    us = [(~R.u(k, f) if descending else R.u(k, f)) for k, f in zip(keys, f64s)]
    order = np.lexsort([pos, run] + us[::-1])  # (the LAST key of lexsort is the most significant)
    return glob[order], keys[0][order]


def _tuples(run, f64s, descending):
    """a run's sort-key tuples as one structured array whose order is the tuples' order (big-endian bytes compare like the numbers)"""
    us = [(~R.u(k, f) if descending else R.u(k, f)) for k, f in zip(run[0], f64s)]
    n = len(run[1])
    out = np.empty((n, len(us)), dtype=">u8")
    for c, k in enumerate(us):
        out[:, c] = k
    return np.ascontiguousarray(out).view(f"S{8 * len(us)}").reshape(n) if n else np.empty(0, f"S{8 * len(us)}")


def splitters(runs, f64s, tile, descending=False):
    """every tile-th record of every run: (run, place in run, co-ranks in every run, global place), in (run, place) order"""
    tups = [_tuples(r, f64s, descending) for r in runs]
    out = []
    for a, ta in enumerate(tups):
        for p in range(tile, len(ta), tile):
            co = [p if b == a else int(np.searchsorted(tb, ta[p], side="right" if b < a else "left")) for b, tb in enumerate(tups)]
            out.append((a, p, co, sum(co)))
    return out


# ---------------------------------------------------------------------------------------------------- the cases both test files walk
def run_shapes(tile):
    """run lengths: k = 1, 2, 3, 8, 16; all / some runs empty (first, middle, last); lengths of 1; tile - 1, tile, tile + 1; 1000x apart"""
    return [
        [5], [tile + 1], [3 * tile + 7],
        [tile - 1, tile], [1, 1], [50, 50_000],
        [0, 0, 0], [0, 5, 0], [3, 0, 4], [tile + 1, 0, 700], [0, tile, 2 * tile],
        [1] * 8, [0, 1, tile - 1, tile, tile + 1, 2 * tile + 3, 17, 0],
        [(i * 37) % 300 for i in range(16)], [40] * 15 + [40_000], [tile] * 16,
    ]


F64_SPECIALS = np.concatenate([np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, 1.5, -1.5]).view(np.int64),
                               np.array([0x7FF0000000000123, -0x000FFFFFFFFFFEDD, 0x7FFFFFFFFFFFFFFF, -1, 0x7FF8000000000001], dtype=np.int64)])
KINDS = ("all_equal", "runs_ascending", "runs_descending", "interleaved", "full_i64", "f64_special", "two_columns", "three_columns")


def cells(kind, lens, rng):
    """(key columns over all rows as int64 bit patterns, f64 flags)"""
    n = int(sum(lens))
    run = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    if kind == "all_equal":
        return [np.full(n, 7, np.int64)], [False]
    if kind == "runs_ascending":  # run s wholly below run s + 1
        return [run * 1_000_000 + rng.integers(0, 1000, n)], [False]
    if kind == "runs_descending":
        return [-run * 1_000_000 + rng.integers(0, 1000, n)], [False]
    if kind == "interleaved":
        return [rng.integers(0, 50, n)], [False]
    if kind == "full_i64":
        c = rng.integers(-(2**63), 2**63 - 1, n)
        return [np.where(rng.random(n) < 0.1, NULL, c)], [False]
    if kind == "f64_special":
        c = (rng.standard_normal(n) * 10).round(1).view(np.int64)
        return [np.where(rng.random(n) < 0.4, rng.choice(F64_SPECIALS, n), c)], [True]
    if kind == "two_columns":  # heavy ties in the leading column
        return [rng.integers(0, 3, n), rng.choice(F64_SPECIALS, n)], [False, True]
    return [rng.choice(np.array([np.nan, -0.0, 0.0, 1.5]).view(np.int64), n), rng.integers(0, 2, n), rng.integers(-3, 3, n)], [True, False, False]
