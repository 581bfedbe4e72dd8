"""Timing of the device window join on the shape of the reference's own benchmark (examples/wj.rfl: n trades, 2 n quotes, windows of +-1 s holding
about 5 000 quotes of the trade's symbol, {bid: (min Bid) ask: (max Ask)}).  Per size, the median of --steps timed steps after --warmup, a device
synchronise inside every timed region:
  ranges_ms   rfx_exec_window_ranges on device columns: the build side (group ids, the two-column sort, run boundaries, times gathered) and the probe
              (the left rows' groups, two searches and the null tests per row)
  fold_ms     rfx_exec_window_fold of both value columns (the gather into the sorted order + one launch each), from the ranges above
  door_ms     the whole verb, rfx_window_join over host tables whose columns are resident from the warm-up call (the residency cache), result table
              with its two new host vectors included; door1_ms the same for rfx_window_join1
The yardstick, named for what it is: `ref_window_join_ms_threads8` / `_threads1`, the compiled reference's own `(window-join ...)` over the same
tables on this box's CPU (oracle/_ref/rayforce -c 8 / -c 1, its own `timeit`, column files loaded outside the timed expression), for the sizes named
by --ref-sizes (the reference needs minutes at 1e7).  One JSON line per size.

    python tools/bench_wj.py [--sizes 1e5,1e6,1e7] [--ref-sizes 1e5,1e6] [--steps 5] [--warmup 1]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rayforce_amd import hostobj as H  # noqa: E402
from rayforce_amd import joins  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402
from bench_median import hwmon, timed  # noqa: E402

T_TIME = 8
NINE = 9 * 3_600_000  # 09:00:00 in milliseconds


def wj_tables(n):
    """examples/wj.rfl in numpy: symbols as 0 AAPL, 1 MSFT, 2 GOOG"""
    i, j = np.arange(n, dtype=np.int64), np.arange(2 * n, dtype=np.int64)
    trades = {"Sym": np.where(i % 100 < 99, 0, 1), "Ts": NINE + i * 3 // 10, "Price": 10 + i}
    quotes = {"Sym": np.select([j % 6 < 3, j % 6 < 5], [0, 1], 2), "Ts": NINE + j * 2 // 10, "Bid": 8 + j // 2, "Ask": 12 + j // 2}
    return trades, quotes, trades["Ts"] - 1000, trades["Ts"] + 1000


def reference_ms(trades, quotes, lo, hi, threads):
    """(window-join [Sym Ts] intervals trades quotes {bid: (min Bid) ask: (max Ask)}) inside the reference binary; None when it is not beside the tree"""
    from oracle import ref
    if not ref.available():
        return None
    with ref.Session() as s:
        s.eval("(set SY [AAPL MSFT GOOG])")
        for side, t in (("l", trades), ("r", quotes)):
            for k, v in t.items():
                s.put(f"{side}_{k}", v.astype(np.int32) if k == "Ts" else v, tp=T_TIME if k == "Ts" else None)
        s.put("w_lo", lo.astype(np.int32), tp=T_TIME)
        s.put("w_hi", hi.astype(np.int32), tp=T_TIME)
        s.eval("(set trades (table [Sym Ts Price] (list (at SY l_Sym) l_Ts l_Price)))")
        s.eval("(set quotes (table [Sym Ts Bid Ask] (list (at SY r_Sym) r_Ts r_Bid r_Ask)))")
        s.eval("(set intervals (list w_lo w_hi))")
        s.out("ms", "(enlist (timeit (window-join [Sym Ts] intervals trades quotes {bid: (min Bid) ask: (max Ask)})))")
        return float(s.run(threads=threads, timeout=1500.0)["ms"][0])


def typed_vector(ops, a, t):
    """a host vector of the reference's type t: 8 TIME (4-byte cells), 6 SYMBOL (8-byte ids)"""
    o = ops.rfx_host_vector(t, a.size)
    d = np.ascontiguousarray(a.astype(np.int32) if t == T_TIME else a.astype(np.int64))
    C.memmove(H.payload(o), d.ctypes.data, d.nbytes)
    return o


def tvec(ops, a):
    return typed_vector(ops, a, T_TIME)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e5,1e6,1e7")
    ap.add_argument("--ref-sizes", default="1e5,1e6", help="comma-separated sizes the reference runs too, or none")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    eng = Engine(0)
    ops = H.lib()
    ops.rfx_host_bind()
    clock = hwmon(eng.device.index)
    ref_sizes = set() if a.ref_sizes == "none" else {int(float(x)) for x in a.ref_sizes.split(",")}
    for n in (int(float(x)) for x in a.sizes.split(",")):
        trades, quotes, lo, hi = wj_tables(n)
        left = {k: eng.column(v) for k, v in trades.items()}
        right = {k: eng.column(v) for k, v in quotes.items()}
        win = (eng.column(lo), eng.column(hi))
        state = {}

        def ranges():
            state["r"] = joins.window_ranges(eng, ["Sym"], "Ts", win, left, right, False)

        def fold():
            perm, li, ri, nlong, _ = state["r"]
            state["bid"] = joins.window_fold(eng, right["Bid"], perm, li, ri, nlong, ["min"])["min"]
            state["ask"] = joins.window_fold(eng, right["Ask"], perm, li, ri, nlong, ["max"])["max"]

        ranges_ms, mhz = timed(ranges, a.steps, a.warmup, clock)
        fold_ms, fold_mhz = timed(fold, a.steps, a.warmup, clock)
        perm, li, ri, nlong, longest = state["r"]
        cells = int((ri - li + 1).clamp(min=0).sum())
        bid_sum, ask_sum = int(state["bid"].sum()), int(state["ask"].sum())
        del left, right, win, perm, li, ri
        state.clear()
        torch.cuda.empty_cache()
        # the door: host tables; the warm-up call leaves their columns resident
        sy = np.array([ops.rfx_host_intern(s.encode(), len(s)) for s in ("AAPL", "MSFT", "GOOG")], np.int64)
        tab = lambda t: ops.rfx_host_table(H.symbols(list(t)), H.list_of([tvec(ops, v) if k == "Ts" else typed_vector(ops, sy[v], H.T_SYMBOL) if k == "Sym" else H.vector(v) for k, v in t.items()]))
        lt, rt = tab(trades), tab(quotes)
        wins = H.list_of([tvec(ops, lo), tvec(ops, hi)])
        d = ops.rfx_host_dict(H.symbols(["bid", "ask"]), H.list_of([H.expr(("min", "Bid")), H.expr(("max", "Ask"))]))
        ks = H.symbols(["Sym", "Ts"])
        door = {}
        for name, fn in (("door_ms", ops.rfx_window_join), ("door1_ms", ops.rfx_window_join1)):
            def call():
                r = fn((C.c_void_p * 5)(ks, wins, lt, rt, d), 5)
                assert not H.is_error(r), H.error_text(r)
                assert ops.rfx_last_window_on_gpu() == 1
                if "cols" not in state:  # (the two new columns are the table's last)
                    cols = H.list_items(H.list_items(r)[1])
                    state["cols"] = {"bid": int(H.to_numpy(cols[-2]).sum()), "ask": int(H.to_numpy(cols[-1]).sum())}
                ops.rfx_host_drop(r)
            door[name], _ = timed(call, a.steps, a.warmup, None)
            if name == "door_ms":
                assert state["cols"] == {"bid": bid_sum, "ask": ask_sum}, (state["cols"], bid_sum, ask_sum)  # (the door and the planner answer alike)
            state.clear()
        for o in (lt, rt, wins, d, ks):
            ops.rfx_host_drop(o)
        ops.rfx_cache_clear()
        row = {"case": f"wj.rfl shape, {n} trades x {2 * n} quotes, min Bid + max Ask", "trades": n, "quotes": 2 * n, "ranges_ms": round(ranges_ms, 3),
               "fold_ms": round(fold_ms, 3), "door_ms": round(door["door_ms"], 3), "door1_ms": round(door["door1_ms"], 3), "window_cells": cells,
               "long_windows": nlong, "longest_window": longest, "fold_cells_per_us": round(2 * cells / (fold_ms * 1e3), 1), "fold_scheme": "direct (lane / wavefront)",
               "sclk_mhz": mhz, "fold_sclk_mhz": fold_mhz, "steps": a.steps}
        for th in (8, 1):
            if n in ref_sizes:
                print(f"reference window-join, {n} trades, {th} thread(s) ...", file=sys.stderr, flush=True)
                r = reference_ms(trades, quotes, lo, hi, th)
                row[f"ref_window_join_ms_threads{th}"] = round(r, 1) if r is not None else "not measured"
            else:
                row[f"ref_window_join_ms_threads{th}"] = "not measured"
        print(json.dumps(row), flush=True)
        eng.trim()
    eng.close()


if __name__ == "__main__":
    main()
