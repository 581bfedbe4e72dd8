"""A/B of the fused scalar fold (k_filter_aggr, rfx_scalar_kernel.hpp): the median time of Engine.filter_aggr over 1e8 rows for one plan per
instantiation family whose register count or scratch an edit of the fold can move -- the template arguments <NC, NA, U, NP, NX, DEEP> each plan lands
in are part of its name.  Run it from the ROOT of a tree: that tree's library answers, so two trees on one box, alternating, give the A/B
(docs/ledger_r07.md holds such a run).  RFX_NO_RTC=1 keeps every plan on the prebuilt kernels.  One JSON line: plan -> median ms of --steps steps.

    cd <tree> && RFX_NO_RTC=1 python <path>/tools/bench_fold.py [--rows 100000000] [--steps 15] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())
from rayforce_amd.engine import Engine  # noqa: E402

X = [("*", "v", "w"), ("+", "v", "w"), ("-", "v", "w"), ("*", "v", ("-", 1.0, "w"))]
FIVE_PREDS = ("and", (">", "v", 0.1), ("<", "v", 0.9), (">", "w", 0.1), ("<", "w", 0.9), ("!=", "v", 0.5))
DEEP3 = ("*", ("*", "v", ("-", 1.0, "w")), ("+", 1.0, "u"))
PLANS = {
    "1col 1 deep expr <1,8,4,8,4,true>": ([("sum", ("*", ("*", "v", ("-", 1.0, "v")), ("+", 1.0, "v")))], None),
    "2col 4 exprs <2,4,4,4,4>": ([("sum", X[0]), ("sum", X[1]), ("sum", X[2]), ("max", X[3])], None),
    "2col 4 exprs 5 preds <2,8,4,8,4>": ([("sum", X[0]), ("sum", X[1]), ("sum", X[2]), ("max", X[3])], FIVE_PREDS),
    "3col 5 aggs <3,8,4,8,0>": ([("sum", "v"), ("min", "w"), ("max", "u"), ("avg", "v"), ("first", "w")], None),
    "3col 5 aggs 2 exprs <3,8,4,8,4>": ([("sum", "v"), ("min", "w"), ("max", "u"), ("sum", X[0]), ("sum", ("*", "u", "w"))], None),
    "3col 5 aggs deep expr <3,8,4,8,4,true>": ([("sum", "v"), ("min", "w"), ("max", "u"), ("sum", DEEP3), ("count", "v")], None),
    "1col 5 aggs <1,8,4,8,0>": ([("sum", "v"), ("min", "v"), ("max", "v"), ("avg", "v"), ("first", "v")], None),
    "2col 1 expr (Q6 shape) <2,1,4,4,1>": ([("sum", X[0])], ("and", (">", "v", 0.1), ("<", "w", 0.9))),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    eng = Engine(0)
    gen = torch.Generator(device=eng.device).manual_seed(3)
    t = {c: torch.rand(a.rows, dtype=torch.float64, device=eng.device, generator=gen) for c in ("v", "w", "u")}
    out = {}
    for name, (aggs, where) in PLANS.items():
        for _ in range(a.warmup):
            eng.filter_aggr(aggs, where, t)
        ts = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.filter_aggr(aggs, where, t)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out[name] = round(ts[len(ts) // 2], 3)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
