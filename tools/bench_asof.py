"""Timing of the device asof join (rfx_asof.hip through rfx_exec_asof_index) and of bin on device-resident columns: trades x quotes with the
quotes' times ascending (the realistic shape) and shuffled, by 1e3 and 1e6 symbols; bin of --bin-rows queries into as many cells.  Per case: the
median of --steps timed steps after --warmup (a device synchronise inside the timed region) of the join index alone -- with its split into BUILD
(right side only: the groups, their stable order, the run boundaries, the times in group order) and PROBE (the left rows' groups and the searches),
from the planner's own RFX_XSTAT_NS_ASOF_* counters, averaged over the timed steps -- and of the whole Engine.asof_join (the index + one right-only column gathered); the searches'
dependent loads (left rows x ceil(log2(mean group length + 1))) over the probe time; the shader clock (hwmon freq1_input, sampled every
millisecond).  The yardstick, named for what it is: `ref_asof_join_ms_threads8` / `_threads1`, the compiled reference's own
`(asof-join [s t] trades quotes)` on this box's CPU (oracle/_ref/rayforce -c 8 / -c 1, its own `timeit`, column files loaded outside the timed
expression), for the cases named by --ref-cases.  One JSON line per case.

    python tools/bench_asof.py [--cases 1e7x1e8,1e8x1e8] [--symbols 1000,1000000] [--ref-cases 1e7x1e8:1000:sorted] [--steps 5] [--warmup 1]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rayforce_amd import _lib as L  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402
from bench_median import hwmon, timed  # noqa: E402

DAY_NS = 86_400_000_000_000


def reference_ms(left, right, threads):
    """(asof-join [s t] trades quotes) inside the reference binary; None when it is not beside the tree"""
    from oracle import ref
    if not ref.available():
        return None
    with ref.Session() as s:
        for k, v in left.items():
            s.put("l_" + k, v.cpu().numpy())
        for k, v in right.items():
            s.put("r_" + k, v.cpu().numpy())
        s.eval(f"(set trades (table [{' '.join(left)}] (list {' '.join('l_' + k for k in left)})))")
        s.eval(f"(set quotes (table [{' '.join(right)}] (list {' '.join('r_' + k for k in right)})))")
        s.out("ms", "(enlist (timeit (asof-join [s t] trades quotes)))")
        return float(s.run(threads=threads, timeout=1500.0)["ms"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1e7x1e8,1e8x1e8")
    ap.add_argument("--symbols", default="1000,1000000")
    ap.add_argument("--ref-cases", default="1e7x1e8:1000:sorted", help="comma-separated case:symbols:order, or none")
    ap.add_argument("--bin-rows", type=float, default=1e8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    eng = Engine(0)
    clock = hwmon(eng.device.index)
    g = torch.Generator(device=eng.device).manual_seed(1)
    ref_cases = set() if a.ref_cases == "none" else set(a.ref_cases.split(","))
    stat = lambda: [eng.xstat(s) for s in (L.RFX_XSTAT_ASOF_JOINS, L.RFX_XSTAT_NS_ASOF_BUILD, L.RFX_XSTAT_NS_ASOF_PROBE)]
    for case in a.cases.split(","):
        nl, nr = (int(float(x)) for x in case.split("x"))
        for nsym in (int(x) for x in a.symbols.split(",")):
            for order in ("sorted", "shuffled"):
                left = {"s": torch.randint(0, nsym, (nl,), dtype=torch.int64, device=eng.device, generator=g),
                        "t": torch.randint(0, DAY_NS, (nl,), dtype=torch.int64, device=eng.device, generator=g)}
                rt = torch.randint(0, DAY_NS, (nr,), dtype=torch.int64, device=eng.device, generator=g)
                right = {"s": torch.randint(0, nsym, (nr,), dtype=torch.int64, device=eng.device, generator=g),
                         "t": torch.sort(rt).values if order == "sorted" else rt,
                         "bid": torch.rand(nr, dtype=torch.float64, device=eng.device, generator=g)}
                del rt
                for _ in range(a.warmup):
                    eng.asof_index(["s"], "t", left, right)
                before = stat()
                ms, mhz = timed(lambda: eng.asof_index(["s"], "t", left, right), a.steps, 0, clock)
                after = stat()
                calls = after[0] - before[0]
                build, probe = (after[1] - before[1]) / calls / 1e6, (after[2] - before[2]) / calls / 1e6  # (means over the timed steps)
                join_ms, _ = timed(lambda: eng.asof_join(["s", "t"], left, right), a.steps, a.warmup, None)
                ids = eng.asof_index(["s"], "t", left, right)
                matched = int((ids != torch.iinfo(torch.int64).min).sum())
                del ids
                loads = nl * math.ceil(math.log2(nr / min(nsym, nr) + 1))
                row = {"case": f"asof {case} rows, {nsym} symbols, quotes {order}", "left_rows": nl, "right_rows": nr, "index_ms": round(ms, 3),
                       "build_ms": round(build, 3), "probe_ms": round(probe, 3), "join_ms": round(join_ms, 3), "matched": matched,
                       "dependent_loads": loads, "loads_per_us": round(loads / (probe * 1e3), 1), "sclk_mhz": mhz, "steps": a.steps}
                if f"{case}:{nsym}:{order}" in ref_cases:
                    for th in (8, 1):
                        print(f"reference asof-join, {th} thread(s) ...", file=sys.stderr, flush=True)
                        r = reference_ms(left, right, th)
                        row[f"ref_asof_join_ms_threads{th}"] = round(r, 1) if r is not None else "not measured"
                print(json.dumps(row), flush=True)
                del left, right
                torch.cuda.empty_cache()
                eng.trim()
    n = int(a.bin_rows)
    if n > 0:
        x = torch.sort(torch.randint(0, DAY_NS, (n,), dtype=torch.int64, device=eng.device, generator=g)).values
        y = torch.randint(0, DAY_NS, (n,), dtype=torch.int64, device=eng.device, generator=g)
        for verb, fn in (("bin", eng.bin), ("binr", eng.binr)):
            ms, mhz = timed(lambda: fn(x, y), a.steps, a.warmup, clock)
            loads = n * math.ceil(math.log2(n + 1))
            print(json.dumps({"case": f"{verb} of {n} queries into {n} sorted cells", "ms": round(ms, 3), "dependent_loads": loads,
                              "loads_per_us": round(loads / (ms * 1e3), 1), "sclk_mhz": mhz, "steps": a.steps}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
