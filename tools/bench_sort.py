"""Timing of the device sort (rfx_sort.hip) through the planner (rfx_exec_sort) on device-resident columns: iasc of i64 keys in [0, 1e6), of full-range
i64 keys and of uniform f64 keys; xdesc's permutation of a 1e6-row result; a two-column xasc.  Per case: the median of --steps timed steps after --warmup
(a device synchronise inside the timed region), the passes executed, the bytes the traffic model counts (pre-pass 16 B per row -- the column read, the
keys written --, every executed pass 8 B per row for its count and 24 B per row for its scatter's reads and writes, the last one writing 8-byte rows)
and that over the time, and the shader clock (hwmon freq1_input, sampled every millisecond).  Two yardsticks in the same run, named for what they are:
`ref_iasc_ms` the compiled reference's own ray_iasc on this box's CPU (oracle/_ref/librayforce_ref.so, when present) at --ref-rows rows, and
`torch_sort_ms` torch.sort(stable=True) on the same device tensor (rocPRIM: for information, not in the product).  One JSON line per case.

    python tools/bench_sort.py [--rows 100000000,1000000000] [--ref-rows 100000000] [--steps 5] [--warmup 1]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rayforce_amd import _lib as L  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402
from bench_median import hwmon, timed  # noqa: E402


def reference_iasc_ms(host_i64):
    """ray_iasc of the compiled reference on the CPU (None when the reference library is not beside the tree)"""
    path = os.path.join(ROOT, "oracle", "_ref", "librayforce_ref.so")
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    lib.ray_init.restype = C.c_int32
    if lib.ray_init() != 0:
        return None
    lib.vector.restype = C.c_void_p
    lib.vector.argtypes = [C.c_int8, C.c_int64]
    lib.ray_iasc.restype = C.c_void_p
    lib.ray_iasc.argtypes = [C.c_void_p]
    lib.drop_obj.argtypes = [C.c_void_p]
    x = lib.vector(5, host_i64.size)
    C.memmove(x + 16, host_i64.ctypes.data, host_i64.nbytes)
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        r = lib.ray_iasc(x)
        dt = (time.perf_counter() - t0) * 1e3
        lib.drop_obj(r)
        best = dt if best is None else min(best, dt)
    lib.drop_obj(x)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000000,1000000000")
    ap.add_argument("--ref-rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    eng = Engine(0)
    clock = hwmon(eng.device.index)
    g = torch.Generator(device=eng.device).manual_seed(1)

    def run(case, cols, n, descending=False, yardsticks=False):
        before = eng.xstat(L.RFX_XSTAT_SORT_PASSES), eng.xstat(L.RFX_XSTAT_SORTS)
        ms, mhz = timed(lambda: eng.sort_index(cols, descending=descending), a.steps, a.warmup, clock)
        calls = max(1, (eng.xstat(L.RFX_XSTAT_SORTS) - before[1]) // len(cols))
        passes = (eng.xstat(L.RFX_XSTAT_SORT_PASSES) - before[0]) // calls
        moved = n * (16 * len(cols) + 32 * passes + 4 * len(cols))
        row = {"case": case, "rows": n, "ms": round(ms, 3), "passes": passes, "model_gb": round(moved / 1e9, 2), "model_tb_s": round(moved / ms / 1e9, 3),
               "sclk_mhz": mhz, "steps": a.steps}
        if yardsticks and not a.no_torch and len(cols) == 1:
            t, _ = timed(lambda: torch.sort(cols[0], stable=True, descending=descending), a.steps, a.warmup, None)
            row["torch_sort_ms"] = round(t, 3)
        if yardsticks and n == a.ref_rows and cols[0].dtype == torch.int64:
            r = reference_iasc_ms(cols[0].cpu().numpy())
            row["ref_iasc_ms"] = round(r, 1) if r is not None else "not measured"
        print(json.dumps(row), flush=True)

    for n in [int(x) for x in a.rows.split(",")]:
        narrow = torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=eng.device, generator=g)
        run("iasc i64 [0,1e6)", [narrow], n, yardsticks=True)
        if n <= 200_000_000:
            second = torch.randint(0, 1000, (n,), dtype=torch.int64, device=eng.device, generator=g)
            run("xasc by two columns ([0,1e3) then [0,1e6))", [second, narrow], n)
            del second
        del narrow
        full = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=eng.device, generator=g)
        run("iasc i64 full range", [full], n, yardsticks=True)
        del full
        f = torch.rand(n, dtype=torch.float64, device=eng.device, generator=g)
        run("iasc f64 uniform", [f], n, yardsticks=True)
        del f
        torch.cuda.empty_cache()
        eng.trim()
    sums = torch.randint(-(1 << 40), 1 << 40, (1_000_000,), dtype=torch.int64, device=eng.device, generator=g)
    run("xdesc of a 1e6-row result by its sum", [sums], 1_000_000, descending=True)
    eng.close()


if __name__ == "__main__":
    main()
