"""Timing of the device sort (rfx_sort.hip) through the planner (rfx_exec_sort) on device-resident columns: iasc of i64 keys in [0, 1e6), of full-range
i64 keys and of uniform f64 keys; xdesc's permutation of a 1e6-row result; a two-column xasc.  Per case: the median of --steps timed steps after --warmup
(a device synchronise inside the timed region), the passes executed, the bytes the traffic model counts (pre-pass 16 B per row -- the column read, the
keys written --, every executed pass 8 B per row for its count and 24 B per row for its scatter's reads and writes, the last one writing 8-byte rows)
and that over the time, and the shader clock (hwmon freq1_input, sampled every millisecond).  Two yardsticks in the same run, named for what they are:
`ref_iasc_ms` the compiled reference's own ray_iasc on this box's CPU (oracle/_ref/librayforce_ref.so, when present) at --ref-rows rows, and
`torch_sort_ms` torch.sort(stable=True) on the same device tensor (rocPRIM: for information, not in the product).  One JSON line per case.
--shards k[,k..]: instead, per shard count the sort over k shards of ONE device (rfx_exec_sort_shards: local radix sorts, one multiway merge,
rfx_merge.hip) beside the unsharded sort of the same column in the same process: the local-sort phase, the merge phase (the planner's own wall-clock
counters) and the total, and the merge's bytes -- (8 * keys + 8) read and 8 written per row -- over its time against the 8 TB/s roofline.  --tile T
runs the merge with another splitter tile (RFX_MERGE_TILE; 0 = the shipped one).  Beside the four cases, per shard count one whose runs interleave
record by record (row mod the shard span): every gap between splitters then holds a tile of every run -- the merge's worst case.

--narrow: instead, the packed-record path over keys of at most 32 bits: iasc of uniform full-range I32 keys (negatives included), of I32 keys in
[0, 1e6), of DATE keys with 10 % nulls, of I16 and of U8 keys.  Per arm, in one process and alternating step by step: the packed path over the raw
cells, for the I32 arms the 8-byte path over the same cells' widened image (rfx_hip_widen_i32 -- what the operator layer could have run with no new
kernel), and torch.sort(stable=True) of the same tensor.  Per path the median, the fastest and the slowest step, the passes, and the bytes of the
passes' traffic model (8 B count + 16 B scatter per row and pass for packed records; 8 + 24 for the 8-byte path) over the median against 8 TB/s.
--out FILE appends the JSON lines to FILE as well.

    python tools/bench_sort.py [--rows 100000000,1000000000] [--ref-rows 100000000] [--steps 5] [--warmup 1]
    python tools/bench_sort.py --rows 100000000 --shards 2,4,8 [--tile 2048]
    python tools/bench_sort.py --narrow --rows 100000000 --steps 7 --warmup 2 [--out profiles/sort_narrow_bench_run1.jsonl]
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


def sharded(a):
    if a.tile:
        os.environ["RFX_MERGE_TILE"] = str(a.tile)  # (read when a planner is created)
    eng = Engine(0)
    tile = a.tile or eng.lib.rfx_hip_merge_tile()
    g = torch.Generator(device=eng.device).manual_seed(1)
    for n in [int(x) for x in a.rows.split(",")]:
        narrow = torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=eng.device, generator=g)
        second = torch.randint(0, 1000, (n,), dtype=torch.int64, device=eng.device, generator=g)
        full = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=eng.device, generator=g)
        f = torch.rand(n, dtype=torch.float64, device=eng.device, generator=g)
        cases = [("iasc i64 [0,1e6)", [narrow]), ("iasc i64 full range", [full]), ("iasc f64 uniform", [f]), ("xasc by two columns ([0,1e3) then [0,1e6))", [second, narrow])]
        one = {}
        for case, cols in cases:
            one[case], _ = timed(lambda: eng.sort_index(cols), a.steps, a.warmup, None)
            print(json.dumps({"case": case, "rows": n, "shards": 1, "ms": round(one[case], 3), "steps": a.steps}), flush=True)
        for k in [int(x) for x in a.shards.split(",")]:
            es = Engine(0, shards=k)
            # the merge's worst case: every shard holds the same keys 0 .. span-1, so every gap between splitters holds a tile of EVERY run
            span = ((n + k - 1) // k + 511) & ~511
            inter = torch.arange(n, dtype=torch.int64, device=eng.device) % span
            name = "iasc i64 interleaved runs (row mod the shard span)"
            one[name], _ = timed(lambda: eng.sort_index([inter]), a.steps, a.warmup, None)
            for case, cols in cases + [(name, [inter])]:
                for _ in range(a.warmup):
                    es.sort_index(cols, over_shards=True)
                before = [es.xstat(s) for s in (L.RFX_XSTAT_NS_SORT_LOCAL, L.RFX_XSTAT_NS_SORT_MERGE)]
                ms, _ = timed(lambda: es.sort_index(cols, over_shards=True), a.steps, 0, None)
                local, merge = [(es.xstat(s) - b) / a.steps / 1e6 for s, b in zip((L.RFX_XSTAT_NS_SORT_LOCAL, L.RFX_XSTAT_NS_SORT_MERGE), before)]
                moved = n * (8 * len(cols) + 8 + 8)
                print(json.dumps({"case": case, "rows": n, "shards": k, "tile": tile, "ms": round(ms, 3), "local_sort_ms_mean": round(local, 3),
                                  "merge_ms_mean": round(merge, 3), "merge_model_gb": round(moved / 1e9, 2), "merge_tb_s": round(moved / merge / 1e9, 3),
                                  "merge_of_8tb_s_roofline": round(moved / merge / 1e9 / 8.0, 3), "one_shard_ms": round(one[case], 3),
                                  "over_one_shard": round(ms / one[case], 2), "steps": a.steps}), flush=True)
            es.close()
        del narrow, second, full, f
        torch.cuda.empty_cache()
    eng.close()


def narrow_arms(a):
    eng = Engine(0)
    g = torch.Generator(device=eng.device).manual_seed(1)
    i32min = -(1 << 31)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def passes_of(fn):
        before = eng.xstat(L.RFX_XSTAT_SORT_PASSES)
        fn()
        return eng.xstat(L.RFX_XSTAT_SORT_PASSES) - before

    for n in [int(x) for x in a.rows.split(",")]:
        arms = [("iasc i32 full range", lambda: torch.randint(i32min, 1 << 31, (n,), dtype=torch.int64, device=eng.device, generator=g).to(torch.int32), True),
                ("iasc i32 [0,1e6)", lambda: torch.randint(0, 1_000_000, (n,), dtype=torch.int32, device=eng.device, generator=g), True),
                ("iasc date, 10% nulls", lambda: torch.where(torch.rand(n, device=eng.device, generator=g) < 0.1, i32min,
                                                              torch.randint(0, 20_000, (n,), dtype=torch.int32, device=eng.device, generator=g)).to(torch.int32), True),
                ("iasc i16 full range", lambda: torch.randint(-(1 << 15), 1 << 15, (n,), dtype=torch.int16, device=eng.device, generator=g), False),
                ("iasc u8 full range", lambda: torch.randint(0, 256, (n,), dtype=torch.uint8, device=eng.device, generator=g), False)]
        for case, make, is_i32 in arms:
            col = make()
            paths = {"packed": lambda: eng.sort_index(col)}
            if is_i32:
                wide = torch.empty(n, dtype=torch.int64, device=eng.device)
                L.check(eng.lib.rfx_hip_widen_i32(eng._ctx, col.data_ptr(), n, wide.data_ptr()), "widen_i32")
                eng.sync()
                paths["wide8"] = lambda: eng.sort_index(wide)
            if not a.no_torch:
                paths["torch"] = lambda: torch.sort(col, stable=True)
            passes = {k: passes_of(f) for k, f in paths.items() if k != "torch"}
            for _ in range(a.warmup):
                for f in paths.values():
                    f()
            ts = {k: [] for k in paths}
            for _ in range(a.steps):  # alternating: every step times every path once
                for k, f in paths.items():
                    ts[k].append(once(f))
            row = {"case": case, "rows": n, "steps": a.steps, "warmup": a.warmup}
            for k, v in ts.items():
                v.sort()
                row[k + "_ms"], row[k + "_ms_min"], row[k + "_ms_max"] = round(v[len(v) // 2], 3), round(v[0], 3), round(v[-1], 3)
            for k, per_pass in (("packed", 24), ("wide8", 32)):
                if k in passes:
                    moved = n * per_pass * passes[k]
                    row[k + "_passes"], row[k + "_model_gb"] = passes[k], round(moved / 1e9, 2)
                    row[k + "_model_of_8tb_s"] = round(moved / row[k + "_ms"] / 1e9 / 8.0, 3)
            if "wide8" in ts:
                row["packed_over_wide8"] = round(row["packed_ms"] / row["wide8_ms"], 3)
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del col, paths
            if is_i32:
                del wide
            torch.cuda.empty_cache()
            eng.trim()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000000,1000000000")
    ap.add_argument("--ref-rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--shards", default="")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--narrow", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.narrow:
        return narrow_arms(a)
    if a.shards:
        return sharded(a)
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
