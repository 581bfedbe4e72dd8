"""Timing of the bucket verbs (rfx_bucket.hip) on one device, 1e8 rows by default.  One JSON line per case; every GPU case runs in a child process of its
own under its own time limit (`timeout -k 10`), and nothing more is started on the GPU after a child that did not end cleanly.

  xrank      Engine.xrank of I64 keys in [0, 1e6) and of full-range I64 keys beside rfx_rank's device work on the same keys in the same run (the sort by
             Engine.sort_index + rfx_hip_inverse_perm: the fused scatter moves the same bytes, so `xrank_over_rank` near 1 is the expectation), and beside
             the compiled reference's own (xrank v 10) with 1 and 8 threads on this box's CPU (oracle/_ref/rayforce, when present: its own `timeit`
             around the verb, the key file's pages touched before).
  xbar       a TIMESTAMP column by an I64 atom; floor of an F64 column: through the Engine (the kernel and its launch alone: device tensors in and out) and
             through the door (rfx_xbar / rfx_floor over a device-column handle: the result's read-back into a host vector included).  Reported as a
             fraction of the HBM roofline at 16 B per row (8 read + 8 written; 8 TB/s peak) and as the share of the door's time that the PCIe read-back
             is (door - kernel) / door.
Times are medians of --steps timed steps after --warmup, a device synchronise inside the timed region; the shader clock is hwmon freq1_input.

    python tools/bench_bucket.py [--rows 100000000] [--steps 5] [--warmup 2] [--case NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
CASES = ("xrank_narrow", "xrank_full", "xbar_ts", "floor_f64")


def reference_xrank_ms(keys, threads):
    """(xrank v 10) inside the compiled reference: wall time of the verb alone, by the reference's own timer around it (None: not beside the tree)"""
    from oracle import ref
    if not ref.available():
        return None
    with ref.Session() as s:
        s.put("v", keys)
        s.eval("(set t0 (sum v))")  # (every page of the mapped key file is touched before the timed call)
        s.eval("(println (timeit (xrank v 10)))")
        out = ref.run_script("\n".join(s.lines) + "\n", threads=threads, timeout=900)
    try:
        return float(out.strip().splitlines()[-1])
    except (ValueError, IndexError):
        return None


def child(case, rows, steps, warmup):
    import torch
    from rayforce_amd import _lib as L
    from rayforce_amd import hostobj as H
    from rayforce_amd.engine import Engine
    from bench_median import hwmon, timed

    eng = Engine(0)
    clock = hwmon(eng.device.index)
    g = torch.Generator(device=eng.device).manual_seed(1)
    n = rows
    row = {"case": case, "rows": n, "steps": steps}
    if case.startswith("xrank"):
        keys = (torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=eng.device, generator=g) if case == "xrank_narrow"
                else torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device=eng.device, generator=g))
        inv = torch.empty_like(keys)

        def rank():
            perm = eng.sort_index(keys)
            L.check(eng.lib.rfx_hip_inverse_perm(eng._ctx, perm.data_ptr(), n, inv.data_ptr()), "inverse_perm")
        # the two alternate inside one process: the same clocks, the same neighbours
        xr, rk = [], []
        for _ in range(2):
            t, mhz = timed(lambda: eng.xrank(keys, 10), steps, warmup, clock)
            xr.append(t)
            t, _ = timed(rank, steps, warmup, clock)
            rk.append(t)
        row.update(xrank_ms=round(min(xr), 3), rank_ms=round(min(rk), 3), xrank_over_rank=round(min(xr) / min(rk), 4), both_runs_ms={"xrank": xr, "rank": rk}, sclk_mhz=mhz)
        host = keys.cpu().numpy()
        del keys, inv
        for th in (1, 8):
            r = reference_xrank_ms(host, th)
            row[f"ref_xrank_{th}t_ms"] = round(r, 1) if r is not None else "not measured"
    else:
        ops = H.lib()
        ops.rfx_host_bind()
        if case == "xbar_ts":
            col = torch.randint(0, 10**15, (n,), dtype=torch.int64, device=eng.device, generator=g)
            kernel = lambda: eng.xbar(col, 5000, "timestamp", "i64")  # noqa: E731
            x = ops.rfx_host_device_vector(9, n, (__import__("ctypes").c_void_p * 1)(col.data_ptr()), 1)
            w = ops.rfx_host_i64(5000)
            door_call = lambda: ops.rfx_xbar(x, w)  # noqa: E731
        else:
            col = (torch.rand(n, dtype=torch.float64, device=eng.device, generator=g) - 0.5) * 1e6
            kernel = lambda: eng.floor(col)  # noqa: E731
            x = H.device_vector(col)
            door_call = lambda: ops.rfx_floor(x)  # noqa: E731

        def door():
            r = door_call()
            assert r and not H.is_error(r) and ops.rfx_last_bucket_on_gpu() == 1
            ops.rfx_host_drop(r)
        k_ms, mhz = timed(kernel, steps, warmup, clock)
        d_ms, _ = timed(door, steps, warmup, clock)
        row.update(kernel_ms=round(k_ms, 3), hbm_frac_16B_per_row=round(16.0 * n / (k_ms * 1e-3) / HBM_PEAK, 4), door_ms=round(d_ms, 3),
                   pcie_share_of_door=round(max(0.0, d_ms - k_ms) / d_ms, 4), readback_gb_s=round(8.0 * n / ((d_ms - k_ms) * 1e-3) / 1e9, 2) if d_ms > k_ms else None,
                   sclk_mhz=mhz)
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    a = ap.parse_args()
    if a.case:
        child(a.case, a.rows, a.steps, a.warmup)
        return 0
    for case in CASES:
        t0 = time.time()
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case, "--rows", str(a.rows), "--steps", str(a.steps),
                            "--warmup", str(a.warmup)], stdin=subprocess.DEVNULL)
        if p.returncode != 0:  # a fault, an abort, a time limit: nothing more is started on the GPU
            print(json.dumps({"case": case, "failed": p.returncode, "seconds": round(time.time() - t0, 1)}), flush=True)
            return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
