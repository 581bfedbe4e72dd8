"""Timing of `as` over vectors (rfx_cast.hip) on one device, 1e8 rows by default.  One JSON line per case; every GPU case runs in a child process of its
own under its own time limit (`timeout -k 10`), and nothing more is started on the GPU after a child that did not end cleanly.

  arms       I64->F64, F64->I64, I64->I32, I32->I64, F64->U8.  Each through the Engine (the kernel and its launch alone: device tensors in and out; a timed
             step is `--reps` calls in a row, so that the window is milliseconds, not one launch) and through the door (rfx_as over a device-column
             handle -- the I32 source, which the door takes as a host vector only, over its resident widened copy -- with the result's read-back into a
             host vector included).  Reported as ms and as a fraction of the HBM roofline at the arm's bytes per row (source cell + result cell; 8 TB/s
             peak).  Beside each, in the same process and alternating with it: torch.Tensor.to(dtype) on the same tensor (for F64->U8 and the other
             out-of-range arms torch answers other cells: a yardstick for time only).
  floor      with the I64->F64 arm: Engine.floor of an F64 column, the same 16 B per row and the same kernel structure, two runs alternating with two
             runs of the cast: `cast_within_floor_spread` says whether the cast's time lies inside [min, max] of the floor runs widened by their spread.
  reference  the compiled reference's own (as 'T v) with 1 and 8 threads on this box's CPU (oracle/_ref/rayforce, when present: its own `timeit` around
             the verb, the column file's pages touched before).
Times are medians of --steps timed steps after --warmup, a device synchronise inside the timed region; the shader clock is hwmon freq1_input.

    python tools/bench_cast.py [--rows 100000000] [--steps 7] [--warmup 2] [--reps 10] [--case NAME]
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
# case -> (source type, target type) by the names Engine.cast takes; bytes per cell
ARMS = {"i64_f64": ("i64", "f64"), "f64_i64": ("f64", "i64"), "i64_i32": ("i64", "i32"), "i32_i64": ("i32", "i64"), "f64_u8": ("f64", "u8")}
BYTES = {"u8": 1, "i32": 4, "i64": 8, "f64": 8}
CODE = {"u8": 2, "i32": 4, "i64": 5, "f64": 10}
CASES = tuple(ARMS) + ("reference",)


def reference(rows):
    """(as 'T v) inside the compiled reference, every arm, 1 and 8 threads: wall time of the verb alone by the reference's own timer"""
    import numpy as np
    from oracle import ref
    row = {"case": "reference", "rows": rows}
    if not ref.available():
        row["ref_ms"] = "not measured"
        return row
    rng = np.random.default_rng(1)
    for th in (1, 8):
        with ref.Session() as s:
            s.put("i64", rng.integers(-(2**40), 2**40, rows))
            s.put("i32", rng.integers(-(2**31), 2**31, rows).astype(np.int32), tp=4)
            s.put("f64", (rng.random(rows) - 0.5) * 1e6)
            for name in ("i64", "i32", "f64"):
                s.eval(f"(set t_{name} (sum {name}))")  # (every page of the mapped column file is touched before the timed calls)
            for src, dst in ARMS.values():
                s.eval(f"(println (timeit (as '{dst.upper()} {src})))")
            out = ref.run_script("\n".join(s.lines) + "\n", threads=th, timeout=900)
        try:
            for case, ms in zip(ARMS, out.strip().splitlines()[-len(ARMS):]):
                row[f"ref_{case}_{th}t_ms"] = round(float(ms), 1)
        except ValueError:
            row[f"ref_{th}t_ms"] = "not measured"
    return row


def child(case, rows, steps, warmup, reps):
    if case == "reference":
        print(json.dumps(reference(rows)), flush=True)
        return
    import ctypes as C

    import torch
    from rayforce_amd import hostobj as H
    from rayforce_amd.engine import Engine
    from bench_median import hwmon, timed

    eng = Engine(0)
    clock = hwmon(eng.device.index)
    g = torch.Generator(device=eng.device).manual_seed(1)
    n = rows
    src, dst = ARMS[case]
    if src == "f64":
        col = (torch.rand(n, dtype=torch.float64, device=eng.device, generator=g) - 0.5) * 1e6
    elif src == "i32":
        col = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device=eng.device, generator=g).to(torch.int32)
    else:
        col = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=eng.device, generator=g)
    tdt = eng._CAST_DTYPE[CODE[dst]]
    per_row = BYTES[src] + BYTES[dst]

    def many(fn):
        def run():
            for _ in range(reps):
                fn()
        return run
    cast = many(lambda: eng.cast(col, dst, src))
    to = many(lambda: col.to(tdt))
    runs = {"cast": [], "torch_to": []}
    others = {"cast": cast, "torch_to": to}
    if case == "i64_f64":
        fcol = (torch.rand(n, dtype=torch.float64, device=eng.device, generator=g) - 0.5) * 1e6
        others["floor"] = many(lambda: eng.floor(fcol))
        runs["floor"] = []
    mhz = None
    for _ in range(2):  # they alternate inside one process: the same clocks, the same neighbours
        for name, fn in others.items():
            t, mhz = timed(fn, steps, warmup, clock)
            runs[name].append(round(t / reps, 4))
    k_ms = min(runs["cast"])
    row = {"case": case, "rows": n, "steps": steps, "reps": reps, "bytes_per_row": per_row, "cast_ms": k_ms, "hbm_frac": round(per_row * n / (k_ms * 1e-3) / HBM_PEAK, 4),
           "torch_to_ms": min(runs["torch_to"]), "runs_ms": runs, "sclk_mhz": mhz}
    if "floor" in runs:
        lo, hi = min(runs["floor"]), max(runs["floor"])
        row.update(floor_ms=lo, floor_spread_ms=round(hi - lo, 4), cast_within_floor_spread=bool(lo - (hi - lo) <= k_ms <= hi + (hi - lo)), cast_over_floor=round(k_ms / lo, 4))
    # the door: the read-back of the result into a fresh host vector included
    ops = H.lib()
    ops.rfx_host_bind()
    if src == "i32":
        host = col.cpu().numpy()
        x = ops.rfx_host_vector(4, n)
        C.memmove(H.payload(x), host.ctypes.data, host.nbytes)
        row["door_source"] = "host vector, resident after the first call"
    else:
        x = ops.rfx_host_device_vector(CODE[src], n, (C.c_void_p * 1)(col.data_ptr()), 1)
        row["door_source"] = "device-column handle"
    t_name = ops.rfx_host_symbol(dst.upper().encode())

    def door():
        r = ops.rfx_as(t_name, x)
        assert r and not H.is_error(r) and ops.rfx_last_cast_on_gpu() == 1
        ops.rfx_host_drop(r)
    d_ms, _ = timed(door, max(3, steps // 2), warmup, clock)
    row.update(door_ms=round(d_ms, 3), readback_gb_s=round(BYTES[dst] * n / ((d_ms - k_ms) * 1e-3) / 1e9, 2) if d_ms > k_ms else None)
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10, help="calls in a row inside one timed step of the device-tensor measurements")
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    a = ap.parse_args()
    if a.case:
        child(a.case, a.rows, a.steps, a.warmup, a.reps)
        return 0
    for case in CASES:
        t0 = time.time()
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--case", case, "--rows", str(a.rows), "--steps", str(a.steps),
                            "--warmup", str(a.warmup), "--reps", str(a.reps)], stdin=subprocess.DEVNULL)
        if p.returncode != 0:  # a fault, an abort, a time limit: nothing more is started on the GPU
            print(json.dumps({"case": case, "failed": p.returncode, "seconds": round(time.time() - t0, 1)}), flush=True)
            return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
