"""Timing of `med` on the device (rfx_median.hip): the scalar median of 1e9 i64 rows, and grouped medians by 6, 1e3 and 1e6 keys over 1e9 rows.  `med_ms`
is the KERNEL alone (rfx_hip_group_median; grouped: a prebuilt slot table of the dense keys 0..k-1, no group-by); `sum_ms` is a whole planner query
(Engine.select with the group-by) over the same device columns, for scale -- not the same work.  The median of --steps timed steps after --warmup, and the
shader clock the device ran at (hwmon freq1_input, sampled every millisecond during the timed median steps).  One JSON line per case.

    python tools/bench_median.py [--rows 1000000000] [--steps 10] [--warmup 2]
"""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayforce_amd import _lib as L  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402


def hwmon(device_index):
    props = torch.cuda.get_device_properties(device_index)
    want = f"{getattr(props, 'pci_domain_id', 0):04x}:{props.pci_bus_id:02x}:{getattr(props, 'pci_device_id', 0):02x}"
    for card in glob.glob("/sys/class/drm/card*/device"):
        if os.path.basename(os.path.realpath(card)).lower().startswith(want):
            hits = glob.glob(os.path.join(card, "hwmon", "hwmon*", "freq1_input"))
            if hits:
                return hits[0]
    return None


def timed(fn, steps, warmup, clock_file):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    freq, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            try:
                with open(clock_file) as f:
                    freq.append(int(f.read()) / 1e6)
            except (OSError, ValueError, TypeError):
                return
            time.sleep(0.001)
    th = threading.Thread(target=poll, daemon=True) if clock_file else None
    if th:
        th.start()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    stop.set()
    if th:
        th.join(timeout=1.0)
    ts.sort()
    fs = sorted(freq)
    return ts[len(ts) // 2], (round(fs[len(fs) // 2]) if fs else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keys", default="0,6,1000,1000000", help="0 = the scalar median")
    a = ap.parse_args()
    eng = Engine(0)
    lib, n = eng.lib, a.rows
    clock = hwmon(eng.device.index)
    g = torch.Generator(device=eng.device).manual_seed(1)
    v = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=eng.device, generator=g)
    out = torch.empty(1_000_000, dtype=torch.float64, device=eng.device)
    for keys in [int(x) for x in a.keys.split(",")]:
        rows = L.MedRows()
        keep = []
        if keys == 0:
            def med():
                L.check(lib.rfx_hip_group_median(eng._ctx, C.byref(rows), C.c_void_p(v.data_ptr()), L.RFX_I64, n, 1, L.RFX_MED_SCALAR, C.c_void_p(out.data_ptr())))
            sum_q = {"from": {"v": v}, "s": ("sum", "v")}
        else:
            k = torch.randint(0, keys, (n,), dtype=torch.int64, device=eng.device, generator=g)
            table = torch.arange(keys, dtype=torch.int64, device=eng.device)  # (dense keys 0..keys-1: slot = key)
            keep += [k, table]
            rows.d_key, rows.d_table, rows.kmin, rows.range = k.data_ptr(), table.data_ptr(), 0, keys

            def med():
                L.check(lib.rfx_hip_group_median(eng._ctx, C.byref(rows), C.c_void_p(v.data_ptr()), L.RFX_I64, n, keys, L.RFX_MED_GROUPED, C.c_void_p(out.data_ptr())))
            sum_q = {"from": {"v": v, "k": k}, "by": "k", "s": ("sum", "v")}
        t_med, mhz = timed(med, a.steps, a.warmup, clock)
        t_sum, _ = timed(lambda: eng.select(sum_q), a.steps, a.warmup, None)
        print(json.dumps({"case": "scalar med" if keys == 0 else f"med by {keys} keys", "rows": n, "med_ms": round(t_med, 3), "med_what": "kernel only", "sum_ms": round(t_sum, 3), "sum_what": "planner query",
                          "sclk_mhz": mhz, "steps": a.steps}), flush=True)
        del keep
    eng.close()


if __name__ == "__main__":
    main()
