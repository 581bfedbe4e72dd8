"""Timing of row / collect (rfx_collect.hip) on one device.  One JSON line per case into profiles/collect_bench_run<N>.jsonl (and to stdout); every GPU case
runs in a child process of its own under its own time limit (`timeout -k 10`), and nothing more is started on the GPU after a child that did not end cleanly.
--steps timed steps after --warmup, the arms alternating step by step in one process, a device synchronise inside the timed region; medians.

  g<G>          --rows rows of an i64 key with G distinct values and four 8-byte value columns.  Arms: `collect1` / `collect4` (Engine.group_collect of one /
                four columns: the planner's group-by for the keys, the join index for every row's group, the partition, the gather), `partition` (Engine.partition
                over the per-row ids made beforehand: the packed sort and the offsets), `torch1` / `torch4` (the outside yardstick on the same tensors:
                torch.sort(stable=True) of the ids, torch.bincount, index_select per column).  The gather kernel alone (rfx_hip_group_collect over a finished
                permutation, one and four columns) is timed by HIP events; `gather*_fraction_of_hbm_peak`: (8 B of permutation per row + 2 x 8 B per row and
                column) over its time over 8 TB/s.  `partition_passes`: the radix passes the partition ran.
  door_g<G>     through the door on host objects at --door-rows rows: rfx_select {p: v by: k} with its read-back and the host's cutting of G vectors, against
                Engine.group_collect of the same column in the same process (the device part alone, result left on the device): the difference is the
                read-back and the list assembly.
  reference     the compiled reference's own select {p: v by: k} with 1 and 8 threads (oracle/_ref/rayforce, when present) at --ref-rows rows, G = 1000; a run
                that takes longer than a minute is "not measured".

    python tools/bench_collect.py [--rows 100000000] [--steps 7] [--warmup 2] [--run 1] [--case NAME]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12
GROUPS = (6, 1000, 1_000_000)
CASES = tuple(f"g{g}" for g in GROUPS) + tuple(f"door_g{g}" for g in GROUPS) + ("reference",)


def device_case(case, a):
    import torch
    from rayforce_amd import _lib as L
    from rayforce_amd.engine import Engine
    eng = Engine(0)
    dev = eng.device
    groups, n = int(case[1:]), a.rows
    gen = torch.Generator(device=dev).manual_seed(5)
    key = torch.randint(0, groups, (n,), device=dev, generator=gen) * 3 + 11
    cols = {f"v{i}": (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) if i % 2 else torch.randint(0, 1 << 40, (n,), device=dev, generator=gen)) for i in range(4)}
    one = {"v0": cols["v0"]}

    def torch_arm(cs):
        gid = (key - 11) // 3  # (the ids come straight off the key: the composition is spared the grouping the collect arms pay for)
        _, perm = torch.sort(gid, stable=True)
        counts = torch.bincount(gid, minlength=groups)
        return counts, [torch.index_select(c, 0, perm) for c in cs.values()]

    # correctness once: every group's cells as the torch composition leaves them (group ORDER differs: first occurrence here, ascending id there)
    keys, offsets, cells = eng.group_collect(key, cols)
    counts, want = torch_arm(cols)
    order = torch.argsort(keys)
    assert torch.equal((offsets[1:] - offsets[:-1])[order], counts[counts > 0]), "group sizes differ from the torch composition"
    g0 = int(order[0])
    lo, hi = int(offsets[g0]), int(offsets[g0 + 1])
    assert all(torch.equal(cells[c][lo:hi].view(torch.int64), want[i][: hi - lo].view(torch.int64)) for i, c in enumerate(cols)), "cells differ from the torch composition"
    ngroups = keys.numel()
    del keys, offsets, cells, counts, want
    gid = (key - 11) // 3
    forms = {"collect1": lambda: eng.group_collect(key, one), "collect4": lambda: eng.group_collect(key, cols), "partition": lambda: eng.partition(gid, groups),
             "torch1": lambda: torch_arm(one), "torch4": lambda: torch_arm(cols)}
    ms = {k: [] for k in forms}
    p0 = eng.xstat(L.RFX_XSTAT_COLLECT_PASSES)
    eng.partition(gid, groups)
    passes = eng.xstat(L.RFX_XSTAT_COLLECT_PASSES) - p0
    for step in range(a.warmup + a.steps):
        for name, f in forms.items():
            eng.sync()
            t0 = time.perf_counter()
            r = f()
            eng.sync()
            if step >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            del r
    # the gather kernel alone, by HIP events, over one finished permutation
    offsets, perm = eng.partition(gid, groups)
    outs = [eng.empty(n, c.dtype) for c in cols.values()]
    cc = (L.CollectCol * 4)()
    for i, c in enumerate(cols.values()):
        cc[i].d_col, cc[i].d_out, cc[i].width = c.data_ptr(), outs[i].data_ptr(), 8
    gms = {1: [], 4: []}
    for step in range(a.warmup + a.steps):
        for nc in (1, 4):
            eng.sync()
            eng.timer_start()
            L.check(eng.lib.rfx_hip_group_collect(eng._ctx, cc, nc, perm.data_ptr(), None, n, n), "collect")
            v = eng.timer_stop()
            if step >= a.warmup:
                gms[nc].append(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    gmed = {k: statistics.median(v) for k, v in gms.items()}
    row = {"case": case, "rows": n, "groups": ngroups, "partition_passes": passes, "ms": {k: round(v, 4) for k, v in med.items()},
           "steps_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "gather_ms": {str(k): round(v, 4) for k, v in gmed.items()}}
    for nc in (1, 4):
        model = n * 8 + nc * n * 16
        row[f"gather{nc}_model_bytes"] = model
        row[f"gather{nc}_fraction_of_hbm_peak"] = round(model / (gmed[nc] * 1e-3) / HBM_PEAK, 5)
    eng.close()
    return row


def door_case(case, a):
    import numpy as np
    import torch
    from rayforce_amd import hostobj as H
    from rayforce_amd.engine import Engine
    ops = H.lib()
    ops.rfx_host_bind()
    groups, n = int(case[6:]), a.door_rows
    rng = np.random.default_rng(3)
    k, v = rng.integers(0, groups, n) * 3 + 11, rng.integers(0, 1 << 40, n)
    t = H.table(dict(k=k, v=v))
    d = H.select_dict(dict(p="v", by="k"), t)
    eng = Engine(0)
    dk, dv = torch.from_numpy(k).to(eng.device), torch.from_numpy(v).to(eng.device)
    sel_ms, dev_ms = [], []
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        r = ops.rfx_select(d)
        t1 = time.perf_counter()
        assert not H.is_error(r) and ops.rfx_last_select_on_gpu() == 1, ops.rfx_ops_last_error().decode()
        ops.rfx_host_drop(r)
        eng.sync()
        t2 = time.perf_counter()
        out = eng.group_collect(dk, {"v": dv})
        eng.sync()
        t3 = time.perf_counter()
        del out
        if step >= a.warmup:
            sel_ms.append((t1 - t0) * 1e3)
            dev_ms.append((t3 - t2) * 1e3)
    sel, devp = statistics.median(sel_ms), statistics.median(dev_ms)
    eng.close()
    return {"case": case, "rows": n, "groups": groups, "select_ms": round(sel, 4), "device_part_ms": round(devp, 4), "read_back_and_lists_ms": round(sel - devp, 4),
            "select_steps_ms": [round(x, 4) for x in sel_ms]}


def reference(a):
    import numpy as np
    from oracle import ref
    row = {"case": "reference", "rows": a.ref_rows, "groups": 1000}
    if not ref.available():
        row["ref_ms"] = "not measured"
        return row
    rng = np.random.default_rng(1)
    n = a.ref_rows
    for th in (1, 8):
        with ref.Session() as s:
            s.put("k", rng.integers(0, 1000, n) * 3 + 11)
            s.put("v", rng.integers(0, 1 << 40, n))
            s.eval("(set t (table [k v] (list k v)))")
            s.eval("(set t_k (sum k))")  # (every page of the mapped column files is touched before the timed call)
            s.eval("(set t_v (sum v))")
            s.eval("(println (timeit (select {p: v by: k from: t})))")
            try:
                out = ref.run_script("\n".join(s.lines) + "\n", threads=th, timeout=60)
                row[f"ref_select_{th}t_ms"] = round(float(out.strip().splitlines()[-1]), 2)
            except (ValueError, RuntimeError, subprocess.TimeoutExpired):
                row[f"ref_select_{th}t_ms"] = "not measured"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--door-rows", type=int, default=10_000_000)
    ap.add_argument("--ref-rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", type=int, default=1)
    ap.add_argument("--case", default=None)
    ap.add_argument("--only", default=None, help="comma-separated cases to run instead of all")
    a = ap.parse_args()
    if a.case:
        row = reference(a) if a.case == "reference" else (door_case(a.case, a) if a.case.startswith("door") else device_case(a.case, a))
        print(json.dumps(row), flush=True)
        return
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"collect_bench_run{a.run}.jsonl")
    with open(path, "w") as f:
        for case in (a.only.split(",") if a.only else CASES):
            cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", case] + [x for k in ("rows", "door_rows", "ref_rows", "steps", "warmup")
                                                                                                             for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                line = json.dumps({"case": case, "failed": p.returncode, "stderr": p.stderr[-800:]})
                f.write(line + "\n")
                print(line, flush=True)
                if case != "reference":
                    sys.exit(1)  # (nothing more on the GPU after a child that did not end cleanly)
                continue
            line = p.stdout.strip().splitlines()[-1]
            f.write(line + "\n")
            f.flush()
            print(line, flush=True)


if __name__ == "__main__":
    main()
