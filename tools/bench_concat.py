"""Timing of concat and raze (rfx_concat.hip) on one device.  One JSON line per case into profiles/concat_bench_run<N>.jsonl (and to stdout); every
GPU case runs in a child process of its own under its own time limit (`timeout -k 10`), and nothing more is started on the GPU after a child that did
not end cleanly.  --steps timed steps after --warmup, the alternatives alternating step by step in one process, a device synchronise inside the timed
region; medians.

  table    (a) a 4-column I64 / F64 table of --rows rows plus a batch of rows / 100 on device tensors: the multi-span kernel (Engine.concat: one launch for
           the four columns), one device-to-device copy per span (rfx_hip_d2d, hipMemcpyAsync: 8 copies), torch.cat per column.
  raze_*   (b) raze of 1000 spans of rows / 1000 cells and of 16 spans of rows / 16 cells, 8-byte and 1-byte cells: the same three.
  ingest   (c) through the door: (concat t batch), then select {s: (sum v) by: k} with --keys keys over the answer, adoption on and off (RFX_CONCAT_ADOPT):
           the time of the select after the append and its uploads.  --ingest-rows rows (the append reads its answer back into host vectors).
  reference  the compiled reference's own concat of the table and raze of the spans with 1 and 8 threads (oracle/_ref/rayforce, when present).
`kernel_fraction_of_hbm_peak` is 2 x the cells' bytes (read once, written once) over the kernel form's time over 8 TB/s.

    python tools/bench_concat.py [--rows 100000000] [--steps 7] [--warmup 2] [--run 1] [--case NAME]
"""
import argparse
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
CASES = ("table", "raze_1000x8", "raze_16x8", "raze_1000x1", "raze_16x1", "ingest_adopt", "ingest_no_adopt", "reference")


def timed(eng, forms, steps, warmup):
    """forms: name -> callable; -> name -> median ms, the forms alternating step by step"""
    ms = {k: [] for k in forms}
    for step in range(warmup + steps):
        for name, f in forms.items():
            eng.sync()
            t0 = time.perf_counter()
            f()
            eng.sync()
            if step >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


def device_case(case, a):
    import torch
    from rayforce_amd.engine import Engine
    eng = Engine(0)
    dev = eng.device
    if case == "table":
        n, nb = a.rows, max(1, a.rows // 100)
        mk = lambda rows: {"k": torch.randint(0, 1 << 40, (rows,), device=dev), "t": torch.arange(rows, device=dev), "p": torch.rand(rows, dtype=torch.float64, device=dev),  # noqa: E731
                           "q": torch.rand(rows, dtype=torch.float64, device=dev)}
        t, b = mk(n), mk(nb)
        lists = [[t[c], b[c]] for c in t]
        cells_bytes = 4 * 8 * (n + nb)
    else:
        ns, w = case[5:].split("x")
        ns, dt = int(ns), (torch.int64 if w == "8" else torch.int8)
        per = a.rows // ns
        src = (torch.arange(a.rows + 64, device=dev) % 251).to(dt)
        lists = [[src[1 + i * per: 1 + (i + 1) * per] for i in range(ns)]]  # (from the second cell: sources that are cell-aligned only)
        cells_bytes = per * ns * int(w)
    outs = [torch.empty(sum(p.numel() for p in parts), dtype=parts[0].dtype, device=dev) for parts in lists]

    def kernel():
        return eng._concat_cols(lists)

    def copies():
        for parts, out in zip(lists, outs):
            at = 0
            for p in parts:
                eng.lib.rfx_hip_d2d(eng._ctx, out.data_ptr() + at, p.data_ptr(), p.numel() * p.element_size())
                at += p.numel() * p.element_size()

    def cat():
        return [torch.cat(parts) for parts in lists]

    got = kernel()
    copies()
    eng.sync()
    assert all(torch.equal(g, o) and torch.equal(g, c) for g, o, c in zip(got, outs, cat())), "the three forms disagree"
    del got
    med, raw = timed(eng, {"kernel": kernel, "span_copies": copies, "torch_cat": cat}, a.steps, a.warmup)
    row = {"case": case, "rows": a.rows, "spans": sum(len(p) for p in lists), "cells_bytes": cells_bytes, "ms": {k: round(v, 4) for k, v in med.items()}, "steps_ms": raw,
           "kernel_fraction_of_hbm_peak": round(2 * cells_bytes / (med["kernel"] * 1e-3) / HBM_PEAK, 4)}
    eng.close()
    return row


def ingest_case(case, a):
    import numpy as np
    from rayforce_amd import hostobj as H
    ops = H.lib()
    ops.rfx_host_bind()
    rng = np.random.default_rng(3)
    n, nb = a.ingest_rows, max(1, a.ingest_rows // 100)
    tab = lambda rows: H.table(dict(k=rng.integers(0, a.keys, rows), v=rng.integers(-1000, 1000, rows).astype(np.float64), w=rng.integers(0, 1 << 40, rows)))  # noqa: E731
    t = tab(n)
    sel_ms, app_ms, ups = [], [], []
    for step in range(a.warmup + a.steps):
        b = tab(nb)
        t0 = time.perf_counter()
        r = ops.rfx_concat(t, b)
        t1 = time.perf_counter()
        assert not H.is_error(r) and ops.rfx_last_concat_on_gpu() == 1
        d = H.select_dict(dict(s=("sum", "v"), by="k"), r)
        s0 = H.to_numpy(ops.rfx_stats(0))[4]
        t2 = time.perf_counter()
        ans = ops.rfx_select(d)
        t3 = time.perf_counter()
        assert not H.is_error(ans) and ops.rfx_last_select_on_gpu() == 1
        if step >= a.warmup:
            app_ms.append((t1 - t0) * 1e3)
            sel_ms.append((t3 - t2) * 1e3)
            ups.append(int(H.to_numpy(ops.rfx_stats(0))[4] - s0))
        for o in (ans, d, b, t):
            ops.rfx_host_drop(o)
        t = r
    return {"case": case, "rows": n, "batch": nb, "keys": a.keys, "adopt": os.environ.get("RFX_CONCAT_ADOPT", "1"), "select_after_append_ms": round(statistics.median(sel_ms), 4),
            "append_ms": round(statistics.median(app_ms), 4), "uploads_per_select": ups, "select_steps_ms": [round(x, 4) for x in sel_ms]}


def reference(a):
    import numpy as np
    from oracle import ref
    row = {"case": "reference", "rows": a.rows}
    if not ref.available():
        row["ref_ms"] = "not measured"
        return row
    rng = np.random.default_rng(1)
    n = a.ref_rows
    row["rows"] = n
    for th in (1, 8):
        with ref.Session() as s:
            for c in ("k", "t", "p", "q"):
                s.put(c, rng.integers(0, 1 << 40, n))
                s.put(c + "b", rng.integers(0, 1 << 40, n // 100))
            s.eval("(set x (table [k t p q] (list k t p q)))")
            s.eval("(set y (table [k t p q] (list kb tb pb qb)))")
            s.eval("(set l (list k t p q k t p q k t p q k t p q))")
            for c in ("k", "t", "p", "q"):
                s.eval(f"(set t_{c} (sum {c}))")  # (every page of the mapped column files is touched before the timed calls)
            s.eval("(println (timeit (concat x y)))")
            s.eval("(println (timeit (raze l)))")
            out = ref.run_script("\n".join(s.lines) + "\n", threads=th, timeout=900)
        try:
            for name, ms in zip(("ref_concat_table", "ref_raze_16_spans"), out.strip().splitlines()[-2:]):
                row[f"{name}_{th}t_ms"] = round(float(ms), 2)
        except ValueError:
            row[f"ref_{th}t_ms"] = "not measured"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--ingest-rows", type=int, default=10_000_000)
    ap.add_argument("--ref-rows", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", type=int, default=1)
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    if a.case:
        row = reference(a) if a.case == "reference" else (ingest_case(a.case, a) if a.case.startswith("ingest") else device_case(a.case, a))
        print(json.dumps(row), flush=True)
        return
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"concat_bench_run{a.run}.jsonl")
    with open(path, "w") as f:
        for case in CASES:
            env = dict(os.environ)
            if case == "ingest_no_adopt":
                env["RFX_CONCAT_ADOPT"] = "0"
            cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", case] + [x for k in ("rows", "ingest_rows", "ref_rows", "keys", "steps", "warmup")
                                                                                                             for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env)
            if p.returncode != 0:
                print(json.dumps({"case": case, "failed": p.returncode, "stderr": p.stderr[-800:]}), flush=True)
                if case != "reference":
                    sys.exit(1)  # (nothing more on the GPU after a child that did not end cleanly)
                continue
            line = p.stdout.strip().splitlines()[-1]
            f.write(line + "\n")
            f.flush()
            print(line, flush=True)


if __name__ == "__main__":
    main()
