"""Timing of upsert (rfx_upsert.hip) on one device.  One JSON line per case into profiles/upsert_bench_run<N>.jsonl (and to stdout); every GPU case runs
in a child process of its own under its own time limit (`timeout -k 10`), and nothing more is started on the GPU after a child that did not end cleanly.
--steps timed steps after --warmup, the arms alternating step by step in one process, a device synchronise inside the timed region; medians.

  k<K>_b<M>_<P>   a 4-column I64 / F64 table of --rows rows with ascending keys (K = 2: the pair (key // 1000, key % 1000)), a batch of M rows of which P per
                  cent match (hot: every batch row hits one of 1 000 keys -- the worst case for the atomicMax).  Arms: `upsert` (Engine.upsert: index, plan,
                  copy, place), `concat_floor` (Engine.concat of the same table and an all-new batch: what the n-cell copy costs at least), `torch` (the outside
                  yardstick on the same tensors: searchsorted over the ascending keys, a torch.unique last-occurrence pass, torch.cat + index_copy_).  The phases
                  `index`, `plan`, `copy`, `place` are timed one by one with HIP events (rfx_hip_timer) in the same process.
                  `place_fraction_of_hbm_peak`: (8 B of dest + two cells per row and column) over the place kernel's time over 8 TB/s.
  door_adopt / door_no_adopt   through the door on host objects: (upsert t 1 batch) with its read-back, then select {s: (sum v) by: g} over the answer, with
                  adoption on and off (RFX_CONCAT_ADOPT): the select's time and uploads.  --door-rows rows.
  reference       the compiled reference's own upsert with 1 and 8 threads (oracle/_ref/rayforce, when present) at --ref-rows rows and a batch of
                  --ref-batch, 50 per cent matched.

    python tools/bench_upsert.py [--rows 100000000] [--steps 7] [--warmup 2] [--run 1] [--case NAME]
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
DEVICE_CASES = tuple(f"k{k}_b{b}_{p}" for k in (1, 2) for b in (100_000, 10_000_000) for p in ("0", "50", "100", "hot"))
CASES = DEVICE_CASES + ("door_adopt", "door_no_adopt", "reference")


def device_case(case, a):
    import torch
    from rayforce_amd import _lib as L
    from rayforce_amd.engine import Engine
    eng = Engine(0)
    dev = eng.device
    nk, m, pct = case.split("_")
    nk, m, n = int(nk[1:]), int(m[1:]), a.rows
    g = torch.Generator(device=dev).manual_seed(5)
    key = torch.arange(n, device=dev)  # ascending and unique: what the torch arm's searchsorted needs
    if pct == "hot":
        bkey = torch.randint(0, 1000, (m,), device=dev, generator=g) * (n // 1000)
    else:
        hit = torch.randint(0, n, (m,), device=dev, generator=g)
        new = n + torch.randperm(m, device=dev, generator=g)
        bkey = torch.where(torch.rand(m, device=dev, generator=g) * 100 < int(pct), hit, new)
    split = (lambda k: [k // 1000, k % 1000]) if nk == 2 else (lambda k: [k])
    names = [f"k{i}" for i in range(nk)] + ["p", "q", "r"][: 4 - nk]
    vals = lambda rows: [torch.rand(rows, dtype=torch.float64, device=dev, generator=g), torch.randint(0, 1 << 40, (rows,), device=dev, generator=g),  # noqa: E731
                         torch.rand(rows, dtype=torch.float64, device=dev, generator=g)][: 4 - nk]
    t = dict(zip(names, split(key) + vals(n)))
    b = dict(zip(names, split(bkey) + vals(m)))
    allnew = dict(b, **dict(zip(names[:nk], split(n + torch.arange(m, device=dev)))))

    def torch_arm():
        pos = torch.searchsorted(key, bkey).clamp(max=n - 1)
        matched = key[pos] == bkey
        rows, j = pos[matched], torch.nonzero(matched).reshape(-1)
        u, inv = torch.unique(rows, return_inverse=True)
        last = torch.full((u.numel(),), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, j, "amax")
        out = {}
        for i, c in enumerate(names):
            o = torch.cat([t[c], b[c][~matched]])
            if i >= nk and u.numel():
                o.index_copy_(0, u, b[c][last])
            out[c] = o
        return out

    got, want = eng.upsert(t, nk, b), torch_arm()
    assert all(torch.equal(got[c].view(torch.int64), want[c].view(torch.int64)) for c in names), "the device and the torch composition disagree"
    a_rows = got[names[0]].numel() - n
    del got, want
    forms = {"upsert": lambda: eng.upsert(t, nk, b), "concat_floor": lambda: eng.concat(t, allnew), "torch": torch_arm}
    ms = {k: [] for k in forms}
    for step in range(a.warmup + a.steps):
        for name, f in forms.items():
            eng.sync()
            t0 = time.perf_counter()
            f()
            eng.sync()
            if step >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    # the phases one by one, by HIP events
    idx, dest = eng.empty(m), eng.empty(m)
    tk = (C.c_void_p * nk)(*[t[c].data_ptr() for c in names[:nk]])
    bk = (C.c_void_p * nk)(*[b[c].data_ptr() for c in names[:nk]])
    und, app = C.c_int(0), C.c_int64(0)
    outs = [eng.empty(n + a_rows, t[c].dtype) for c in names]
    pc = (L.UpsertCol * 4)()
    for i, c in enumerate(names):
        pc[i].d_batch, pc[i].d_out, pc[i].width, pc[i].appends_only = b[c].data_ptr(), outs[i].data_ptr(), 8, int(i < nk)
    phases = {
        "index": lambda: eng._xcheck(eng.lib.rfx_exec_upsert_index(eng._x, tk, bk, nk, n, m, idx.data_ptr(), C.byref(und)), "index"),
        "plan": lambda: eng._xcheck(eng.lib.rfx_exec_upsert_plan(eng._x, idx.data_ptr(), m, n, dest.data_ptr(), C.byref(app)), "plan"),
        "copy": lambda: eng._concat_cols([[t[c]] for c in names]),
        "place": lambda: L.check(eng.lib.rfx_hip_upsert_place(eng._ctx, pc, 4, dest.data_ptr(), m, n, n + a_rows), "place"),
    }
    pms = {k: [] for k in phases}
    for step in range(a.warmup + a.steps):
        for name, f in phases.items():
            eng.sync()
            eng.timer_start()
            f()
            v = eng.timer_stop()
            if step >= a.warmup:
                pms[name].append(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    pmed = {k: statistics.median(v) for k, v in pms.items()}
    place_bytes = m * 8 + 2 * 8 * (m * (4 - nk) + a_rows * nk)
    row = {"case": case, "rows": n, "batch": m, "keys": nk, "appended": a_rows, "ms": {k: round(v, 4) for k, v in med.items()}, "phase_ms": {k: round(v, 4) for k, v in pmed.items()},
           "steps_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "place_model_bytes": place_bytes,
           "place_fraction_of_hbm_peak": round(place_bytes / (pmed["place"] * 1e-3) / HBM_PEAK, 5),
           "copy_over_concat_floor": round(pmed["copy"] / med["concat_floor"], 4)}
    eng.close()
    return row


def door_case(case, a):
    import numpy as np
    from rayforce_amd import hostobj as H
    ops = H.lib()
    ops.rfx_host_bind()
    rng = np.random.default_rng(3)
    n, nb = a.door_rows, max(1, a.door_rows // 100)
    t = H.table(dict(k=np.arange(n, dtype=np.int64) * 2, g=rng.integers(0, 100_000, n), v=rng.integers(-1000, 1000, n).astype(np.float64), w=rng.integers(0, 1 << 40, n)))
    one = ops.rfx_host_i64(1)
    sel_ms, up_ms, ups, rows = [], [], [], n
    for step in range(a.warmup + a.steps):
        b = H.table(dict(k=rng.integers(0, 4 * rows, nb), g=rng.integers(0, 100_000, nb), v=rng.integers(-1000, 1000, nb).astype(np.float64), w=rng.integers(0, 1 << 40, nb)))
        t0 = time.perf_counter()
        r = ops.rfx_upsert((C.c_void_p * 3)(t, one, b), 3)
        t1 = time.perf_counter()
        assert not H.is_error(r) and ops.rfx_last_upsert_on_gpu() == 1, ops.rfx_ops_last_error().decode()
        d = H.select_dict(dict(s=("sum", "v"), by="g"), r)
        s0 = H.to_numpy(ops.rfx_stats(0))[4]
        t2 = time.perf_counter()
        ans = ops.rfx_select(d)
        t3 = time.perf_counter()
        assert not H.is_error(ans) and ops.rfx_last_select_on_gpu() == 1
        if step >= a.warmup:
            up_ms.append((t1 - t0) * 1e3)
            sel_ms.append((t3 - t2) * 1e3)
            ups.append(int(H.to_numpy(ops.rfx_stats(0))[4] - s0))
        for o in (ans, d, b, t):
            ops.rfx_host_drop(o)
        t = r
    return {"case": case, "rows": n, "batch": nb, "adopt": os.environ.get("RFX_CONCAT_ADOPT", "1"), "upsert_with_read_back_ms": round(statistics.median(up_ms), 4),
            "select_after_upsert_ms": round(statistics.median(sel_ms), 4), "uploads_per_select": ups, "select_steps_ms": [round(x, 4) for x in sel_ms]}


def reference(a):
    import numpy as np
    from oracle import ref
    row = {"case": "reference", "rows": a.ref_rows, "batch": a.ref_batch}
    if not ref.available():
        row["ref_ms"] = "not measured"
        return row
    rng = np.random.default_rng(1)
    n, m = a.ref_rows, a.ref_batch
    for th in (1, 8):
        with ref.Session() as s:
            s.put("k", np.arange(n, dtype=np.int64) * 2)
            s.put("kb", rng.integers(0, 4 * n, m))
            for c in ("p", "q", "r"):
                s.put(c, rng.integers(0, 1 << 40, n))
                s.put(c + "b", rng.integers(0, 1 << 40, m))
            s.eval("(set x (table [k p q r] (list k p q r)))")
            s.eval("(set y (list kb pb qb rb))")
            for c in ("k", "p", "q", "r"):
                s.eval(f"(set t_{c} (sum {c}))")  # (every page of the mapped column files is touched before the timed call)
            s.eval("(println (timeit (upsert x 1 y)))")
            try:
                out = ref.run_script("\n".join(s.lines) + "\n", threads=th, timeout=100)
                row[f"ref_upsert_{th}t_ms"] = round(float(out.strip().splitlines()[-1]), 2)
            except (ValueError, RuntimeError, subprocess.TimeoutExpired):
                row[f"ref_upsert_{th}t_ms"] = "not measured"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--door-rows", type=int, default=10_000_000)
    ap.add_argument("--ref-rows", type=int, default=10_000_000)
    ap.add_argument("--ref-batch", type=int, default=10_000)
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
    path = os.path.join(ROOT, "profiles", f"upsert_bench_run{a.run}.jsonl")
    with open(path, "w") as f:
        for case in (a.only.split(",") if a.only else CASES):
            env = dict(os.environ)
            if case == "door_no_adopt":
                env["RFX_CONCAT_ADOPT"] = "0"
            cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", case] + [x for k in ("rows", "door_rows", "ref_rows", "ref_batch", "steps", "warmup")
                                                                                                             for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
            p = subprocess.run(cmd, capture_output=True, text=True, env=env)
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
