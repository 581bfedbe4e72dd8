"""Timing of the device set verbs (rfx_set.hip through rfx_exec_distinct / rfx_exec_member / rfx_exec_set_filter) on device-resident columns of
--rows cells: `distinct` of 1e6 dense keys and of 1e7 / --rows keys spread over 1e12 (the hash route); `in` and `find` of --rows cells against 1e6
and against --rows keys on both routes; `sect` / `except` fused (one probe + ordered compaction of the values) against the unfused chain
(in -> where -> at) in the same run; `union` of two halves.  Per case: the mean of --steps timed steps after --warmup (a device synchronise inside
the timed region), the planner's own build / probe split (RFX_XSTAT_NS_SET_*, means over the timed steps), the bytes the verb must at least move
(operands read once + the answer written once) and what fraction of the 8 TB/s roofline that is.  Yardsticks in the same run, named for what they
are: `torch_ms` -- torch.unique / torch.isin / torch.sort on the same tensors -- and, for the cases named by --ref-cases, `ref_ms_threads8` /
`_threads1`: the compiled reference's own verb under its `timeit` on this box's CPU (oracle/_ref/rayforce -c 8 / -c 1 where it was built, column
files loaded outside the timed expression).  One JSON line per case; a step that ran longer than --limit seconds ends the case ("over the limit").  That limit is read AFTER a step returns: it
keeps a slow case from running all its steps, it cannot end a step that hangs -- run the tool under an outer `timeout -k 10 SECONDS` sized to the run.

    python tools/bench_set.py [--rows 1e8] [--steps 5] [--warmup 1] [--ref-cases distinct_dense,in_dense_1e6] [--ref-rows 1e7] [--only distinct,in]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rayforce_amd import _lib as L  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402

ROOF = 8e12  # bytes / s


def timed(fn, steps, warmup, limit):
    """mean milliseconds of the timed steps only; None when a step ran over the limit (checked once the step has returned)"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        if ts[-1] > limit * 1e3:
            return None
    return sum(ts) / len(ts)


def reference_ms(expr, cols, threads):
    """`expr` over the named columns inside the reference binary under its own timeit; None when the binary is not beside the tree"""
    from oracle import ref
    if not ref.available():
        return None
    with ref.Session() as s:
        for k, v in cols.items():
            s.put(k, v.cpu().numpy())
        s.out("ms", f"(enlist (timeit {expr}))")
        return float(s.run(threads=threads, timeout=1500.0)["ms"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds one step may take")
    ap.add_argument("--only", default="", help="comma-separated verbs (distinct,in,find,sect,except,union); default all")
    ap.add_argument("--ref-cases", default="none", help="comma-separated case names to time in the reference too, or none")
    ap.add_argument("--ref-rows", type=float, default=1e7, help="the reference is timed on the first this many cells (its figure names them)")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    n = int(a.rows)
    only = set(a.only.split(",")) if a.only else None
    refs = set() if a.ref_cases == "none" else set(a.ref_cases.split(","))
    eng = Engine(0)
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda hi, m: torch.randint(0, hi, (m,), dtype=torch.int64, device=dev, generator=g)
    stat = lambda: [eng.xstat(s) for s in (L.RFX_XSTAT_NS_SET_BUILD, L.RFX_XSTAT_NS_SET_PROBE)]

    def spread(keys, m):  # m cells drawn from `keys` distinct keys spread over 1e12
        if keys >= m:
            x = rnd(10**12, m)
        else:
            x = rnd(10**12, keys)[rnd(keys, m)]
        x[0], x[1] = 0, 10**12
        return x

    def report(name, verb, fn, bytes_moved, torch_fn=None, ref=None, extra=None):
        if only is not None and verb not in only:
            return
        for _ in range(a.warmup):
            fn()
        before = stat()
        ms = timed(fn, a.steps, 0, a.limit)
        after = stat()
        row = {"case": name, "rows": n, "route": eng.last_set_route, "steps": a.steps}
        if ms is None:
            row["ms"] = "over the limit"
        else:
            row.update(ms=round(ms, 3), build_ms=round((after[0] - before[0]) / a.steps / 1e6, 3), probe_ms=round((after[1] - before[1]) / a.steps / 1e6, 3),
                       min_bytes=bytes_moved, achieved_tb_s=round(bytes_moved / (ms * 1e-3) / 1e12, 3), roofline_fraction=round(bytes_moved / (ms * 1e-3) / ROOF, 3))
        if extra:
            row.update(extra())
        if torch_fn is not None and not a.no_torch:
            try:
                t = timed(torch_fn, a.steps, a.warmup, a.limit)
                row["torch_ms"] = round(t, 3) if t is not None else "over the limit"
            except RuntimeError as e:  # (torch.unique / isin sort: out of memory at the largest sizes)
                row["torch_ms"] = "not measured: " + str(e)[:60]
            torch.cuda.empty_cache()
        if ref is not None and name in refs:
            expr, cols = ref
            m = int(a.ref_rows)
            cols = {k: v[:m] for k, v in cols.items()}
            for th in (8, 1):
                print(f"reference {expr}, {th} thread(s), {m} cells ...", file=sys.stderr, flush=True)
                r = reference_ms(expr, cols, th)
                row[f"ref_ms_threads{th}"] = round(r, 1) if r is not None else "not measured"
            row["ref_rows"] = m
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        eng.trim()

    # ---- distinct
    x = rnd(10**6, n)
    report("distinct_dense", "distinct", lambda: eng.distinct(x), n * 8 + 10**6 * 8, lambda: torch.unique(x), ("(distinct x)", {"x": x}))
    for keys in (10**7, n):
        x = spread(keys, n)
        d = min(keys, n)
        report(f"distinct_hash_{keys:.0e}_keys", "distinct", lambda: eng.distinct(x), n * 8 + d * 8, lambda: torch.unique(x), ("(distinct x)", {"x": x}))
    # ---- in / find: n cells against 1e6 and against n keys, both routes
    for keys in (10**6, n):
        for route in ("dense", "hash"):
            # (dense: the two scopes meet in at most 2^20 values, however many cells hold them)
            x = rnd(2**20, n) if route == "dense" else spread(max(2, 2 * keys), n)
            y = rnd(2**20, keys) if route == "dense" else x[rnd(n, keys)].clone()
            if route == "hash":
                y[: keys // 2] = rnd(10**12, keys // 2)  # (half of the keys occur in x, half do not)
                y[0] = 10**12
            report(f"in_{route}_{keys:.0e}", "in", lambda: eng.isin(x, y), n * 9 + keys * 8, lambda: torch.isin(x, y), ("(in x y)", {"x": x, "y": y}))
            report(f"find_{route}_{keys:.0e}", "find", lambda: eng.find(y, x), n * 16 + keys * 8, None, ("(find y x)", {"x": x, "y": y}))
            if keys == 10**6:
                for verb, fused, keep in (("sect", eng.sect, True), ("except", eng.except_, False)):
                    def unfused():
                        m = eng.isin(x, y)
                        ids = eng.where(m if keep else 1 - m)
                        return eng.at_ids(x, ids)
                    kept = int(fused(x, y).numel())
                    report(f"{verb}_{route}_fused", verb, lambda: fused(x, y), n * 8 + keys * 8 + kept * 8, None, (f"({verb} x y)", {"x": x, "y": y}))
                    report(f"{verb}_{route}_unfused_in_where_at", verb, unfused, n * 8 + keys * 8 + kept * 8)
            del x, y
    # ---- union of two halves
    h = n // 2
    x, y = rnd(10**6, h), rnd(2 * 10**6, h)
    report("union_dense_halves", "union", lambda: eng.union(x, y), n * 8 + 2 * 10**6 * 8, lambda: torch.unique(torch.cat([x, y])), ("(union x y)", {"x": x, "y": y}))
    x, y = spread(10**7, h), spread(10**7, h)
    report("union_hash_halves", "union", lambda: eng.union(x, y), n * 8 + 2 * 10**7 * 8, lambda: torch.unique(torch.cat([x, y])), ("(union x y)", {"x": x, "y": y}))
    eng.close()


if __name__ == "__main__":
    main()
