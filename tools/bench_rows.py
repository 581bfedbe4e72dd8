#!/usr/bin/env python
"""Timings of the row verbs on one MI355X (none is asserted anywhere):

    python tools/bench_rows.py [--rows 100000000] [--reps 5]

filter of 1, 4 and 8 I64 columns at 1 %, 10 % and 50 % selectivity through its two write-outs (ring, direct) and, in the same run, the composed path
Engine.where + at_ids per column; head and cyclic take and reverse against their byte roofline (8 TB/s); filter through the door over device-column
handles and take / reverse through the door (read-back included); with --reference the compiled reference's own verbs with 1 and 8 threads.  Run it twice: the ring form ships only where
it beats the direct form by more than the spread between the two runs.  One JSON line per figure."""
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
from rayforce_amd import hostobj as H  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    n, eng = a.rows, Engine(0)
    cols = [eng.gen_i64(n, 10 + k, 1_000_000_000) for k in range(8)]
    key = eng.gen_i64(n, 3, 1000)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    for pct in (1, 10, 50):
        tree = ("<", key, pct * 10)
        mask = eng.mask_of(tree)
        for ncols in (1, 4, 8):
            tab = {f"c{k}": cols[k] for k in range(ncols)}
            res = {form: timed(lambda f=form: eng.filter(tab, mask, form=f), a.reps) for form in ("ring", "direct")}
            res["fused_tree_direct"] = timed(lambda: eng.filter(tab, tree, form="direct"), a.reps)

            def composed():
                ids = eng.where(mask)
                return [eng.at_ids(c, ids) for c in tab.values()]
            res["where_at_ids"] = timed(composed, a.reps)
            emit(verb="filter", rows=n, selectivity=pct, columns=ncols, ms=res)
    for name, fn, byts in (("take_head", lambda: eng.take(cols[0], n // 2), n // 2 * 16), ("take_cyclic", lambda: eng.take(cols[0], -(n + n // 2)), (n + n // 2) * 16),
                           ("reverse", lambda: eng.reverse(cols[0]), n * 16)):
        ms = timed(fn, a.reps)
        emit(verb=name, rows=n, ms=ms, roofline_fraction=byts / 8e12 * 1e3 / ms)
    ops = H.lib()
    ops.rfx_host_bind()
    hm = ops.rfx_host_device_vector(1, n, (C.c_void_p * 1)(eng.mask_of(("<", key, 100)).data_ptr()), 1)
    hc = ops.rfx_host_device_vector(5, n, (C.c_void_p * 1)(cols[0].data_ptr()), 1)

    def door():
        r = ops.rfx_filter(hc, hm)
        assert r and not H.is_error(r) and ops.rfx_last_rows_on_gpu() == 1
        ops.rfx_host_drop(r)
    emit(verb="filter_door_device_handles", rows=n, selectivity=10, ms=timed(door, a.reps))
    cnt = {"head": H.atom(n // 2), "cyclic": H.atom(-(n + n // 2))}

    def door_call(fn, *args):
        def run():
            r = fn(hc, *args)
            assert r and not H.is_error(r) and ops.rfx_last_rows_on_gpu() == 1
            ops.rfx_host_drop(r)
        return run
    for name, run in (("take_head", door_call(ops.rfx_take, cnt["head"])), ("take_cyclic", door_call(ops.rfx_take, cnt["cyclic"])), ("reverse", door_call(ops.rfx_reverse))):
        emit(verb=name + "_door_device_handle", rows=n, ms=timed(run, max(1, a.reps // 2)))  # (read-back into a fresh host vector included)
    if a.reference:
        from oracle import ref, rfo
        for threads in (1, 8):
            with ref.Session() as s:
                s.put("v", rfo.gen_i64(n, 10, 1_000_000_000))
                s.put("m", (rfo.gen_i64(n, 3, 1000) < 100).astype(np.int8))
                for call in ("filter v m", f"take v {n // 2}", f"take v {-(n + n // 2)}", "reverse v"):
                    s.eval(f'(println "{call}" (timeit ({call})))')
                emit(verb="reference", threads=threads, stdout=s.run(threads=threads)["_stdout"])
    eng.close()


if __name__ == "__main__":
    main()
