"""Timing of the open / high / low / close query on the device,

    select {o: (first p) h: (max p) l: (min p) c: (last p) from: trades by: {s: sym b: (xbar ts w)}}

over --rows trades of --keys symbols (ts ascending; w splits the day into 8 bars), through the operator door (rfx_select over device column handles: the
whole query with its plan walk, the result's read-back and the host table) and through the planner alone (Engine.select: device results).  Beside it the
CONTROL: the same query with (max q) over a second i64 column in place of (last p) -- what `last` costs over a MAX of an i64 column is the difference
(`last` is planned as such a MAX over a derived row column, plus the pass that derives it and the gather at the end).  Every answer is checked against
torch.  Per case: the median of --steps timed steps after --warmup, and the shader clock the device ran at.  One JSON line per case.

    python tools/bench_ohlc.py [--rows 100000000,1000000000] [--keys 1000,1000000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rayforce_amd import hostobj as H  # noqa: E402
from rayforce_amd.engine import Engine  # noqa: E402
from bench_median import hwmon, timed  # noqa: E402

NULL = -(2**63)


def torch_answer(s, b, p, q):
    """(keys, open, high, low, close, max q) per (s, b) group in ascending (s, b) order; nulls skipped by min / max / last, first positional"""
    comb = s * (1 << 32) + b
    uk, inv = torch.unique(comb, return_inverse=True)
    g, n = len(uk), len(comb)
    rows = torch.arange(n, device=comb.device)
    big = torch.iinfo(torch.int64)
    first = torch.full((g,), n, dtype=torch.int64, device=comb.device).scatter_reduce(0, inv, rows, "amin")
    ok = p != NULL
    lastrow = torch.full((g,), -1, dtype=torch.int64, device=comb.device).scatter_reduce(0, inv[ok], rows[ok], "amax")
    hi = torch.full((g,), big.min, dtype=torch.int64, device=comb.device).scatter_reduce(0, inv[ok], p[ok], "amax")
    lo = torch.full((g,), big.max, dtype=torch.int64, device=comb.device).scatter_reduce(0, inv[ok], p[ok], "amin")
    close = torch.where(lastrow >= 0, p[lastrow.clamp(min=0)], torch.full_like(lastrow, NULL))
    mq = torch.full((g,), big.min, dtype=torch.int64, device=comb.device).scatter_reduce(0, inv, q, "amax")
    return uk, p[first], hi, lo, close, mq, lastrow >= 0


def check(res, want, control):
    uk, o, h, l, c, mq, has = want
    comb = res["s"] * (1 << 32) + res["b"]
    order = torch.argsort(comb)
    assert torch.equal(comb[order], uk), "groups"
    assert torch.equal(res["o"][order], o), "first"
    assert torch.equal(res["h"][order][has], h[has]) and torch.equal(res["l"][order][has], l[has]), "max / min"
    assert torch.equal(res["c"][order], mq if control else c), "max (control)" if control else "last"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000000,1000000000")
    ap.add_argument("--keys", default="1000,1000000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    eng = Engine(0)
    ops = H.lib()
    ops.rfx_host_bind()
    clock = hwmon(eng.device.index)
    gen = torch.Generator(device=eng.device).manual_seed(1)
    for n in [int(x) for x in a.rows.split(",")]:
        for keys in [int(x) for x in a.keys.split(",")]:
            day = 8 * 3_600_000
            w = day // 8
            t = {"s": torch.randint(0, keys, (n,), dtype=torch.int64, device=eng.device, generator=gen),
                 "ts": torch.sort(torch.randint(0, day, (n,), dtype=torch.int64, device=eng.device, generator=gen)).values,
                 "p": torch.randint(1, 1 << 40, (n,), dtype=torch.int64, device=eng.device, generator=gen),
                 "q": torch.randint(1, 1 << 40, (n,), dtype=torch.int64, device=eng.device, generator=gen)}
            t["p"][torch.rand(n, device=eng.device, generator=gen) < 0.05] = NULL
            want = torch_answer(t["s"], (t["ts"] // w) * w, t["p"], t["q"])
            tab = H.device_table(t)
            for control in (False, True):
                close = ("max", "q") if control else ("last", "p")
                q = {"by": {"s": "s", "b": ("xbar", "ts", w)}, "o": ("first", "p"), "h": ("max", "p"), "l": ("min", "p"), "c": close}
                res = eng.select({"from": t, **q})
                check(res, want, control)
                d = H.select_dict(q, tab)

                def door():
                    r = ops.rfx_select(d)
                    assert not H.is_error(r), H.error_text(r)
                    ops.rfx_host_drop(r)
                r = ops.rfx_select(d)
                assert not H.is_error(r) and ops.rfx_last_select_on_gpu() == 1, ops.rfx_ops_last_error()
                got = {k: torch.from_numpy(v).to(eng.device) for k, v in H.table_to_numpy(r).items()}
                ops.rfx_host_drop(r)
                check(got, want, control)
                t_door, mhz = timed(door, a.steps, a.warmup, clock)
                t_plan, _ = timed(lambda: eng.select({"from": t, **q}), a.steps, a.warmup, None)
                ops.rfx_host_drop(d)
                print(json.dumps({"case": "ohlc, control: (max q) for (last p)" if control else "ohlc", "rows": n, "keys": keys, "groups": int(len(want[0])),
                                  "door_ms": round(t_door, 3), "planner_ms": round(t_plan, 3), "sclk_mhz": mhz, "steps": a.steps, "checked": "torch"}), flush=True)
            ops.rfx_host_drop(tab)
            del t, want, res, got
            torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
