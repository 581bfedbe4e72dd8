"""Drop-in proof for `last` and `dev` in select: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and answers
the same queries twice in ONE process -- by the plugin and by its own ray_select.  The OHLC query over 8 000 rows with a pool of 8 (fewer than 16 384
selected rows: aggr_map does not split, the reference's answer is its one-chunk answer) and over 40 000 rows with a pool of 1; the scalar `dev`; and the
shapes the plugin hands back (dev under by: / where:, where the reference itself answers null).  last and every integer column agree bit for bit; the
scalar dev within lastdev_ref.dev_close's bound."""
import os

import numpy as np
import pytest

import lastdev_ref as R
from oracle import ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")

OHLC = "{o: (first p) h: (max p) l: (min p) c: (last p) cf: (last f) from: trades by: {s: s b: (xbar ts 5000)}}"
OHLC_W = "{o: (first p) c: (last p) from: trades where: (< a 60) by: s}"


@pytest.mark.parametrize("n,threads", [(8_000, 8), (40_000, 1)])
def test_ohlc_and_dev_inside_the_real_reference(built, n, threads):
    import torch
    assert torch.cuda.is_available()
    assert ref.available(), "oracle/_ref/rayforce is not built"
    rng = np.random.default_rng(n)
    cols = {"s": rng.integers(0, 40, n), "ts": np.sort(rng.integers(0, 100_000, n)), "p": rng.integers(1, 10**6, n), "f": rng.standard_normal(n) + 100.0,
            "a": rng.integers(0, 100, n)}
    # 30 % nulls in p -- but never on the first row of a group of either query: what `first` answers over a null first row is not this test's subject
    nul = rng.random(n) < 0.3
    for key, sel in ((cols["s"] * 1_000_000 + (cols["ts"] // 5000) * 5000, np.ones(n, bool)), (cols["s"], cols["a"] < 60)):
        rows = np.flatnonzero(sel)
        nul[rows[np.unique(key[rows], return_index=True)[1]]] = False
    cols["p"][nul] = R.NULL_I64
    cols["f"][rng.random(n) < 0.3] = np.nan
    with ref.Session() as s:
        s.table("trades", cols)
        s.eval(f'(set gsel (loadfn "{LIB}" "rfx_select" 1))')
        s.eval(f'(set gstat (loadfn "{LIB}" "rfx_stats" 1))')
        outs = []
        for name, q, names in (("ohlc", OHLC, ["s", "b", "o", "h", "l", "c", "cf"]), ("ohlcw", OHLC_W, ["s", "o", "c"]),
                               ("sc", "{c: (last p) d: (dev p) df: (dev f) from: trades}", ["c", "d", "df"]),
                               ("scw", "{c: (last p) from: trades where: (< a 60)}", ["c"])):
            s.eval(f"(set g_{name} (gsel {q}))")
            s.eval(f"(set r_{name} (select {q}))")
            for c in names:
                s.out(f"g_{name}_{c}", f"(at g_{name} '{c})")
                s.out(f"r_{name}_{c}", f"(at r_{name} '{c})")
                outs.append(f"{name}_{c}")
        s.out("stats_on", "(gstat 0)")
        # handed back: the reference answers null in every cell there (ray_dev's l = ray_cnt(pair) reads 0), and so does the plugin -- through the host
        for name, q in (("dby", "{d: (dev p) from: trades by: s}"), ("dwh", "{d: (dev p) from: trades where: (< a 60)}")):
            s.eval(f"(set g_{name} (gsel {q}))")
            s.eval(f"(set r_{name} (select {q}))")
            s.out(f"g_{name}_d", f"(at g_{name} 'd)")
            s.out(f"r_{name}_d", f"(at r_{name} 'd)")
        s.out("stats", "(gstat 0)")
        res = s.run(threads=threads)
    for name in outs:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape, name
        if name in ("sc_d", "sc_df"):
            col = cols["p" if name == "sc_d" else "f"]
            print(name, "device", float(g[0]), "reference", float(r[0]))
            assert R.dev_close(float(g[0]), float(r[0]), col), (name, g, r)
        else:
            assert R.same_bits(g, r), (name, int((g.view(np.int64) != r.view(np.int64)).sum()))
    # the reference's own answer is the one-chunk answer here
    b = (cols["ts"] // 5000) * 5000
    combined = cols["s"] * 1_000_000 + b
    uk, inv = np.unique(combined, return_inverse=True)
    want = R.group_last(cols["p"], inv.reshape(-1), len(uk))
    at = np.searchsorted(uk, res["r_ohlc_s"] * 1_000_000 + res["r_ohlc_b"])
    assert len(at) == len(uk) and R.same_bits(res["r_ohlc_c"], want[at])
    assert res["stats_on"][0] == 4 and res["stats_on"][1] == 0  # selects on the GPU, selects delegated
    for name in ("dby", "dwh"):
        assert R.same_bits(res[f"g_{name}_d"], res[f"r_{name}_d"]) and np.isnan(res[f"r_{name}_d"]).all(), name
    assert res["stats"][0] == 4 and res["stats"][1] == 2
