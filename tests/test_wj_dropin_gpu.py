"""Drop-in proof for window-join and window-join1: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and
answers the same tables twice in ONE process -- by the plugin and by its own built-ins -- with a pool of 8: 1e5 trades against 2e5 quotes, the quotes
sorted by time and shuffled, and a trades table with symbols the quotes lack.  Integer columns and the F64 min / max / first / last agree bit for bit;
F64 sum / avg (non-negative cells: no cancellation) within the project's 1e-9 relative rule for F64 sums -- the reference adds in row order, the
device as a tree."""
import os

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
NL, NR = 100_000, 200_000
AGGS = ("sum", "min", "max", "count", "avg", "first", "last")


def test_window_verbs_inside_the_real_reference(built):
    import torch
    assert torch.cuda.is_available()
    assert ref.available(), "oracle/_ref/rayforce is not built"
    rng = np.random.default_rng(41)
    nsym = 40
    day = 3_600_000
    lt = rng.integers(0, day, NL)
    lo, hi = lt - rng.integers(0, 2000, NL), lt + rng.integers(0, 2000, NL)  # ~ 1.4 quotes per second and symbol: windows of 0 .. 6 rows ...
    wide = rng.choice(NL, 300, replace=False)
    lo[wide], hi[wide] = lt[wide] - 600_000, lt[wide] + 600_000              # ... and some of ~ 1 700
    ls = rfo.gen_i64(NL, 4, nsym)
    absent = ls.copy()
    absent[::7] = nsym + 3  # a symbol the quotes lack: null rows
    rs, rt = rfo.gen_i64(NR, 7, nsym), np.sort(rng.integers(0, day, NR))
    vi = rfo.gen_i64(NR, 9, 1_000_000) - 500_000
    vf = np.abs(rfo.gen_f64(NR, 8))
    vi[rng.random(NR) < 0.01] = -(2**63)
    vf[rng.random(NR) < 0.01] = np.nan
    p = rng.permutation(NR)
    with ref.Session() as s:
        s.put("l_s", ls)
        s.put("l_absent", absent)
        for n, v in (("l_t", lt), ("lo", lo), ("hi", hi)):
            s.put(n, v.astype(np.int32), tp=8)
        s.put("l_q", rfo.gen_i64(NL, 6, 100))
        s.eval("(set trades (table [s t q] (list l_s l_t l_q)))")
        s.eval("(set trades2 (table [s t q] (list l_absent l_t l_q)))")
        for tag, order in (("sorted", np.arange(NR)), ("shuffled", p)):
            s.put(f"r_s_{tag}", rs[order])
            s.put(f"r_t_{tag}", rt[order].astype(np.int32), tp=8)
            s.put(f"r_vi_{tag}", vi[order])
            s.put(f"r_vf_{tag}", vf[order])
            s.eval(f"(set quotes_{tag} (table [s t vi vf] (list r_s_{tag} r_t_{tag} r_vi_{tag} r_vf_{tag})))")
        s.eval(f'(set gwj (loadfn "{LIB}" "rfx_window_join" 5))')
        s.eval(f'(set gwj1 (loadfn "{LIB}" "rfx_window_join1" 5))')
        s.eval(f'(set gstat (loadfn "{LIB}" "rfx_stats" 1))')
        aggs = " ".join(f"{a}_{x}: ({a} v{x})" for x in "if" for a in AGGS)
        outs = []
        for tag in ("sorted", "shuffled"):
            for left in ("trades", "trades2"):
                for verb, g in (("window-join", "gwj"), ("window-join1", "gwj1")):
                    name = f"{left}_{tag}_{g}"
                    s.eval(f"(set g_{name} ({g} [s t] (list lo hi) {left} quotes_{tag} {{{aggs}}}))")
                    s.eval(f"(set r_{name} ({verb} [s t] (list lo hi) {left} quotes_{tag} {{{aggs}}}))")
                    for c in ["s", "t", "q"] + [f"{a}_{x}" for x in "if" for a in AGGS]:
                        s.out(f"g_{name}_{c}", f"(at g_{name} '{c})")
                        s.out(f"r_{name}_{c}", f"(at r_{name} '{c})")
                        outs.append(f"{name}_{c}")
        s.out("stats", "(gstat 0)")
        res = s.run(threads=8)
    for name in outs:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape == (NL,), name
        if name.endswith(("sum_f", "avg_f")):
            assert np.array_equal(np.isnan(g), np.isnan(r)), name
            ok = ~np.isnan(r)
            err = np.abs(g[ok] - r[ok])
            print(name, "largest relative error", float((err / np.maximum(np.abs(r[ok]), 1e-300)).max()) if ok.any() else 0.0)
            assert (err <= 1e-9 * np.abs(r[ok])).all(), name
        else:
            assert np.array_equal(g.view(np.int64), r.view(np.int64)), (name, int((g.view(np.int64) != r.view(np.int64)).sum()))
    # the cases are what they are meant to be: null rows for the absent symbol, windows of a lane and of a wave
    cnt = res["r_trades2_sorted_gwj_count_i"]
    assert (cnt[::7] == 0).all() and (cnt > 1000).any() and ((cnt > 0) & (cnt <= 16)).any()
    # (with ties in time WHICH quote is the last one at or before lo depends on the rows' order, so only the counts are the same for both orders)
    assert np.array_equal(res["g_trades_sorted_gwj_count_i"], res["g_trades_shuffled_gwj_count_i"])
    assert not np.array_equal(res["g_trades_sorted_gwj_count_i"], res["g_trades_sorted_gwj1_count_i"])
    assert res["stats"][2] == 8 and res["stats"][3] == 0  # joins on the GPU, joins delegated
