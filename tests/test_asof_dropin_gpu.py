"""Drop-in proof for asof-join, bin and binr: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and
answers the same objects twice in ONE process -- by the plugin and by its own built-ins -- with a pool of 8 (the reference splits the probe over its
pool: chunk = ll / n), over a right table sorted by time and over a shuffled one.  Equality of bits for every typed column; right-only columns are
compared where every row matches (elsewhere the reference returns a LIST of Null objects, this engine typed nulls)."""
import os

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
N = 100_000


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (needs /root/reference at build time)")
def test_asof_verbs_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(31)
    nsym = 300
    trades = {"s": rfo.gen_i64(N, 4, nsym), "t": rng.integers(10, 1_000_000, N), "px": rfo.gen_f64(N, 5), "q": rfo.gen_i64(N, 6, 100)}
    quotes = {"s": rfo.gen_i64(N, 7, nsym), "t": rng.integers(10, 1_000_000, N), "bid": rfo.gen_f64(N, 8), "q": rfo.gen_i64(N, 9, 100) + 1000}
    quotes["s"][:nsym] = np.arange(nsym)  # every symbol's first quote before every trade: in `full` every trade has a quote
    first = quotes["t"].copy()
    first[:nsym] = 1
    tables = {"sorted": np.concatenate([first[:nsym], np.sort(first[nsym:])]), "shuffled": first}
    absent = trades["s"].copy()
    absent[::7] = nsym + 3  # a symbol the quotes lack: those rows stay unmatched
    with ref.Session() as s:
        for k, v in trades.items():
            s.put("l_" + k, v)
        s.put("l_absent", absent)
        for k in ("s", "bid", "q"):
            s.put("r_" + k, quotes[k])
        s.eval("(set trades (table [s t px q] (list l_s l_t l_px l_q)))")
        s.eval("(set trades2 (table [s t px q] (list l_absent l_t l_px l_q)))")
        for tag, t in tables.items():
            s.put("r_t_" + tag, t)
            s.eval(f"(set quotes_{tag} (table [s t bid q] (list r_s r_t_{tag} r_bid r_q)))")
        s.eval(f'(set gaj (loadfn "{LIB}" "rfx_asof_join" 3))')
        s.eval(f'(set gbin (loadfn "{LIB}" "rfx_bin" 2))')
        s.eval(f'(set gbinr (loadfn "{LIB}" "rfx_binr" 2))')
        s.eval(f'(set gstat (loadfn "{LIB}" "rfx_stats" 1))')
        outs = []
        for tag in tables:
            for left, cols in (("trades", ("s", "t", "px", "q", "bid")), ("trades2", ("s", "t", "px", "q"))):
                name = f"{left}_{tag}"
                s.eval(f"(set g_{name} (gaj [s t] {left} quotes_{tag}))")
                s.eval(f"(set r_{name} (asof-join [s t] {left} quotes_{tag}))")
                for c in cols:
                    s.out(f"g_{name}_{c}", f"(at g_{name} '{c})")
                    s.out(f"r_{name}_{c}", f"(at r_{name} '{c})")
                    outs.append(f"{name}_{c}")
            for verb in ("bin", "binr"):
                s.out(f"g_{verb}_{tag}", f"(g{verb} r_t_{tag} l_t)")
                s.out(f"r_{verb}_{tag}", f"({verb} r_t_{tag} l_t)")
                outs.append(f"{verb}_{tag}")
        s.out("stats", "(gstat 0)")
        res = s.run(threads=8)
    for name in outs:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape == (N,), name
        assert np.array_equal(g.view(np.int64), r.view(np.int64)), name
    # the shuffled table is answered differently from the sorted one (the probe sequence, not the greatest time), by both alike
    assert not np.array_equal(res["g_trades_sorted_bid"].view(np.int64), res["g_trades_shuffled_bid"].view(np.int64))
    assert res["stats"][2] == 4 and res["stats"][3] == 0  # joins on the GPU, joins delegated
