"""Drop-in proof for the set verbs: the REAL RayforceDB binary (oracle/_ref/rayforce, a pool of 8) loads rfx_distinct / rfx_find / rfx_in / rfx_sect /
rfx_except / rfx_union from librfx.so through its own plugin loader and answers the same objects twice in ONE process -- by the plugin and by its
own built-ins -- over I64 columns on the dense and on the hash route and over a SYMBOL column.  Equality of bits, order included, and
rfx_set_stats -- loaded like the verbs -- counts every one of the plugin's calls as answered by the device, none handed to the host; a SYMBOL answer
is compared as the rows of its source that hold its cells (writing a symbol vector to a file would store strings)."""
import os

import numpy as np
import pytest

from oracle import ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
N = 300_000
VERBS = ("distinct", "find", "in", "sect", "except", "union")


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (needs /root/reference at build time)")
def test_set_verbs_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(77)
    pool = rng.integers(0, 10**12, 60_000)
    pool[0], pool[1] = 0, 10**12
    cols = {"dense": (rng.integers(-500, 90_000, N), rng.integers(40_000, 140_000, N // 3)),
            "hash": (np.concatenate([pool[:2], pool[rng.integers(0, 40_000, N - 2)]]), np.concatenate([pool[:2], pool[rng.integers(20_000, 60_000, N // 3)]]))}
    nsym = 200
    with ref.Session() as s:
        s.put("si", rng.integers(0, nsym, N))
        s.put("sj", rng.integers(nsym // 2, nsym + nsym // 2, N // 3))
        s.eval(f"(set SY (map (fn [i] (as 'symbol (format \"s%\" i))) (til {2 * nsym})))")
        s.eval("(set x_sym (at SY si))")
        s.eval("(set y_sym (at SY sj))")
        for tag, (x, y) in cols.items():
            s.put("x_" + tag, x)
            s.put("y_" + tag, y)
        for v in VERBS:
            s.eval(f'(set g{v} (loadfn "{LIB}" "rfx_{v}" {1 if v == "distinct" else 2}))')
        s.eval(f'(set gstat (loadfn "{LIB}" "rfx_set_stats" 1))')
        s.out("stats0", "(gstat 0)")
        outs = []
        for tag in ("dense", "hash", "sym"):
            s.eval(f"(set c_{tag} (concat x_{tag} y_{tag}))")
            for v in VERBS:
                args = f"x_{tag}" if v == "distinct" else f"x_{tag} y_{tag}"
                for who, fn in (("g", "g" + v), ("r", v)):
                    e = f"({fn} {args})"
                    if tag == "sym" and v not in ("in", "find"):
                        e = f"(find {'c_sym' if v == 'union' else 'x_sym'} {e})"
                    s.out(f"{who}_{v}_{tag}", e)
                outs.append(f"{v}_{tag}")
        s.out("stats", "(gstat 0)")
        res = s.run(threads=8)
    for name in outs:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert np.array_equal(g, r), name
    assert res["g_distinct_hash"].size > 30_000 and not np.array_equal(res["g_distinct_hash"], np.sort(res["g_distinct_hash"]))  # (slot order, not sorted)
    assert np.array_equal(res["g_distinct_dense"], np.sort(res["g_distinct_dense"]))
    # rfx_set_stats: [answered by the device path, handed to the host, then the answered calls by route: none, dense, hash, disjoint, atom].
    # Inside the binary a host IS bound, so a declined call would be answered by ray_* and equal trivially: all 18 plugin calls are the device's.
    st = res["stats"] - res["stats0"]
    print("set stats", st.tolist())
    assert st[0] == 3 * len(VERBS) and st[1] == 0, st
    assert st[3] >= len(VERBS) and st[4] >= len(VERBS) and st[3] + st[4] == st[0], st  # (the I64 tags' routes are known; the symbol ids are the reference's)
