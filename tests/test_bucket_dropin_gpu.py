"""Drop-in proof for the bucket verbs: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and answers
xrank / xbar / within / floor / ceil / round / neg over the same table twice in ONE process -- by the plugin and by its own built-ins.  Equality of bits."""
import os

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
ARITY = {"xrank": 2, "xbar": 2, "within": 2, "floor": 1, "ceil": 1, "round": 1, "neg": 1}
CALLS = (("xrank_v", "xrank v 10"), ("xrank_p", "xrank p 4"), ("xrank_sorted", "xrank sv 7"), ("xbar_ts", "xbar ts 5000"), ("xbar_p", "xbar p 0.25"),
         ("xbar_d", "xbar d 7"), ("xbar_a_v", "xbar a w"), ("within_a", "within a [10 500]"), ("floor_p", "floor p"), ("ceil_p", "ceil p"), ("round_p", "round p"),
         ("neg_a", "neg a"), ("neg_p", "neg p"), ("neg_i", "neg i"), ("xbar_p_7", "xbar p 7"), ("xbar_p_07", "xbar p 0.7"), ("xbar_a_07", "xbar a 0.7"))
# f64 cells by an atom whose reciprocal is inexact, at lengths that cross the reference's chunk edges and leave a vector remainder: the cells are
# multiples of the atom, give or take an ulp, where a true division and a product with the reciprocal floor to different integers
INEXACT = (4097, 20011, 2**20 + 5)
CALLS += tuple((f"xbar_q{n}_{k}", f"xbar q{'abc'[i]}{k} {y}") for i, n in enumerate(INEXACT) for k, y in (("s", "7"), ("t", "0.7")))


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_bucket_verbs_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 100_003
    p = (rfo.gen_f64(n, 5) - 0.5) * 1000.0
    p[::97] = np.nan
    p[1::97] = -0.0
    p[2::97] = 0.5
    a = rfo.gen_i64(n, 2, 1000) - 200
    a[::89] = -(2**63)
    w = rfo.gen_i64(n, 3, 19) - 9  # divisors: zero and negative widths among them
    with ref.Session() as s:
        s.put("v", rfo.gen_i64(n, 4, 5000))
        s.put("ts", rfo.gen_i64(n, 7, 10**12), tp=9)
        s.put("p", p)
        s.put("a", a)
        s.put("w", w)
        s.put("d", (rfo.gen_i64(n, 8, 40000) - 20000).astype(np.int32), tp=7)
        s.put("i", (rfo.gen_i64(n, 9, 40000) - 20000).astype(np.int32), tp=4)
        rng = np.random.default_rng(5)
        for i, m in enumerate(INEXACT):
            for k, y in (("s", 7.0), ("t", 0.7)):
                c = rng.integers(-(2**40), 2**40, 200_000).astype(np.float64) * y
                c = np.concatenate([c, np.nextafter(c, np.inf), np.nextafter(c, -np.inf)])
                pick = c[np.floor(c / y) != np.floor(c * (1.0 / y))][:700]  # the two divisions floor to different integers
                assert pick.size == 700
                q = np.resize(rng.permutation(np.concatenate([pick, c[:90], np.full(7, np.nan)])), m)
                s.put(f"q{'abc'[i]}{k}", q)
        s.eval("(set sv (asc v))")  # carries ATTR_ASC: both sides answer from the attribute
        for verb, arity in ARITY.items():
            s.eval(f'(set g{verb} (loadfn "{LIB}" "rfx_{verb}" {arity}))')
        for name, call in CALLS:
            s.out(f"g_{name}", f"(g{call})")
            s.out(f"r_{name}", f"({call})")
        res = s.run(threads=8)
    for name, _ in CALLS:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, r.dtype, g.shape, r.shape)
        assert g.tobytes() == r.tobytes(), (name, np.flatnonzero(g.view(np.uint8) != r.view(np.uint8))[:5])
    assert len(res["g_xrank_v"]) == n and res["g_within_a"].dtype == np.int8 and res["g_xbar_d"].dtype == np.int32
