"""Drop-in proof for the sort verbs: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and answers
iasc / idesc / asc / desc / rank / xasc / xdesc over the same objects twice in ONE process -- by the plugin and by its own built-ins.  Equality of bits."""
import os

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
UNARY = ("iasc", "idesc", "asc", "desc", "rank")
TABLE_KEYS = (("k", "'k"), ("v", "'v"), ("kv", "[k v]"), ("k1ka", "[k1 k a]"))


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (needs /root/reference at build time)")
def test_sort_verbs_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 100_003
    v = rfo.gen_f64(n, 5)
    v[::97] = np.nan
    v[1::97] = -0.0
    cols = {"k": rfo.gen_i64(n, 4, 5000), "a": rfo.gen_i64(n, 2, 1_000_000) - 500_000, "v": v, "k1": rfo.gen_i64(n, 14, 7)}
    with ref.Session() as s:
        s.table("t", cols)
        for verb in UNARY:
            s.eval(f'(set g{verb} (loadfn "{LIB}" "rfx_{verb}" 1))')
        s.eval(f'(set gxasc (loadfn "{LIB}" "rfx_xasc" 2))')
        s.eval(f'(set gxdesc (loadfn "{LIB}" "rfx_xdesc" 2))')
        for c in ("a", "v"):
            for verb in UNARY:
                s.out(f"g_{verb}_{c}", f"(g{verb} (at t '{c}))")
                s.out(f"r_{verb}_{c}", f"({verb} (at t '{c}))")
        # a vector the reference itself marked ATTR_ASC (the result of its own asc): both sides answer from the attribute
        s.eval("(set sa (asc (at t 'a)))")
        for verb in UNARY:
            s.out(f"g_{verb}_sa", f"(g{verb} sa)")
            s.out(f"r_{verb}_sa", f"({verb} sa)")
        for tag, keys in TABLE_KEYS:
            for verb in ("xasc", "xdesc"):
                s.eval(f"(set g_{verb}_{tag} (g{verb} t {keys}))")
                s.eval(f"(set r_{verb}_{tag} ({verb} t {keys}))")
                for c in cols:
                    s.out(f"g_{verb}_{tag}_{c}", f"(at g_{verb}_{tag} '{c})")
                    s.out(f"r_{verb}_{tag}_{c}", f"(at r_{verb}_{tag} '{c})")
        res = s.run(threads=8)
    names = [f"{verb}_{c}" for c in ("a", "v", "sa") for verb in UNARY] + [f"{verb}_{tag}_{c}" for tag, _ in TABLE_KEYS for verb in ("xasc", "xdesc") for c in cols]
    for name in names:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert np.array_equal(g.view(np.int64), r.view(np.int64)), name
    assert len(res["g_iasc_a"]) == n
