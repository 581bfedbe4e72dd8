"""Drop-in proof for the row verbs: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and answers filter /
take / reverse over the same objects twice in ONE process -- by the plugin and by its own built-ins.  Equality of bits."""
import os

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
ARITY = {"filter": 2, "take": 2, "reverse": 1}
CALLS = (("filter_v", "filter v m"), ("filter_p", "filter p m"), ("filter_d", "filter d m"), ("filter_b", "filter m m"), ("filter_ts", "filter ts m"),
         ("take_v_head", "take v 1000"), ("take_v_tail", "take v -1000"), ("take_v_cyclic", "take v 250007"), ("take_d_cyclic", "take d -250007"),
         ("take_p_range", "take p [5 70001]"), ("take_p_range_end", "take p [-9 100]"), ("take_atom", "take 7 1000"), ("take_m", "take m -77"),
         ("reverse_v", "reverse v"), ("reverse_sv", "reverse sv"), ("reverse_d", "reverse d"), ("reverse_m", "reverse m"), ("reverse_p", "reverse p"))
# SYMBOL vectors and atoms cannot leave the reference as column files: plugin and built-in are compared inside it, cells (==) and type
SYMBOL_CALLS = (("sy_filter", "filter sy m", None), ("sy_head", "take sy 1000", 1000), ("sy_tail", "take sy -1000", 1000), ("sy_cyclic", "take sy -250007", 250007),
                ("sy_range", "take sy [5 70001]", 70001), ("sy_reverse", "reverse sy", 100_003), ("sy_atom", "take 'zz 1000", 1000), ("sy_atom_neg", "take 'zz -7", 7))
TABLE_CALLS = (("tfilter", "filter t m"), ("ttake", "take t -5000"), ("ttake_range", "take t [11 4097]"))


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_row_verbs_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 100_003
    p = (rfo.gen_f64(n, 5) - 0.5) * 1000.0
    p[::97] = np.nan
    d = (rfo.gen_i64(n, 8, 40000) - 20000).astype(np.int32)
    d[::89] = -(2**31)
    with ref.Session() as s:
        s.put("v", rfo.gen_i64(n, 4, 5000))
        s.put("ts", rfo.gen_i64(n, 7, 10**12), tp=9)
        s.put("p", p)
        s.put("d", d, tp=7)
        s.put("m", (rfo.gen_i64(n, 3, 10) < 3).astype(np.int8))
        s.eval(f"(set sy (take [aa bb cc dd ee ff gg] {n}))")
        s.eval("(set sv (asc v))")  # carries ATTR_ASC: the answer carries ATTR_DESC
        s.eval("(set t (table [v p d m ts v2] (list v p d m ts v)))")
        for verb, arity in ARITY.items():
            s.eval(f'(set g{verb} (loadfn "{LIB}" "rfx_{verb}" {arity}))')
        for name, call in CALLS:
            s.out(f"g_{name}", f"(g{call})")
            s.out(f"r_{name}", f"({call})")
        for name, call in TABLE_CALLS:
            s.eval(f"(set g_{name} (g{call}))")
            s.eval(f"(set r_{name} ({call}))")
            for c in ("v", "p", "d", "m", "ts", "v2"):
                s.out(f"g_{name}_{c}", f"(at g_{name} '{c})")
                s.out(f"r_{name}_{c}", f"(at r_{name} '{c})")
        for name, call, _ in SYMBOL_CALLS:
            s.out(f"eq_{name}", f"(== (g{call}) ({call}))")
            s.out(f"ty_{name}", f"(enlist (== (type (g{call})) (type ({call}))))")
        # the attribute of a reversed sorted vector, seen through a verb that trusts it
        s.out("g_attr", "(asc (greverse sv))")
        s.out("r_attr", "(asc (reverse sv))")
        res = s.run(threads=8)
    names = [nm for nm, _ in CALLS] + [f"{nm}_{c}" for nm, _ in TABLE_CALLS for c in ("v", "p", "d", "m", "ts", "v2")] + ["attr"]
    for name in names:
        g, r = res["g_" + name], res["r_" + name]
        assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, r.dtype, g.shape, r.shape)
        assert g.tobytes() == r.tobytes(), (name, np.flatnonzero(g.view(np.uint8) != r.view(np.uint8))[:5])
    for name, _, cells in SYMBOL_CALLS:
        assert res["eq_" + name].all() and res["ty_" + name].tolist() == [1], name
        assert cells is None or len(res["eq_" + name]) == cells, (name, len(res["eq_" + name]))
    assert 0 < len(res["eq_sy_filter"]) == len(res["g_filter_v"])
    assert len(res["g_take_v_cyclic"]) == 250007 and res["g_filter_d"].dtype == np.int32 and res["g_reverse_m"].dtype == np.int8
