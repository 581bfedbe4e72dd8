"""Drop-in proof for the sort verbs over narrow keys: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader
and answers iasc / asc / rank over a DATE and a U8 column twice in ONE process -- by the plugin and by its own built-ins.  Equality of bits, type code
and attribute byte."""
import os
import struct

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
VERBS = ("iasc", "asc", "rank")
DTYPES = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}


def read_file(path):
    """(oracle/ref.py's read_col knows no U8 payloads)"""
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        return np.frombuffer(f.read(), DTYPES[tp], n).copy(), tp, attrs


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_narrow_sort_verbs_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 100_003
    d = (rfo.gen_i64(n, 8, 40000) - 20000).astype(np.int32)
    d[::89] = -(2**31)  # nulls: first ascending
    with ref.Session() as s:
        s.put("d", d, tp=7)
        s.put("v", rfo.gen_i64(n, 4, 2**40) - 2**39)
        s.eval("(set u (as 'U8 v))")  # a U8 vector cannot travel as a column file
        for verb in VERBS:
            s.eval(f'(set g{verb} (loadfn "{LIB}" "rfx_{verb}" 1))')
        for c in ("d", "u"):
            for verb in VERBS:
                s.eval(f'(set "{os.path.join(s.dir, f"out_g_{verb}_{c}")}" (g{verb} {c}))')
                s.eval(f'(set "{os.path.join(s.dir, f"out_r_{verb}_{c}")}" ({verb} {c}))')
        s.run(threads=8)
        for c, tp in (("d", 7), ("u", 2)):
            for verb in VERBS:
                g, r = read_file(os.path.join(s.dir, f"out_g_{verb}_{c}")), read_file(os.path.join(s.dir, f"out_r_{verb}_{c}"))
                assert g[1:] == r[1:] and g[0].shape == r[0].shape == (n,), (verb, c, g[1:], r[1:], g[0].shape, r[0].shape)
                assert g[1] == (tp if verb == "asc" else 5), (verb, c, g[1])
                assert g[0].tobytes() == r[0].tobytes(), (verb, c, np.flatnonzero(g[0] != r[0])[:5])
