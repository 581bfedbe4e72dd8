"""Drop-in proof for the nested columns of select ... by:: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader
and answers the same three queries twice in ONE process -- by the plugin's rfx_select and by its own select: a collected column beside an aggregate, (row
column), and both beside a count under where:.  A LIST column is compared as its razed cells and the lengths of its items; equality of bits, type code and
attribute byte, the key and aggregate columns included (so the group order too); rfx_stats says the three answers came from the device."""
import os
import struct

import numpy as np
import pytest

import collect_ref as R
from oracle import ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
DTYPES = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 6: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}
QUERIES = {"q1": ("{p: price q: (sum qty) by: sym from: trades}", ("sym", "q"), ("p",)),
           "q2": ("{r: (row price) by: sym from: trades}", ("sym",), ("r",)),
           "q3": ("{p: price r: (row price) c: (count qty) by: sym from: trades where: (< a 37)}", ("sym", "c"), ("p", "r"))}


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        return np.frombuffer(f.read(), DTYPES[tp], n).copy(), tp, attrs


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_nested_select_columns_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, groups = 100_003, 1000  # (a thousand dense keys: the reference's own group order does not depend on its pool there)
    sym = R.key_column(n, groups, base=500)
    a = R.value_column("i64", n, 9) % 100
    price, qty = R.value_column("f64", n, 4), R.value_column("i64", n, 5) % 1000
    with ref.Session() as s:
        for name, col in dict(sym=sym, price=price, qty=qty, a=a).items():
            s.put(name, col)
        s.eval("(set trades (table [sym price qty a] (list sym price qty a)))")
        s.eval(f'(set gsel (loadfn "{LIB}" "rfx_select" 1))')
        s.eval(f'(set gstats (loadfn "{LIB}" "rfx_stats" 1))')
        out = lambda name, expr: s.eval(f'(set "{os.path.join(s.dir, "out_" + name)}" {expr})')  # noqa: E731
        out("stats0", "(gstats 0)")
        names = []
        for q, (text, plain, nested) in QUERIES.items():
            s.eval(f"(set g_{q} (gsel {text}))")
            s.eval(f"(set r_{q} (select {text}))")
            for side in "gr":
                for c in plain:
                    out(f"{side}_{q}_{c}", f"(at {side}_{q} '{c})")
                for c in nested:
                    out(f"{side}_{q}_{c}", f"(raze (at {side}_{q} '{c}))")
                    out(f"{side}_{q}_{c}_len", f"(map count (at {side}_{q} '{c}))")
            names += [f"{q}_{c}" for c in plain] + [f"{q}_{c}{x}" for c in nested for x in ("", "_len")]
        out("stats1", "(gstats 0)")
        ref.run_script("\n".join(s.lines) + "\n", threads=8)
        for name in names:
            g, r = read_file(os.path.join(s.dir, "out_g_" + name)), read_file(os.path.join(s.dir, "out_r_" + name))
            assert g[1:] == r[1:] and g[0].shape == r[0].shape, (name, g[1:], r[1:], g[0].shape, r[0].shape)
            assert g[0].tobytes() == r[0].tobytes(), (name, np.flatnonzero(g[0].view(np.uint8) != r[0].view(np.uint8))[:5])
        # ... and both are the restatement's answer
        keys, offsets, (cells,), rows = R.group_collect(sym, [price], a < 37)
        assert np.array_equal(read_file(os.path.join(s.dir, "out_g_q3_sym"))[0], keys) and np.array_equal(read_file(os.path.join(s.dir, "out_g_q3_r"))[0], rows)
        assert read_file(os.path.join(s.dir, "out_g_q3_p"))[0].tobytes() == cells.tobytes()
        assert np.array_equal(read_file(os.path.join(s.dir, "out_g_q3_p_len"))[0], np.diff(offsets))
        s0, s1 = read_file(os.path.join(s.dir, "out_stats0"))[0], read_file(os.path.join(s.dir, "out_stats1"))[0]
        assert s1[0] - s0[0] == 3 and s1[1] - s0[1] == 0, "the three selects ran on the device, none was handed back"
