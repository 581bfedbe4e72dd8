"""Drop-in proof for `as`: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and casts the same vectors twice
in ONE process -- by the plugin's rfx_as and by its own `as`.  Equality of bits, type code and attribute byte; and the error both give for B8 -> U8."""
import os
import struct

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
CALLS = (("f64_v", "'F64 v"), ("i32_v", "'I32 v"), ("u8_f", "'U8 f"), ("i64_f", "'i64 f"), ("i16_v", "'I16 v"), ("ts_d", "'TIMESTAMP d"), ("date_ts", "'date ts"),
         ("f64_b", "'F64 b"), ("i64_h", "'I64 h"), ("b8_v", "'B8 v"), ("same_v", "'I64 sv"), ("f64_sv", "'F64 sv"), ("empty", "'U8 eb"))
DTYPES = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}


def read_file(path):
    """(oracle/ref.py's read_col knows no U8 / I16 payloads)"""
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        return np.frombuffer(f.read(), DTYPES[tp], n).copy(), tp, attrs


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_as_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 100_003
    v = rfo.gen_i64(n, 4, 2**40) - 2**39
    v[::89] = -(2**63)
    v[1::89] = 2**63 - 1
    f = (rfo.gen_f64(n, 5) - 0.5) * 1e5
    for k, cell in enumerate((np.nan, np.inf, -np.inf, 300.7, -1.9, 2147483648.0, -2147483649.0, 9.3e18, -9.3e18, 32768.0, 5e-324, -0.0)):
        f[k::97] = cell
    with ref.Session() as s:
        s.put("v", v)
        s.put("f", f)
        s.put("ts", rfo.gen_i64(n, 7, 10**15), tp=9)
        s.put("d", (rfo.gen_i64(n, 8, 40000) - 20000).astype(np.int32), tp=7)
        s.put("b", (rfo.gen_i64(n, 9, 256) - 128).astype(np.int8), tp=1)
        s.put("eb", np.empty(0, np.int8), tp=1)
        s.eval("(set h (as 'I16 v))")  # an I16 vector cannot travel as a column file
        s.eval("(set sv (asc v))")     # carries ATTR_ASC: the same type keeps it on both sides, a converted vector drops it
        s.eval(f'(set gas (loadfn "{LIB}" "rfx_as" 2))')
        for name, call in CALLS:
            s.eval(f'(set "{os.path.join(s.dir, "out_g_" + name)}" (gas {call}))')
            s.eval(f'(set "{os.path.join(s.dir, "out_r_" + name)}" (as {call}))')
        for fn in ("as", "gas"):  # B8 -> U8: the reference has no such arm; the plugin hands the call to the host's own verb, whose error comes back
            for name in ("'U8", "'u8"):
                s.eval('(println "cast-error:")')
                s.eval(f"(println (try ({fn} {name} b) (fn [e] e)))")
        res = s.run(threads=8)
        for name, _ in CALLS:
            g, r = read_file(os.path.join(s.dir, "out_g_" + name)), read_file(os.path.join(s.dir, "out_r_" + name))
            assert g[1:] == r[1:] and g[0].shape == r[0].shape, (name, g[1:], r[1:], g[0].shape, r[0].shape)
            assert g[0].tobytes() == r[0].tobytes(), (name, np.flatnonzero(g[0].view(np.uint8) != r[0].view(np.uint8))[:5])
        assert read_file(os.path.join(s.dir, "out_g_u8_f"))[1] == 2 and len(read_file(os.path.join(s.dir, "out_g_f64_v"))[0]) == n
        assert read_file(os.path.join(s.dir, "out_g_same_v"))[2] == 2 and read_file(os.path.join(s.dir, "out_g_f64_sv"))[2] == 0
    lines = res["_stdout"].splitlines()
    errors = [lines[i + 1].strip() for i, l in enumerate(lines) if l.strip() == "cast-error:" and i + 1 < len(lines)]
    assert len(errors) == 4 and errors[0] and len(set(errors)) == 1, errors
