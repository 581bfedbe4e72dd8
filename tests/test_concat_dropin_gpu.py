"""Drop-in proof for concat and raze: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and appends the same
table, razes the same list and concatenates the same vectors twice in ONE process -- by the plugin's rfx_concat / rfx_raze and by its own verbs.  Equality
of bits, type code and attribute byte; a shape the device does not take (operands of two types) comes back as the host's own answer; and the plugin's
counters show that the select over the appended table uploaded nothing."""
import os
import struct

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
DTYPES = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 6: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}
VECTORS = (("vv_i64", "k kb"), ("vv_f64", "v vb"), ("vv_date", "d db"), ("vv_b8", "m mb"), ("va_i64", "k (first kb)"), ("av_f64", "(first vb) v"),
           ("vv_empty", "(take k [0 0]) kb"), ("raze3", None), ("raze_date", None))
COLS = ("k", "v", "d", "m", "ts", "w")


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        return np.frombuffer(f.read(), DTYPES[tp], n).copy(), tp, attrs


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_concat_and_raze_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, nb = 100_003, 1_003

    def cols(rows, seed):
        v = (rfo.gen_f64(rows, seed) - 0.5) * 1000.0
        v[::97] = np.nan
        d = (rfo.gen_i64(rows, seed + 1, 40000) - 20000).astype(np.int32)
        d[::89] = -(2**31)
        return dict(k=rfo.gen_i64(rows, seed + 2, 1000), v=v, d=d, m=(rfo.gen_i64(rows, seed + 3, 10) < 3).astype(np.int8), ts=rfo.gen_i64(rows, seed + 4, 10**12),
                    w=rfo.gen_i64(rows, seed + 5, 2**40))

    types = dict(k=5, v=10, d=7, m=1, ts=9, w=5)
    with ref.Session() as s:
        for name, a in cols(n, 3).items():
            s.put(name, a, tp=types[name])
        for name, a in cols(nb, 11).items():
            s.put(name + "b", a, tp=types[name])
        s.eval("(set t (table [k v d m ts w] (list k v d m ts w)))")
        s.eval("(set b (table [w ts m d v k] (list wb tsb mb db vb kb)))")  # the batch's columns in another order
        s.eval(f'(set gconcat (loadfn "{LIB}" "rfx_concat" 2))')
        s.eval(f'(set graze (loadfn "{LIB}" "rfx_raze" 1))')
        s.eval(f'(set gsel (loadfn "{LIB}" "rfx_select" 1))')
        s.eval(f'(set gstats (loadfn "{LIB}" "rfx_stats" 1))')
        out = lambda name, expr: s.eval(f'(set "{os.path.join(s.dir, "out_" + name)}" {expr})')  # noqa: E731
        s.eval("(set gt (gconcat t b))")
        s.eval("(set rt (concat t b))")
        out("stats0", "(gstats 0)")
        s.eval("(set ga (gsel {s: (sum w) from: gt by: k}))")
        out("stats1", "(gstats 0)")
        s.eval("(set ra (select {s: (sum w) from: rt by: k}))")
        for c in COLS:
            out(f"g_t_{c}", f"(at gt '{c})")
            out(f"r_t_{c}", f"(at rt '{c})")
        for c in ("k", "s"):
            out(f"g_a_{c}", f"(at ga '{c})")
            out(f"r_a_{c}", f"(at ra '{c})")
        for name, call in VECTORS:
            if call:
                out(f"g_{name}", f"(gconcat {call})")
                out(f"r_{name}", f"(concat {call})")
        out("g_raze3", "(graze (list k (take k [0 0]) kb k))")
        out("r_raze3", "(raze (list k (take k [0 0]) kb k))")
        out("g_raze_date", "(graze (list db d))")
        out("r_raze_date", "(raze (list db d))")
        # a shape handed to the host: operands of two types -- the reference answers a LIST of the two; both sides must say the same
        out("g_host", "(enlist (count (gconcat k v)))")
        out("r_host", "(enlist (count (concat k v)))")
        out("host_type", "(enlist (== (type (gconcat k v)) (type (concat k v))))")
        ref.run_script("\n".join(s.lines) + "\n", threads=8)
        names = [f"t_{c}" for c in COLS] + ["a_k", "a_s"] + [nm for nm, _ in VECTORS] + ["host"]
        for name in names:
            g, r = read_file(os.path.join(s.dir, "out_g_" + name)), read_file(os.path.join(s.dir, "out_r_" + name))
            assert g[1:] == r[1:] and g[0].shape == r[0].shape, (name, g[1:], r[1:], g[0].shape, r[0].shape)
            assert g[0].tobytes() == r[0].tobytes(), (name, np.flatnonzero(g[0].view(np.uint8) != r[0].view(np.uint8))[:5])
        assert len(read_file(os.path.join(s.dir, "out_g_t_k"))[0]) == n + nb and len(read_file(os.path.join(s.dir, "out_g_raze3"))[0]) == 2 * n + nb
        assert read_file(os.path.join(s.dir, "out_host_type"))[0].tolist() == [1]
        s0, s1 = read_file(os.path.join(s.dir, "out_stats0"))[0], read_file(os.path.join(s.dir, "out_stats1"))[0]
        assert s1[0] - s0[0] == 1, "the select over the appended table ran on the device"
        assert s1[4] - s0[4] == 0, "... and uploaded nothing: the appended columns were resident"
