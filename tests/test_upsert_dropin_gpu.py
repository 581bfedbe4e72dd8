"""Drop-in proof for upsert and insert: the REAL RayforceDB binary (oracle/_ref/rayforce) loads librfx.so through its own plugin loader and maintains the
same keyed table twice in ONE process -- by the plugin's rfx_upsert / rfx_insert and by its own verbs.  Equality of bits, type code and attribute byte;
(set t (upsert t 1 batch)) followed by a select gives the host's own answer and uploads nothing -- the answer came from the device and stayed there (a
table the host had answered would have to be uploaded); the quoted-symbol form is answered by the host in place and later selects see the new cells."""
import os
import struct

import numpy as np
import pytest

from oracle import ref, rfo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rayforce_amd", "librfx.so")
DTYPES = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 6: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}
COLS = ("k", "g", "v", "ts", "w")


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        return np.frombuffer(f.read(), DTYPES[tp], n).copy(), tp, attrs


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/rayforce not built (the reference's sources were not there at build time)")
def test_upsert_and_insert_inside_the_real_reference(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, nb = 100_003, 1_003

    def cols(rows, seed, keys):
        v = (rfo.gen_f64(rows, seed) - 0.5) * 1000.0
        v[::97] = np.nan
        return dict(k=keys, g=rfo.gen_i64(rows, seed + 2, 1000), v=v, ts=rfo.gen_i64(rows, seed + 4, 10**12), w=rfo.gen_i64(rows, seed + 5, 2**40))

    types = dict(k=5, g=5, v=10, ts=9, w=5)
    bk = rfo.gen_i64(nb, 17, 6 * n)  # about half of them multiples of 3: matched; some twice
    bk[-1] = bk[3] = 3 * 77
    with ref.Session() as s:
        for name, a in cols(n, 3, np.arange(n, dtype=np.int64) * 3).items():
            s.put(name, a, tp=types[name])
        for name, a in cols(nb, 11, bk).items():
            s.put(name + "b", a, tp=types[name])
        s.eval("(set t (table [k g v ts w] (list k g v ts w)))")
        s.eval("(set b (table [w ts g v k] (list wb tsb gb vb kb)))")  # the batch's columns in another order
        s.eval("(set bl (list kb gb vb))")                             # a short LIST: ts and w append nulls, their matched rows stay
        s.eval(f'(set gupsert (loadfn "{LIB}" "rfx_upsert" 3))')
        s.eval(f'(set ginsert (loadfn "{LIB}" "rfx_insert" 3))')
        s.eval(f'(set gsel (loadfn "{LIB}" "rfx_select" 1))')
        s.eval(f'(set gstats (loadfn "{LIB}" "rfx_stats" 1))')
        out = lambda name, expr: s.eval(f'(set "{os.path.join(s.dir, "out_" + name)}" {expr})')  # noqa: E731
        s.eval("(set gt t)")
        s.eval("(set rt t)")
        s.eval("(set gt (gupsert gt 1 b))")
        s.eval("(set rt (upsert rt 1 b))")
        out("stats0", "(gstats 0)")
        s.eval("(set ga (gsel {s: (sum w) c: (count v) from: gt by: g}))")
        out("stats1", "(gstats 0)")
        s.eval("(set ra (select {s: (sum w) c: (count v) from: rt by: g}))")
        s.eval("(set gl (gupsert t 1 bl))")
        s.eval("(set rl (upsert t 1 bl))")
        s.eval("(set gi (ginsert t b))")
        s.eval("(set ri (insert t b))")
        # the quoted-symbol form: the host's own verb, in place on the global; the plugin's select over it afterwards sees the new cells
        s.eval("(set q t)")
        s.eval("(set gq0 (gsel {s: (sum w) from: q by: g}))")  # (q's columns are resident now)
        s.eval("(gupsert 'q 1 b)")
        s.eval("(set gq (gsel {s: (sum w) c: (count v) from: q by: g}))")
        for c in COLS:
            for tag in ("t", "l", "i"):
                out(f"g_{tag}_{c}", f"(at g{tag} '{c})")
                out(f"r_{tag}_{c}", f"(at r{tag} '{c})")
            out(f"g_q_{c}", f"(at q '{c})")
            out(f"r_q_{c}", f"(at rt '{c})")
        for c in ("g", "s", "c"):
            out(f"g_a_{c}", f"(at ga '{c})")
            out(f"r_a_{c}", f"(at ra '{c})")
            out(f"g_qa_{c}", f"(at gq '{c})")
            out(f"r_qa_{c}", f"(at ra '{c})")
        ref.run_script("\n".join(s.lines) + "\n", threads=8)
        names = [f"{tag}_{c}" for tag in ("t", "l", "i", "q") for c in COLS] + [f"{tag}_{c}" for tag in ("a", "qa") for c in ("g", "s", "c")]
        for name in names:
            g, r = read_file(os.path.join(s.dir, "out_g_" + name)), read_file(os.path.join(s.dir, "out_r_" + name))
            assert g[1:] == r[1:] and g[0].shape == r[0].shape, (name, g[1:], r[1:], g[0].shape, r[0].shape)
            assert g[0].tobytes() == r[0].tobytes(), (name, np.flatnonzero(g[0].view(np.uint8) != r[0].view(np.uint8))[:5])
        matched = int(np.sum((bk % 3 == 0) & (bk < 3 * n)))
        assert 0 < matched < nb and len(read_file(os.path.join(s.dir, "out_g_t_k"))[0]) == n + nb - matched
        assert len(read_file(os.path.join(s.dir, "out_g_i_k"))[0]) == n + nb
        s0, s1 = read_file(os.path.join(s.dir, "out_stats0"))[0], read_file(os.path.join(s.dir, "out_stats1"))[0]
        assert s1[0] - s0[0] == 1, "the select over the upserted table ran on the device"
        assert s1[4] - s0[4] == 0, "... and uploaded nothing: the upsert was the device's and its columns were resident"
