"""The numpy restatement of `last` and `dev` (tests/lastdev_ref.py) against the compiled reference's own answers (tests/golden/lastdev_golden.npz, written by
tests/golden/make_lastdev_golden.py from aggr_last / aggr_dev / ray_last / ray_dev): last bit for bit, dev within the bounds of a 1e-9 relative f64 sum.
And the library's surface: the new entry points are declared, exported, and `dev` has a function object."""
import ctypes as C
import os
import re

import numpy as np

import lastdev_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
Z = np.load(os.path.join(HERE, "golden", "lastdev_golden.npz"))


def selected(z, p, itype, shift, filt):
    """the selected rows' values and group ids in row order, as the index says them"""
    vals, ix = z[p + "vals"], z[p + "ix"]
    rows = z[p + "filter"] if filt else np.arange(len(vals))
    gids = ix if itype == 0 else ix[z[p + "keys"][rows] - shift]
    return vals[rows], gids.astype(np.int64)


def test_grouped_goldens():
    assert len(Z["group_cases"]) == 12
    for ci in range(len(Z["group_cases"])):
        _, vt, itype, groups, shift, filt = (int(x) for x in Z["group_cases"][ci])
        p = f"g{ci}_"
        v, g = selected(Z, p, itype, shift, filt)
        assert R.same_bits(R.group_last(v, g, groups), Z[p + "last"]), ci
        got = R.group_dev(v, g, groups)
        assert R.group_dev_close(got, Z[p + "dev"], v, g, groups) is None, (ci, R.group_dev_close(got, Z[p + "dev"], v, g, groups))


def test_the_shapes_the_goldens_must_hold():
    """a one-row group, an all-null group, a group whose last row is null, one whose only value is its first row, an all-equal group, +-inf and subnormals"""
    _, vt, itype, groups, shift, filt = (int(x) for x in Z["group_cases"][0])
    v, g = selected(Z, "g0_", itype, shift, filt)
    n = np.bincount(g, minlength=groups)
    nn = np.bincount(g[~R.is_null(v)], minlength=groups)
    rows = R.group_last_rows(v, g, groups)
    lastrow = np.zeros(groups, np.int64)
    lastrow[g] = np.arange(len(g))
    firstrow = np.full(groups, len(g), np.int64)
    np.minimum.at(firstrow, g, np.arange(len(g)))
    assert (n == 1).any() and ((n > 1) & (nn == 0)).any() and ((rows >= 0) & (rows < lastrow)).any() and ((n > 1) & (nn == 1) & (rows == firstrow)).any()
    assert (Z["g0_dev"][n > 1] == 0.0).any()
    f = Z["g2_vals"]
    assert np.isinf(f).any() and (np.abs(f[np.isfinite(f) & (f != 0)]) < 2.3e-308).any() and np.signbit(f[f == 0]).any()


def test_the_reference_with_8_executors_differs_at_40_000_rows():
    """the evidence for DESIGN.md section 4: AGGR_COLLECT keeps the first chunk that has a value"""
    vt, itype, groups, shift = (int(x) for x in Z["big_meta"])
    keys, vals, ix = Z["big_keys"], Z["big_vals"], Z["big_ix"]
    g = ix if itype == 0 else ix[keys - shift]
    assert R.same_bits(R.group_last(vals, g.astype(np.int64), groups), Z["big_last"])
    assert int(Z["big_last_differs_c8"]) == 1
    assert not np.array_equal(Z["big_last"], Z["big_last_c8"])


def test_scalar_goldens():
    for si in range(int(Z["scalar_cases"])):
        v = Z[f"s{si}_vals"]
        assert R.same_bits(np.asarray(R.last(v)), Z[f"s{si}_last"][0]), (si, v[-3:])
        assert R.dev_close(R.dev(v), float(Z[f"s{si}_dev"][0]), v), (si, R.dev(v), Z[f"s{si}_dev"][0])


def test_new_symbols_are_declared_and_exported(built):
    from rayforce_amd import _lib as L
    hdr = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("rfx_ops.h", "rfx_exec.h", "rfx_hip.h")}
    lib = C.CDLL(L.library_path()) if hasattr(L, "library_path") else C.CDLL(os.path.join(ROOT, "rayforce_amd", "librfx.so"))
    for name, h in (("rfx_last", "rfx_ops.h"), ("rfx_dev", "rfx_ops.h"), ("rfx_exec_dev", "rfx_exec.h"), ("rfx_exec_group_dev", "rfx_exec.h"),
                    ("rfx_hip_last_rows", "rfx_hip.h"), ("rfx_hip_last_gather", "rfx_hip.h"), ("rfx_hip_dev_derive", "rfx_hip.h"),
                    ("rfx_hip_dev_finalise", "rfx_hip.h"), ("rfx_hip_dev", "rfx_hip.h")):
        assert re.search(r"\b" + name + r"\s*\(", hdr[h]), name
        assert getattr(lib, name) is not None, name
    assert "RFX_AGG_LAST = 6" in hdr["rfx_hip.h"] and L.RFX_AGG_LAST == 6 and L.AGGS["last"] == 6


def test_dev_and_last_have_function_objects(built):
    from rayforce_amd import hostobj as H
    o = H.lib()
    o.rfx_host_fn.restype = C.c_void_p
    o.rfx_host_fn.argtypes = [C.c_char_p]
    dev, last, med = o.rfx_host_fn(b"dev"), o.rfx_host_fn(b"last"), o.rfx_host_fn(b"med")
    assert dev and last and med
    fn = lambda p: C.c_int64.from_address(p + 8).value
    assert fn(dev) == C.cast(o.rfx_dev, C.c_void_p).value and fn(last) == C.cast(o.rfx_last, C.c_void_p).value
    assert len({fn(dev), fn(last), fn(med)}) == 3
