"""`med` on the MI355X (rfx_median.hip): the flat kernels against the numpy restatement (tests/median_ref.py) bit for bit over every size class of
group, and the operator door -- rfx_select answers (med col) itself, scalar and under one by: column, and hands every other shape back."""
import ctypes as C

import numpy as np
import pytest
import torch

import median_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H

pytestmark = pytest.mark.gpu
T_MAPFILTER, T_MAPGROUP = 71, 72


def dev_median(eng, values, gids=None, groups=1, rule=R.GROUPED, preds=None, mask=None, key=None, table=None, kmin=0):
    lib = eng.lib
    v = torch.from_numpy(values).to(eng.device)
    rows = L.MedRows()
    keep = [v]
    if gids is not None:
        g = torch.from_numpy(gids).to(eng.device)
        keep.append(g)
        rows.d_gids = g.data_ptr()
    if key is not None:
        k, t = torch.from_numpy(key).to(eng.device), torch.from_numpy(table).to(eng.device)
        keep += [k, t]
        rows.d_key, rows.d_table, rows.kmin, rows.range = k.data_ptr(), t.data_ptr(), kmin, len(table)
    if mask is not None:
        m = torch.from_numpy(mask.astype(np.int8)).to(eng.device)
        keep.append(m)
        rows.d_mask = m.data_ptr()
    if preds is not None:
        rows.preds, rows.npred, rows.logic = C.cast(preds[0], C.c_void_p), preds[1], L.RFX_AND
    out = torch.empty(max(groups, 1), dtype=torch.float64, device=eng.device)
    torch.cuda.synchronize()
    vt = L.RFX_F64 if values.dtype == np.float64 else L.RFX_I64
    L.check(lib.rfx_hip_group_median(eng._ctx, C.byref(rows), C.c_void_p(v.data_ptr()), vt, len(values), groups, rule, C.c_void_p(out.data_ptr())), "group_median")
    return out.cpu().numpy()[:groups]


def values_of(rng, kind, n):
    if kind == "i64":
        return rng.integers(-(10**12), 10**12, n)
    if kind == "lowbits":  # equal in every digit but the last two: every radix digit is walked
        return (np.int64(0x1234_5678_9ABC_0000) + rng.integers(0, 1 << 16, n)).astype(np.int64)
    if kind == "extremes":
        return rng.choice(np.array([R.NULL_I64, 2**63 - 1, -(2**63) + 1, 0, -1, 1, 2**62], np.int64), n)
    v = rng.standard_normal(n)
    r = rng.integers(0, 40, n)
    v[r == 0], v[r == 1], v[r == 2], v[r == 3], v[r == 4] = np.nan, 0.0, -0.0, np.inf, -np.inf
    return v


def gids_of(rng, shape, n):
    if shape == "one":
        return np.zeros(n, np.int64), 1
    if shape == "many":
        g = min(1_000_000, max(n // 10, 1))
        return rng.integers(0, g, n), g
    if shape == "tiny":  # groups of one to three rows
        sizes = rng.integers(1, 4, n)
        ids = np.repeat(np.arange(n), sizes)[:n]
        return rng.permutation(ids).astype(np.int64), int(ids.max()) + 1
    if shape == "zipf":
        z = rng.zipf(1.3, n) - 1
        _, inv = np.unique(z, return_inverse=True)
        return inv.astype(np.int64), int(inv.max()) + 1
    if shape == "mix":  # one huge group, mid-size ones, tiny ones
        g = np.where(rng.random(n) < 0.4, 0, np.where(rng.random(n) < 0.5, 1 + rng.integers(0, max(n // 2000, 1), n), 0))
        tiny = g == 0
        tiny &= rng.random(n) < 0.3
        g[tiny] = 1 + max(n // 2000, 1) + rng.integers(0, max(n // 3, 1), tiny.sum())
        _, inv = np.unique(g, return_inverse=True)
        return inv.astype(np.int64), int(inv.max()) + 1
    raise ValueError(shape)


@pytest.mark.parametrize("n", [100_000, 3_000_000])
@pytest.mark.parametrize("shape", ["one", "many", "tiny", "zipf", "mix"])
@pytest.mark.parametrize("kind", ["i64", "lowbits", "extremes", "f64"])
def test_flat_kernel_equals_the_restatement(eng, n, shape, kind):
    rng = np.random.default_rng(hash((n, shape, kind)) & 0xFFFF)
    v = values_of(rng, kind, n)
    g, groups = gids_of(rng, shape, n)
    g[rng.random(n) < 0.01] = -1  # rows that do not count
    assert R.same_bits(dev_median(eng, v, g, groups), R.group_median(v, g, groups))


@pytest.mark.parametrize("kind", ["i64", "lowbits", "extremes"])
def test_scalar_rule_at_1e7(eng, kind):
    rng = np.random.default_rng(5)
    n = 10_000_000 + (kind == "extremes")
    v = values_of(rng, kind, n)
    got = dev_median(eng, v, rule=R.SCALAR)
    assert R.same_bits(got[0], R.median(v))


def test_one_group_of_1e8_rows(eng):
    n = 100_000_000
    v = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=eng.device)
    v[::7] = v[::7] & 0xFFFF  # many repeats in the low range
    s = torch.sort(v).values
    want = (float(s[(n - 1) // 2]) + float(s[n // 2])) / 2.0
    lib = eng.lib
    out = torch.empty(1, dtype=torch.float64, device=eng.device)
    torch.cuda.synchronize()
    rows = L.MedRows()
    L.check(lib.rfx_hip_group_median(eng._ctx, C.byref(rows), C.c_void_p(v.data_ptr()), L.RFX_I64, n, 1, R.GROUPED, C.c_void_p(out.data_ptr())), "group_median")
    assert float(out[0]) == want


def test_where_mask_and_key_table(eng):
    rng = np.random.default_rng(9)
    n = 2_000_000
    v = rng.standard_normal(n)
    key = rng.integers(100, 5100, n)
    mask = rng.random(n) < 0.5
    uk = np.unique(key)
    table = np.full(5000, R.NULL_I64, np.int64)
    table[uk - 100] = np.arange(len(uk))
    got = dev_median(eng, v, groups=len(uk), key=key, table=table, kmin=100, mask=mask)
    g = np.where(mask, table[key - 100], -1)
    assert R.same_bits(got, R.group_median(v, g, len(uk)))


# ---------------------------------------------------------------------------------------------------- the door
@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    o.rfx_host_bind()
    return o


def ask(ops, q, tab):
    d = H.select_dict(q, tab)
    r = ops.rfx_select(d)
    ops.rfx_host_drop(d)
    on_gpu = ops.rfx_last_select_on_gpu()
    if H.is_error(r):
        ops.rfx_host_drop(r)
        return None, on_gpu
    out = H.table_to_numpy(r)
    ops.rfx_host_drop(r)
    return out, on_gpu


def door_table(n=300_000, seed=3, keys=1000):
    rng = np.random.default_rng(seed)
    host = {"k": rng.integers(0, keys, n), "s": rng.integers(0, 2**40, n) * 1_000_003, "v": rng.integers(-1000, 1000, n),
            "f": rng.standard_normal(n), "a": rng.integers(0, 100, n)}
    host["v"][rng.random(n) < 0.02] = R.NULL_I64
    host["f"][rng.random(n) < 0.02] = np.nan
    return host


def test_scalar_med_through_the_door(ops):
    host = door_table()
    tab = H.table(host)
    got, on_gpu = ask(ops, {"m": ("med", "v"), "t": ("sum", "a"), "c": ("count", "v")}, tab)
    ops.rfx_host_drop(tab)
    assert on_gpu == 1, ops.rfx_ops_last_error()
    assert R.same_bits(got["m"][0], R.median(host["v"]))
    assert int(got["t"][0]) == int(host["a"].sum())


@pytest.mark.parametrize("q,why", [({"by": "k", "m": ("med", "v")}, "med under by:"),               # ray_med of a MAPGROUP pair: null there
                                   ({"where": ("<", "a", 50), "m": ("med", "v")}, "med under where:"),  # ... of a MAPFILTER pair: null there
                                   ({"m": ("med", "f")}, "med: column type"),                           # scalar f64: err_type in the reference
                                   ({"m": ("med", ("+", "v", "a"))}, "med of an expression")])
def test_shapes_the_reference_does_not_answer_with_a_median_go_to_the_host(ops, q, why):
    host = door_table(n=10_000)
    tab = H.table(host)
    _, on_gpu = ask(ops, q, tab)
    ops.rfx_host_drop(tab)
    assert on_gpu == 0
    assert why in ops.rfx_ops_last_error().decode()  # (standalone: no host ray_select behind the door, so an error object naming the reason)


@pytest.mark.parametrize("q", [{"m": ("med", "f")},                       # scalar f64: err_type in the reference
                               {"m": ("med", ("+", "v", "a"))},           # med of an expression
                               {"by": "f", "m": ("med", "v")},            # f64 key
                               {"by": {"k": "k", "a": "a"}, "m": ("med", "v")}])  # several keys
def test_out_of_scope_shapes_go_to_the_host(ops, q):
    host = door_table(n=10_000)
    tab = H.table(host)
    _, on_gpu = ask(ops, q, tab)
    ops.rfx_host_drop(tab)
    assert on_gpu == 0  # (standalone: no host ray_select behind the door, so an error object)


def test_rfx_med_operator(ops):
    rng = np.random.default_rng(4)
    v = rng.integers(-(2**62), 2**62, 100_001)
    r = ops.rfx_med(H.vector(v))
    assert not H.is_error(r), H.error_text(r)
    assert H.header(r).type == -L.RFX_F64
    assert R.same_bits(C.c_double.from_address(r + 8).value, R.median(v))  # (an atom's value sits in its header's last 8 bytes)
    ops.rfx_host_drop(r)


def test_rfx_med_over_mapgroup_ids_and_shift(ops):
    rng = np.random.default_rng(6)
    n, groups = 50_000, 700
    vals = rng.standard_normal(n)
    vals[rng.random(n) < 0.05] = np.nan
    gids = rng.integers(0, groups, n)
    for filt in (None, np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int64)):
        for itype in (0, 1):
            ix = H.lib().rfx_host_list(7)
            arr = (C.c_void_p * 7).from_address(H.payload(ix))
            arr[0], arr[1] = H.atom(itype), H.atom(groups)
            if itype == 0:
                arr[2] = H.vector(gids if filt is None else gids[filt])
                arr[3] = H.atom(R.NULL_I64)
            else:  # SHIFT: the key table over keys shifted by 1000, the source column the keys
                arr[2] = H.vector(np.arange(groups, dtype=np.int64))
                arr[3] = H.atom(1000)
                arr[4] = H.vector(gids + 1000)
            if filt is not None:
                arr[5] = H.vector(filt)
            pair = H.list_of([H.vector(vals), ix])
            H.header(pair).type = T_MAPGROUP
            r = ops.rfx_med(pair)
            assert not H.is_error(r), H.error_text(r)
            got = H.to_numpy(r)
            ops.rfx_host_drop(r)
            ops.rfx_host_drop(pair)
            g = gids if filt is None else gids[filt]
            v = vals if filt is None else vals[filt]
            assert R.same_bits(got, R.group_median(v, g, groups)), (filt is None, itype)


def test_more_than_2_pow_26_tiny_groups(eng):
    """7e7 one-row groups: more tiny segments than one wave each could launch (64 * 7e7 work-items > 2^32) -- the select kernels walk their segments."""
    n = 70_000_000
    v = np.arange(n, dtype=np.int64) * 3 - 10**9
    got = dev_median(eng, v, np.arange(n, dtype=np.int64), n)
    assert np.array_equal(got, v.astype(np.float64))


def test_golden_fixture_through_rfx_med(ops):
    """the compiled reference's own aggr_med / ray_med answers (tests/golden/med_golden.npz) through rfx_med over the same MAPGROUP indexes and vectors"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "med_golden.npz"))
    for ci in range(len(z["group_cases"])):
        _, vt, itype, groups, shift, filt = (int(x) for x in z["group_cases"][ci])
        p = f"g{ci}_"
        ix = H.lib().rfx_host_list(7)
        arr = (C.c_void_p * 7).from_address(H.payload(ix))
        arr[0], arr[1] = H.atom(itype), H.atom(groups)
        arr[2] = H.vector(z[p + "ix"])
        arr[3] = H.atom(shift)
        if itype == 1:
            arr[4] = H.vector(z[p + "keys"])
        if filt:
            arr[5] = H.vector(z[p + "filter"])
        vals = H.vector(z[p + "vals"])
        H.header(vals).type = vt  # (TIMESTAMP values keep their type)
        pair = H.list_of([vals, ix])
        H.header(pair).type = T_MAPGROUP
        r = ops.rfx_med(pair)
        assert not H.is_error(r), H.error_text(r)
        assert R.same_bits(H.to_numpy(r), z[p + "med"]), ci
        ops.rfx_host_drop(r)
        ops.rfx_host_drop(pair)
    for si in range(int(z["scalar_cases"])):
        v = z[f"s{si}_vals"]
        r = ops.rfx_med(H.vector(v))
        assert not H.is_error(r), H.error_text(r)
        assert R.same_bits(C.c_double.from_address(r + 8).value, z[f"s{si}_med"][0]), si
        ops.rfx_host_drop(r)
