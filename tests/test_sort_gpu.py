"""The device sort on the GPU, all by equality of bits: the flat kernels against the numpy restatement (tests/sort_ref.py), every case of the
reference's fixture (tests/golden/sort_golden.npz) through rfx_iasc .. rfx_xdesc, the shapes handed back, full-size runs by properties."""
import ctypes as C

import numpy as np
import pytest
import torch

import sort_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H
from rayforce_amd.engine import Engine, RfxError
from test_sort_cpu import GOLD, VERBS, restated

pytestmark = pytest.mark.gpu
NULL = -(2**63)
MIN = torch.iinfo(torch.int64).min


def dev_bits(eng, bits, f64):
    return eng.column(bits.view(np.float64) if f64 else bits)


def sort_index(eng, col, f64, desc, perm_in=None):
    n = col.numel()
    out = torch.empty(n, dtype=torch.int64, device=col.device)
    passes = C.c_int32(-1)
    L.check(eng.lib.rfx_hip_sort_index(eng._ctx, col.data_ptr(), L.RFX_F64 if f64 else L.RFX_I64, n, int(desc),
                                       perm_in.data_ptr() if perm_in is not None else None, out.data_ptr(), C.byref(passes)), "sort_index")
    eng.sync()
    return out, passes.value


def varying_digits(bits, f64):
    k = R.u(bits, f64)
    return sum(1 for d in range(8) if len(np.unique((k >> np.uint64(8 * d)) & np.uint64(255))) > 1)


def cells_of(rng, kind, n):
    """(int64 bit patterns, f64?)"""
    if kind == "narrow":
        return rng.integers(0, 1_000_000, n), False
    if kind == "full":
        return rng.integers(-(2**63), 2**63 - 1, n), False
    if kind == "one_digit":
        return (rng.integers(0, 256, n) << 40) + 7, False
    if kind == "extremes":
        return rng.choice(np.array([NULL, NULL + 1, 2**63 - 1, 0, -1, 1], np.int64), n), False
    f = (rng.standard_normal(n) * 1e3).view(np.int64)
    sp = np.concatenate([np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 5e-324, -1e-310]).view(np.int64), [-0x0008000000000000, 0x7FF0000000000123]]).astype(np.int64)
    return np.where(rng.random(n) < 0.2, rng.choice(sp, n), f), True


@pytest.mark.parametrize("n", [1, 63, 65, 100_000, 3_000_001])
@pytest.mark.parametrize("kind", ["narrow", "full", "one_digit", "extremes", "f64"])
def test_flat_kernels_equal_the_restatement(eng, kind, n):
    rng = np.random.default_rng(n * 31 + len(kind))
    bits, f64 = cells_of(rng, kind, n)
    bits = np.ascontiguousarray(bits, dtype=np.int64)
    col = dev_bits(eng, bits, f64)
    pin = rng.permutation(n).astype(np.int64)
    dpin = eng.column(pin)
    for desc in (False, True):
        got, passes = sort_index(eng, col, f64, desc)
        assert np.array_equal(got.cpu().numpy(), R.order(bits, f64, desc)[0]), (kind, n, desc)
        assert passes == varying_digits(bits, f64), (kind, n, desc, passes)
        # one level of a multi-column sort: the keys read through an incoming permutation
        got, passes = sort_index(eng, col, f64, desc, dpin)
        assert np.array_equal(got.cpu().numpy(), pin[R.order(bits[pin], f64, desc)[0]]), (kind, n, desc, "perm_in")
        assert passes == varying_digits(bits, f64)
        vals = eng.sort_values(col, desc)
        assert np.array_equal(vals.cpu().numpy().view(np.int64), R.values(bits, f64, desc)[0]), (kind, n, desc, "values")
    before = eng.xstat(L.RFX_XSTAT_SORTS), eng.xstat(L.RFX_XSTAT_SORT_PASSES)
    perm = eng.sort_index(col)
    assert eng.xstat(L.RFX_XSTAT_SORTS) - before[0] == 1 and eng.xstat(L.RFX_XSTAT_SORT_PASSES) - before[1] == varying_digits(bits, f64)
    inv = torch.empty_like(perm)
    L.check(eng.lib.rfx_hip_inverse_perm(eng._ctx, perm.data_ptr(), n, inv.data_ptr()), "inverse_perm")
    eng.sync()
    assert np.array_equal(inv.cpu().numpy(), R.rank(bits, f64)[0])


def test_all_equal_keys_run_no_pass(eng):
    bits = np.full(70_000, 42, np.int64)
    got, passes = sort_index(eng, eng.column(bits), False, True)
    assert passes == 0 and np.array_equal(got.cpu().numpy(), np.arange(70_000))


def test_two_columns_through_the_planner(eng):
    rng = np.random.default_rng(5)
    n = 200_003
    a, b = rng.integers(0, 50, n), (rng.integers(-3, 3, n) * 0.5).view(np.int64)
    for desc in (False, True):
        got = eng.sort_index([eng.column(a), eng.column(b.view(np.float64))], descending=desc)
        assert np.array_equal(got.cpu().numpy(), R.lex_order([a, b], [False, True], desc))


def test_sharded_sort_is_refused_with_its_reason():
    e = Engine(0, shards=2)
    try:
        with pytest.raises(RfxError, match="sort over a sharded table"):
            e.sort_index(torch.arange(1000, device="cuda:0"))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- the door
@pytest.fixture(scope="module")
def ops(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = H.lib()
    o.rfx_host_bind()
    return o


def host_vector(ops, bits, t, attrs=0):
    o = ops.rfx_host_vector(t, bits.size)
    if bits.size:
        C.memmove(H.payload(o), np.ascontiguousarray(bits).ctypes.data, bits.nbytes)
    H.header(o).attrs = attrs
    return o


def raw_cells(o):
    h = H.header(o)
    return np.frombuffer((C.c_char * (h.len * 8)).from_address(H.payload(o)), dtype=np.int64).copy()


def test_fixture_vectors_through_the_operators(ops):
    gold = np.load(GOLD)
    for row in gold["vector_cases"]:
        ci, t, attrs = int(row[0]), int(row[1]), int(row[2])
        bits = gold[f"v{ci}_in"]
        for vi, verb in enumerate(VERBS):
            x = host_vector(ops, bits, t, attrs)
            r = getattr(ops, "rfx_" + verb)(x)
            name = f"{gold['vector_names'][ci]} {verb}"
            assert not H.is_error(r), (name, H.error_text(r))
            assert H.header(r).type == int(row[3 + 2 * vi]) and H.header(r).attrs == int(row[4 + 2 * vi]), name
            assert np.array_equal(raw_cells(r), gold[f"v{ci}_{verb}"]), name
            assert ops.rfx_last_sort_on_gpu() == int(len(bits) > 0 and not attrs & 6), name
            ops.rfx_host_drop(r)
            ops.rfx_host_drop(x)


def test_fixture_tables_through_xasc_and_xdesc(ops):
    gold = np.load(GOLD)
    names = [str(s) for s in gold["t_names"]]
    types = [int(t) for t in gold["t_types"]]
    syms = np.array([ops.rfx_host_intern(str(s).encode(), len(str(s))) for s in gold["t_symbols"]], np.int64)
    back = {int(s): i for i, s in enumerate(syms)}

    def table():
        cols = [host_vector(ops, syms[gold[f"t_in_{n}"]] if t == R.T_SYMBOL else gold[f"t_in_{n}"], t) for n, t in zip(names, types)]
        return ops.rfx_host_table(H.symbols(names), H.list_of(cols))

    for i, case in enumerate(gold["table_cases"]):
        verb, form, keys = str(case).split("|")
        keys = [k for k in keys.split(",") if k]
        y = ops.rfx_host_symbol(keys[0].encode()) if form == "atom" else ops.rfx_host_vector(R.T_I64, 0) if form == "empty_i64" else H.symbols(keys)
        tab = table()
        r = getattr(ops, "rfx_" + verb)(tab, y)
        assert not H.is_error(r), (case, H.error_text(r))
        assert H.header(r).type == H.T_TABLE
        assert ops.rfx_last_sort_on_gpu() == int(bool(keys)), case
        rk, rv = H.list_items(r)
        assert [ops.rfx_host_symbol_name(int(s)).decode() for s in raw_cells(rk)] == names
        for n, t, c in zip(names, types, H.list_items(rv)):
            assert H.header(c).type == t, (case, n)
            got = raw_cells(c)
            if t == R.T_SYMBOL:
                got = np.array([back[int(s)] for s in got], np.int64)
            assert np.array_equal(got, gold[f"t{i}_{n}"]), (case, n)
        for o in (r, tab, y):
            ops.rfx_host_drop(o)


def test_shapes_outside_the_device_path_are_handed_back(ops):
    # (standalone: no host verb behind the door, so an error object naming the reason -- never an answer of ours)
    x = host_vector(ops, np.arange(10, dtype=np.int64), R.T_SYMBOL)
    r = ops.rfx_iasc(x)
    assert H.is_error(r) and ops.rfx_last_sort_on_gpu() == 0 and "key type" in ops.rfx_ops_last_error().decode()
    i32 = ops.rfx_host_vector(4, 10)
    tab = ops.rfx_host_table(H.symbols(["a", "b"]), H.list_of([H.vector(np.arange(10)), i32]))
    y = ops.rfx_host_symbol(b"a")
    r2 = ops.rfx_xasc(tab, y)
    assert H.is_error(r2) and ops.rfx_last_sort_on_gpu() == 0 and "not an 8-byte vector" in ops.rfx_ops_last_error().decode()
    tab2 = H.table({"a": np.arange(10), "s": np.arange(10)})
    H.header(H.list_items(H.list_items(tab2)[1])[1]).type = R.T_SYMBOL
    ys = ops.rfx_host_symbol(b"s")
    r3 = ops.rfx_xdesc(tab2, ys)
    assert H.is_error(r3) and "key type" in ops.rfx_ops_last_error().decode()


def test_xdesc_of_a_grouped_select_by_its_sum(ops):
    rng = np.random.default_rng(8)
    n = 3_000_000
    host = {"k": rng.integers(0, 1_000_000, n), "v": rng.integers(-1000, 1000, n)}
    tab = H.table(host)
    d = H.select_dict({"by": "k", "s": ("sum", "v")}, tab)
    sel = ops.rfx_select(d)
    assert not H.is_error(sel) and ops.rfx_last_select_on_gpu() == 1
    want = H.table_to_numpy(sel)
    y = ops.rfx_host_symbol(b"s")
    r = ops.rfx_xdesc(sel, y)
    assert not H.is_error(r), H.error_text(r)
    assert ops.rfx_last_sort_on_gpu() == 1
    got = H.table_to_numpy(r)
    perm = R.order(want["s"], False, True)[0]
    assert len(perm) > 900_000
    for name in want:
        assert np.array_equal(got[name], want[name][perm]), name


# ---------------------------------------------------------------------------------------------------- full size, by properties
def gather(eng, col, ids):
    out = torch.empty(ids.numel(), dtype=col.dtype, device=col.device)
    L.check(eng.lib.rfx_hip_gather(eng._ctx, col.data_ptr(), ids.data_ptr(), ids.numel(), out.data_ptr()), "gather")
    eng.sync()
    return out


def check_sorted(eng, col, f64, perm, desc=False):
    """perm is a permutation; the sort key is monotone along it; equal neighbours keep ascending rows"""
    n = col.numel()
    inv = torch.empty_like(perm)
    L.check(eng.lib.rfx_hip_inverse_perm(eng._ctx, perm.data_ptr(), n, inv.data_ptr()), "inverse_perm")
    eng.sync()
    back = gather(eng, inv, perm)  # inv[perm[j]] == j for every j <=> every row is hit exactly once (n cells, n distinct targets)
    assert bool(((perm >= 0) & (perm < n)).all())
    step = 1 << 27
    for a in range(0, n, step):
        b = min(n, a + step)
        assert bool((back[a:b] == torch.arange(a, b, device=col.device)).all())
    del inv, back
    keys = torch.empty(n, dtype=torch.int64, device=col.device)
    L.check(eng.lib.rfx_hip_median_keys(eng._ctx, col.data_ptr(), L.RFX_F64 if f64 else L.RFX_I64, n, keys.data_ptr()), "keys")
    eng.sync()
    ks = gather(eng, keys, perm)
    del keys
    ks ^= MIN  # u as a signed number of the same order
    for a in range(0, n - 1, step):
        b = min(n - 1, a + step)
        lo, hi = ks[a:b], ks[a + 1:b + 1]
        assert bool(((hi < lo) if desc else (hi > lo)).logical_or((hi == lo) & (perm[a + 1:b + 1] > perm[a:b])).all())


@pytest.mark.parametrize("f64", [False, True])
def test_1e8_rows_by_properties(eng, f64):
    n = 100_000_000
    g = torch.Generator(device="cuda:0").manual_seed(3)
    if f64:
        col = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=g)
        col[::1000] = float("nan")
        col[1::1000] = -0.0
    else:
        col = torch.randint(-(2**62), 2**62, (n,), dtype=torch.int64, device="cuda:0", generator=g)
        col[::1000] = MIN
    for desc in (False, True):
        perm = eng.sort_index(col, descending=desc)
        check_sorted(eng, col, f64, perm, desc)
        del perm
    torch.cuda.empty_cache()


def test_2_pow_31_plus_5_rows_of_narrow_keys(eng):
    """the largest size tested: rows travel as 4 bytes up to 2^32 - 1 of them; this is past the signed 32-bit boundary"""
    n = 2**31 + 5
    torch.cuda.empty_cache()
    eng.trim()
    free = torch.cuda.mem_get_info(0)[0]
    need = n * (8 + 8 + 24 + 8 + 8 + 4)  # column, permutation, sort scratch, the check's inverse / gathered keys, slack
    if free < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory, {free >> 30} GiB free")
    g = torch.Generator(device="cuda:0").manual_seed(4)
    col = torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device="cuda:0", generator=g)
    before = eng.xstat(L.RFX_XSTAT_SORT_PASSES)
    perm = eng.sort_index(col)
    assert eng.xstat(L.RFX_XSTAT_SORT_PASSES) - before == 3
    check_sorted(eng, col, False, perm)
    del perm, col
    torch.cuda.empty_cache()
    eng.trim()
