"""The numpy restatement of `med` (tests/median_ref.py) against the compiled reference's own answers (tests/golden/med_golden.npz, written by
tests/golden/make_med_golden.py through aggr_med / ray_med), against the contract written out case by case, and against a plain sort-based
definition -- so the GPU tests that use it at scale are held to the reference's rules."""
import os

import numpy as np
import pytest

import median_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "med_golden.npz")


def golden_groups(z, ci):
    """case ci of the fixture: (values in index order, group id per value, groups, aggr_med's answer)"""
    _, vt, itype, groups, shift, filt = (int(x) for x in z["group_cases"][ci])
    p = f"g{ci}_"
    keys, vals, ix = z[p + "keys"], z[p + "vals"], z[p + "ix"]
    rows = z[p + "filter"] if filt else np.arange(len(keys))
    gids = ix if itype == 0 else ix[keys[rows] - shift]  # IDS: one id per (filtered) row; SHIFT: the key table at source - shift
    return vals[rows], gids.astype(np.int64), groups, z[p + "med"]


def test_restatement_equals_the_reference_aggr_med():
    z = np.load(GOLD)
    kinds = set()
    for ci in range(len(z["group_cases"])):
        v, g, groups, want = golden_groups(z, ci)
        kinds.add((int(z["group_cases"][ci][1]), int(z["group_cases"][ci][2]), int(z["group_cases"][ci][5])))
        assert R.same_bits(R.group_median(v, g, groups), want), ci
    assert len(kinds) == 12  # i64 / f64 / timestamp values x SHIFT / IDS indexes x with / without filter ids


def test_restatement_equals_the_reference_ray_med():
    z = np.load(GOLD)
    for si in range(int(z["scalar_cases"])):
        v = z[f"s{si}_vals"]
        assert R.same_bits(R.median(v), z[f"s{si}_med"][0]), (si, v[:8])

NULL = R.NULL_I64


def plain(values, rule):
    """The reference's own steps for one group: sort ascending by its sort keys, then its formula."""
    v = np.asarray(values)
    s = v[np.argsort(R.sort_keys(v), kind="stable")]
    l = len(s)
    if l == 0:
        return np.nan
    if l % 2:
        return float(s[l // 2])
    if v.dtype == np.float64:
        return float(R.flush(R.flush(R.flush(s[l // 2 - 1]) + R.flush(s[l // 2])) / 2.0))
    if rule == R.SCALAR:
        with np.errstate(over="ignore"):
            return float(np.int64(s[l // 2 - 1]) + np.int64(s[l // 2])) / 2.0
    return (float(s[l // 2 - 1]) + float(s[l // 2])) / 2.0


def test_sort_keys_order_the_reference_way():
    f = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf])
    k = R.sort_keys(f)
    assert k[0] == 0 and np.all(np.diff(k[1:].astype(object)) > 0)  # NaN first, then -inf .. +inf with -0.0 before +0.0
    assert R.same_bits(R.from_keys(k, True), f)
    i = np.array([NULL, -5, 0, 7, 2**63 - 1], np.int64)
    k = R.sort_keys(i)
    assert np.all(np.diff(k.astype(object)) > 0) and np.array_equal(R.from_keys(k, False), i)


def test_written_out_cases():
    grouped = [([3, 1, 2], 2.0), ([4, 1, 3, 2], 2.5), ([NULL], -9.223372036854775808e18), ([NULL, 5], (-9.223372036854775808e18 + 5.0) / 2.0),
               ([7, 7, 7, 7], 7.0), ([2**62, 2**62 + 2], 4.611686018427387904e18 + 1)]
    for vals, want in grouped:
        v = np.array(vals, np.int64)
        got = R.group_median(v, np.zeros(len(v), np.int64), 1)[0]
        assert R.same_bits(got, want), (vals, got, want)
        assert R.same_bits(got, plain(v, R.GROUPED)), vals
    # scalar: l counts the non-null values, the ranks index the whole sorted vector (nulls first); the i64 sum wraps
    scalar = [([3, 1, 2], 2.0), ([NULL], np.nan), ([NULL, 5], -9.223372036854775808e18), ([NULL, 5, 7], float(np.int64(NULL + 5)) / 2.0),
              ([2**62, 2**62 + 2], float(np.int64(-(2**63) + 2)) / 2.0), ([], np.nan)]
    for vals, want in scalar:
        assert R.same_bits(R.median(np.array(vals, np.int64)), want), vals


def test_f64_cases():
    for vals, want in [([np.nan, 1.0, 2.0], 1.0), ([np.nan, 1.0], np.nan), ([-0.0, 0.0], 0.0), ([-0.0], -0.0), ([-np.inf, np.inf], np.nan),
                       ([np.inf, 1.0, np.inf], np.inf), ([5e-324, 1e-323], 0.0), ([-1e-310, 1.0, -1e-310], -1e-310)]:  # (subnormals flushed only in arithmetic)
        v = np.array(vals)
        got = R.group_median(v, np.zeros(len(v), np.int64), 1)[0]
        assert R.same_bits(got, want), (vals, got, want)
        assert R.same_bits(got, plain(v, R.GROUPED)), vals


@pytest.mark.parametrize("seed", range(20))
def test_groups_against_the_plain_definition(seed):
    rng = np.random.default_rng(seed)
    n, groups = int(rng.integers(1, 400)), int(rng.integers(1, 40))
    gids = rng.integers(-1, groups, n)
    if seed % 2:
        v = rng.choice(np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 5e-324, -1.5, 2.25, 1e300]), n)
    else:
        v = rng.choice(np.array([NULL, 2**63 - 1, -(2**62), 0, 1, -1, 3, 2**62], np.int64), n)
    got = R.group_median(v, gids, groups)
    want = np.array([plain(v[gids == g], R.GROUPED) for g in range(groups)])
    assert R.same_bits(got, want)
