"""The sort verbs over 1-, 2- and 4-byte keys without a GPU: the numpy restatement (tests/sort_narrow_ref.py) equals the fixture written from the
compiled reference (tests/golden/sort_narrow_golden.npz, tests/golden/make_sort_narrow_golden.py) in every case, bit for bit, and the fixture holds
the cases it is meant to."""
import os

import numpy as np
import pytest

import sort_narrow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sort_narrow_golden.npz")
VERBS = ("iasc", "idesc", "asc", "desc", "rank")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def cases(gold):
    """(name, cells, type, attrs, {verb: (cells or None for an error, type, attrs)})"""
    for row in gold["vector_cases"]:
        ci, t, attrs = int(row[0]), int(row[1]), int(row[2])
        ans = {}
        for vi, verb in enumerate(VERBS):
            rt, ra = int(row[3 + 2 * vi]), int(row[4 + 2 * vi])
            ans[verb] = (None if rt == R.T_ERR else gold[f"v{ci}_{verb}"], rt, ra)
        yield str(gold["vector_names"][ci]), gold[f"v{ci}_in"], t, attrs, ans


def test_fixture_covers_the_listed_cases(gold):
    all_cases = list(cases(gold))
    names = [c[0] for c in all_cases]
    assert {c[2] for c in all_cases} == {R.T_B8, R.T_U8, R.T_I16, R.T_I32, R.T_DATE, R.T_TIME}
    assert {len(c[1]) for c in all_cases} == {0, 1, 2, 63, 64, 65, 130, 200, 300, 500, 700, 4097, 20011}
    assert {c[0] for c in all_cases if len(c[1]) == 20011} == {"i32_ties", "i16_ties"}
    for t in (R.T_B8, R.T_U8, R.T_I16, R.T_I32, R.T_DATE, R.T_TIME):
        assert {0, 1, 2, 63, 64, 65} <= {len(c[1]) for c in all_cases if c[2] == t}, t
    assert all(c[1].dtype == R.DTYPE[c[2]] for c in all_cases)
    by = {c[0]: c for c in all_cases}
    assert {R.NULL_I32, 2**31 - 1, -1, 0} <= set(by["i32_special"][1].tolist()) and -(2**15) in by["i16_special"][1] and 255 in by["u8_special"][1]
    for nm in ("date_nulls", "time_nulls"):
        share = float(np.mean(by[nm][1] == R.NULL_I32))
        assert 0.07 < share < 0.13, (nm, share)
    assert all(f"i32_digit{d}" in names for d in range(4)) and all(f"i16_digit{d}" in names for d in range(2))
    for d in range(4):
        assert R.varying_digits(by[f"i32_digit{d}"][1]) == 1
    assert set(by["b8_bytes"][1].tolist()) - {0, 1}
    for tag in ("i32", "date", "i16", "u8", "b8"):
        assert all(f"{tag}_attrs{a}" in names for a in (1, 2, 3, 4, 5)), tag
        assert np.array_equal(by[f"{tag}_attrs4"][1], np.sort(by[f"{tag}_attrs4"][1]))  # (ascending data under ATTR_DESC)
    # every answer holds cells, a type code and an attribute byte; errors are recorded as such -- the reference's reverse has no I16 arm
    errors = {(c[0], v) for c in all_cases for v in VERBS if c[4][v][0] is None}
    assert errors == {("i16_attrs2", "desc"), ("i16_attrs3", "desc"), ("i16_attrs4", "asc"), ("i16_attrs5", "asc"), ("i16_attrs4_empty", "asc")}


def test_restatement_equals_the_reference(gold):
    for name, cells, t, attrs, ans in cases(gold):
        for verb in VERBS:
            want, wt, wa = ans[verb]
            got, ga = R.restated(verb, cells, attrs)
            tag = f"{name} {verb}"
            if want is None:
                assert got is None, tag
                continue
            assert got is not None, tag
            assert wt == (t if verb in ("asc", "desc") else R.T_I64), tag
            if verb in ("asc", "desc"):
                assert want.dtype == cells.dtype and got.dtype == cells.dtype, tag
            else:
                assert want.dtype == np.int32, tag  # (permutations are stored as int32)
            assert np.array_equal(got, want), tag
            assert ga == wa, (tag, ga, wa)


def test_the_widened_image_has_the_same_key():
    rng = np.random.default_rng(3)
    cells = np.concatenate([rng.integers(-(2**31), 2**31, 1000), [R.NULL_I32, 2**31 - 1, -1, 0]]).astype(np.int32)
    for desc in (False, True):
        assert np.array_equal(R.key32_of_widened(R.widen(cells), desc), R.key32(cells, desc))
    assert R.key32(np.array([R.NULL_I32], np.int32))[0] == 0


def test_python_constants_match_the_header():
    from rayforce_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "rfx_hip.h")).read()
    for name in ("RFX_B8", "RFX_U8", "RFX_I16", "RFX_I32", "RFX_I32_WIDE"):
        assert f"{name} = {getattr(L, name):#x}" in text or f"{name} = {getattr(L, name)}" in text, name
