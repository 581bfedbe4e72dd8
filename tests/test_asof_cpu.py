"""The asof join's, bin's and binr's contract without a GPU: the numpy restatement (tests/asof_ref.py) equals the fixture written from the compiled
reference (tests/golden/asof_golden.npz, tests/golden/make_asof_golden.py) in every case, bit for bit; the library as built exports the operators,
the planner and the kernel entry points, and the standalone host binds the verbs' names."""
import ctypes as C
import os

import numpy as np
import pytest

import asof_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "asof_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def index_case(gold, ci):
    name, nk = str(gold["index_cases"][ci]).split("|")
    nk = int(nk)
    return name, [gold[f"i{ci}_lk{j}"] for j in range(nk)], gold[f"i{ci}_lt"], [gold[f"i{ci}_rk{j}"] for j in range(nk)], gold[f"i{ci}_rt"], gold[f"i{ci}_ids"]


def table_case(gold, ci):
    """(name, keys, left {name: (cells, type)}, right, expected {name: (cells, null flags, type as the reference returned it)})"""
    name, keys = str(gold["table_cases"][ci]).split("|")
    sides = []
    for side in ("l", "r"):
        sides.append({str(n): (gold[f"t{ci}_{side}_{n}"], int(t)) for n, t in zip(gold[f"t{ci}_{side}_names"], gold[f"t{ci}_{side}_types"])})
    want = {str(n): (gold[f"t{ci}_out_{n}"], gold[f"t{ci}_null_{n}"], int(t)) for n, t in zip(gold[f"t{ci}_out_names"], gold[f"t{ci}_out_types"])}
    return name, keys.split(","), sides[0], sides[1], want


def test_fixture_covers_the_listed_cases(gold):
    names = [str(c).split("|")[0] for c in gold["index_cases"]]
    nks = {int(str(c).split("|")[1]) for c in gold["index_cases"]}
    assert nks == {1, 2, 3}
    nls = {len(gold[f"i{i}_lt"]) for i in range(len(names))}
    nrs = {len(gold[f"i{i}_rt"]) for i in range(len(names))}
    assert {0, 1, 63, 64, 65, 4097, 20011} <= nls and {0, 1, 63, 64, 65, 4097, 20011} <= nrs
    unsorted = 0
    for i in range(len(names)):
        _, lk, lt, rk, rt, ids = index_case(gold, i)
        if len(lk) == 1 and len(rt):
            order = np.argsort(rk[0], kind="stable")
            same = rk[0][order][1:] == rk[0][order][:-1]
            unsorted += bool((same & (rt[order][1:] < rt[order][:-1])).any())
    assert unsorted >= 4
    for want in ("issue_example", "ties", "before_first", "nulls_sorted", "nulls_unsorted", "wide_three_keys", "group_lengths_sorted", "group_lengths_unsorted",
                 "one_group_sorted", "one_group_unsorted"):
        assert want in names
    i = names.index("group_lengths_unsorted")
    assert set(np.bincount(gold[f"i{i}_rk0"])) == {1, 2, 3, 64, 65}
    i = names.index("nulls_sorted")
    assert (gold[f"i{i}_lk0"] == R.NULL).any() and (gold[f"i{i}_rk1"] == R.NULL).any() and (gold[f"i{i}_lt"] == R.NULL).any() and (gold[f"i{i}_rt"] == R.NULL).any()
    tnames = [str(c).split("|")[0] for c in gold["table_cases"]]
    ttypes = {int(gold[f"t{i}_l_types"][list(gold[f"t{i}_l_names"]).index("t")]) for i in range(len(tnames))}
    assert {R.T_I64, R.T_TIMESTAMP, R.T_TIME} <= ttypes
    assert "empty_left" in tnames and "empty_right" in tnames and "all_matched" in tnames
    lists = sum(int((gold[f"t{i}_out_types"] == R.T_LIST).any()) for i in range(len(tnames)))
    assert 0 < lists < len(tnames)  # both: right-only columns that came back as LISTs of Null objects, and tables of typed vectors only
    bnames = [str(c).split("|")[0] for c in gold["bin_cases"]]
    for want in ("sorted", "unsorted", "all_equal", "empty_x", "empty_y", "below_and_above", "nulls_sorted", "sorted_duplicates", "timestamp"):
        assert want in bnames


def test_the_issue_example_is_what_the_reference_answers(gold):
    _, lk, lt, rk, rt, ids = index_case(gold, 0)
    assert lk[0][0] == 1 and lt[0] == 5 and list(rt[rk[0] == 1]) == [4, 2, 6, 3]
    assert ids[0] == 1  # time 2: where the probe sequence lands, not the greatest time <= 5 (row 0, time 4)
    names = [str(c).split("|")[0] for c in gold["bin_cases"]]
    i = names.index("issue_example")
    assert list(gold[f"b{i}_bin"]) == [-1, -1, 5, 1]


def test_restatement_equals_the_reference_on_the_join_index(gold):
    for ci in range(len(gold["index_cases"])):
        name, lk, lt, rk, rt, ids = index_case(gold, ci)
        got = R.asof_index(lk, lt, rk, rt)
        assert got.dtype == np.int64 and np.array_equal(got, ids), name


def test_restatement_equals_the_reference_on_whole_tables(gold):
    for ci in range(len(gold["table_cases"])):
        name, keys, left, right, want = table_case(gold, ci)
        got = R.asof_join(keys, left, right)
        assert list(got) == list(want), name
        for col, (cells, nul, t) in want.items():
            gc, gn, gt = got[col]
            assert np.array_equal(gn, nul), (name, col)
            assert np.array_equal(np.where(nul == 1, 0, gc), np.where(nul == 1, 0, cells)), (name, col)
            # a typed vector keeps its type; a LIST is what the reference makes of a right-only column with an unmatched row (and only of that)
            assert t == (R.T_LIST if nul.any() else gt), (name, col, t)


def test_restatement_equals_the_reference_on_bin_and_binr(gold):
    for ci, case in enumerate(gold["bin_cases"]):
        x, y = gold[f"b{ci}_x"], gold[f"b{ci}_y"]
        assert np.array_equal(R.bin_(x, y), gold[f"b{ci}_bin"]), case
        assert np.array_equal(R.binr(x, y), gold[f"b{ci}_binr"]), case


SYMBOLS = ["rfx_asof_join", "rfx_bin", "rfx_binr", "rfx_last_asof_on_gpu", "rfx_exec_asof_index", "rfx_exec_bin", "rfx_hip_seg_search", "rfx_hip_asof_runs"]


def test_library_exports_the_asof_entry_points():
    lib = C.CDLL(os.path.join(ROOT, "rayforce_amd", "librfx.so"))
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_python_bindings_declare_them_and_the_host_binds_the_names():
    from rayforce_amd import _lib as L, hostobj as H
    from rayforce_amd.engine import Engine
    for s in SYMBOLS[4:]:
        assert s in L.PROTOTYPES or s in L.EXEC_PROTOTYPES, s
    for m in ("asof_index", "asof_join", "bin", "binr"):
        assert hasattr(Engine, m), m
    lib = H.lib()
    for name, sym, shape in (("asof-join", "rfx_asof_join", 103), ("bin", "rfx_bin", 102), ("binr", "rfx_binr", 102)):
        fn = lib.rfx_host_fn(name.encode())
        assert fn, name
        assert H.header(fn).type == shape and H.header(fn).attrs == 0, name
        assert C.c_int64.from_address(fn + 8).value == C.cast(getattr(lib, sym), C.c_void_p).value, name
