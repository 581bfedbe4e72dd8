"""The sort verbs' contract without a GPU: the numpy restatement (tests/sort_ref.py) equals the fixture written from the compiled reference
(tests/golden/sort_golden.npz, tests/golden/make_sort_golden.py) in every case, bit for bit; the library as built exports the operators, the
planner and the kernel entry points, and the standalone host binds the verbs' names."""
import ctypes as C
import os

import numpy as np
import pytest

import sort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sort_golden.npz")
VERBS = ("iasc", "idesc", "asc", "desc", "rank")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def restated(verb, bits, f64, attrs):
    if verb in ("iasc", "idesc"):
        return R.order(bits, f64, verb == "idesc", attrs)
    if verb in ("asc", "desc"):
        return R.values(bits, f64, verb == "desc", attrs)
    return R.rank(bits, f64, attrs)


def test_fixture_covers_the_listed_cases(gold):
    names = list(gold["vector_names"])
    lens = {len(gold[f"v{i}_in"]) for i in range(len(names))}
    assert {0, 1, 2, 63, 64, 65, 4097, 20011} <= lens
    assert all(f"i64_digit{d}" in names for d in range(8))
    assert {int(r[2]) for r in gold["vector_cases"]} >= {0, 1, 2, 3, 4, 5}
    assert {int(r[1]) for r in gold["vector_cases"]} == {R.T_I64, R.T_TIMESTAMP, R.T_F64}
    forms = {c.split("|")[1] + str(len([k for k in c.split("|")[2].split(",") if k])) for c in gold["table_cases"]}
    assert {"atom1", "vector1", "vector2", "vector3", "vector0", "empty_i640"} <= forms


def test_restatement_equals_the_reference_on_vectors(gold):
    for row in gold["vector_cases"]:
        ci, t, attrs = int(row[0]), int(row[1]), int(row[2])
        bits = gold[f"v{ci}_in"]
        for vi, verb in enumerate(VERBS):
            want, wt, wa = gold[f"v{ci}_{verb}"], int(row[3 + 2 * vi]), int(row[4 + 2 * vi])
            got, ga = restated(verb, bits, t == R.T_F64, attrs)
            name = f"{gold['vector_names'][ci]} {verb}"
            assert wt == (t if verb in ("asc", "desc") else R.T_I64), name
            assert np.array_equal(got, want), name
            assert ga == wa, (name, ga, wa)


def test_restatement_equals_the_reference_on_tables(gold):
    names = list(gold["t_names"])
    types = dict(zip(names, (int(t) for t in gold["t_types"])))
    cols = {n: gold[f"t_in_{n}"] for n in names}
    for i, case in enumerate(gold["table_cases"]):
        verb, form, keys = case.split("|")
        keys = [k for k in keys.split(",") if k]
        n = len(cols["r"])
        perm = R.lex_order([cols[k] for k in keys], [types[k] == R.T_F64 for k in keys], verb == "xdesc") if keys else np.arange(n)
        for nm in names:
            assert np.array_equal(gold[f"t{i}_{nm}"], cols[nm][perm]), (case, nm)


SYMBOLS = ["rfx_iasc", "rfx_idesc", "rfx_asc", "rfx_desc", "rfx_rank", "rfx_xasc", "rfx_xdesc", "rfx_last_sort_on_gpu", "rfx_exec_sort",
           "rfx_exec_sort_values", "rfx_hip_sort_index", "rfx_hip_sort_values", "rfx_hip_inverse_perm"]


def test_library_exports_the_sort_entry_points():
    lib = C.CDLL(os.path.join(ROOT, "rayforce_amd", "librfx.so"))
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_python_bindings_declare_them_and_the_host_binds_the_names():
    from rayforce_amd import _lib as L, hostobj as H
    from rayforce_amd.engine import Engine
    for s in SYMBOLS[8:]:
        assert s in L.PROTOTYPES or s in L.EXEC_PROTOTYPES, s
    assert hasattr(Engine, "sort_index") and hasattr(Engine, "sort_values")
    lib = H.lib()
    for name, shape in (("iasc", 101), ("idesc", 101), ("asc", 101), ("desc", 101), ("rank", 101), ("xasc", 102), ("xdesc", 102)):
        fn = lib.rfx_host_fn(name.encode())
        assert fn, name
        assert H.header(fn).type == shape and H.header(fn).attrs == 0, name
        assert C.c_int64.from_address(fn + 8).value == C.cast(getattr(lib, "rfx_" + name), C.c_void_p).value, name
