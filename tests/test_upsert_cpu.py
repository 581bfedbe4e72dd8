"""upsert and insert without a GPU: the numpy restatement (tests/upsert_ref.py) equals every case the compiled reference answered
(tests/golden/upsert_golden.npz) and a literal per-cell replay of the reference's loop on random small cases; the fixture holds what the issue lists; the
two verb rows behind rfx_host_fn; every reason the door gives before it needs a device, with its text in rfx_ops_last_error(); and the restatement of
the three device calls (plan, place, fill), the reference of tests/test_upsert_edges_gpu.py, pinned to a per-row loop, to the replay and to the fixture."""
import ctypes as C

import numpy as np
import pytest

import upsert_door as D
import upsert_ref as R
from rayforce_amd import _lib as L
from rayforce_amd import hostobj as H

CASES = R.load_cases()


@pytest.fixture(scope="module")
def ops(built):
    o = H.lib()
    o.rfx_host_bind()
    return o


def test_the_fixture_holds_what_the_issue_lists():
    by = {c["name"]: c for c in CASES}
    for n in (0, 1, 64, 4097, 2**20 + 5):
        for m in (1, 63, 64, 65, 1025, 4097):  # (a batch of no rows is the host's for both verbs: HOST_SHAPES empty_batch, insert_empty)
            c = by[f"grid_n{n}_m{m}"]
            assert (c["n"], c["m"]) == (n, m)
    assert {"pattern_all", "pattern_none", "pattern_runs", "pattern_dups", "pattern_newdups", "table_dups", "sparse_keys", "keys2", "keys3", "ts_key",
            "nine_columns", "short_list", "dict_shuffled_missing", "table_shuffled_missing", "record_all", "record_none", "record_dict_all",
            "record_dict_none", "insert_list", "insert_dict", "insert_table", "insert_record", "host_empty_batch", "host_insert_empty"} <= set(by)
    assert by["pattern_runs"]["m"] // 2 > 2048 and by["pattern_dups"]["m"] % 2048 == 1  # runs longer than a block's rows; the last duplicate alone in the last block
    assert len(by["nine_columns"]["types"]) == 9 > L.RFX_MAX_COLS
    widths = {np.dtype(R.DTYPE[tp]).itemsize for tp in by["none_every_width"]["types"]}
    assert widths == {1, 2, 4, 8}
    for tp, _a, cells in by["none_every_width"]["out"]:  # the null cell / NaN among the appended cells
        tail = cells[by["none_every_width"]["n"]:]
        if tp == R.F64:
            assert np.isnan(tail).any()
        elif tp in (R.I16, R.I32):
            assert (tail == np.iinfo(R.DTYPE[tp]).min).any()
    assert {c["shape"] for c in CASES if c.get("host")} == set(R.HOST_SHAPES)


def test_the_restatement_equals_every_golden_case():
    ran = 0
    for c in CASES:
        if c.get("host"):
            continue
        got = R.answer(c)
        assert len(got) == len(c["out"]), c["name"]
        for (tp, attrs, cells), want in zip(got, c["out"]):
            D.same_column(c["name"], tp, attrs, cells, want)
        ran += 1
    assert ran == sum(1 for c in CASES if not c.get("host")) and ran >= 60


def test_the_restatement_equals_the_per_cell_replay():
    rng = np.random.default_rng(20261021)
    forms = ("list", "dict", "table")
    for trial in range(200):
        keys = int(rng.integers(0, 4))
        p = int(rng.integers(max(keys, 1), 7))
        types = [R.I64 if i < max(keys, 1) else int(rng.choice([R.I64, R.F64, R.TS, R.B8, R.I16, R.I32])) for i in range(p)]
        form = forms[int(rng.integers(0, 3))]
        if form == "list":
            given = list(range(int(rng.integers(max(keys, 1), p + 1)) if keys else p))
        else:
            rest = [i for i in range(max(keys, 1), p) if rng.random() < 0.6]
            given = [int(i) for i in rng.permutation(list(range(max(keys, 1))) + rest)]
        c = dict(name=f"trial{trial}", verb="upsert" if keys else "insert", keys=keys, form=form, types=types, n=int(rng.integers(0, 40)),
                 m=int(rng.integers(6, 60)), pattern=R.PATTERNS[int(rng.integers(0, 3))], given=given, tdup=int(rng.integers(0, 2)))
        for (tp, attrs, cells), want in zip(R.answer(c), R.replay(c)):
            D.same_column(c["name"], tp, attrs, cells, want)


def test_the_plan_equals_its_per_row_loop():
    """R.plan, the reference of tests/test_upsert_edges_gpu.py: 200 random (n, m, idx), the hostile "none" values among heavily repeated rows"""
    rng = np.random.default_rng(20261022)
    for trial in range(200):
        n, m = int(rng.integers(0, 301)), int(rng.integers(1, 5001))
        none = np.array(R.HOSTILE + (n, n + 5, 2**62), dtype=np.int64)
        rows = rng.integers(0, n, m) // int(rng.integers(1, 9)) if n else np.zeros(m, dtype=np.int64)  # (the divisor: heavier repeats)
        idx = np.where((rng.random(m) < rng.random()) if n else True, none[rng.integers(0, len(none), m)], rows)
        (dest, a), (want, wa) = R.plan(idx, n), R.plan_loop(idx, n)
        assert a == wa and dest.dtype == want.dtype and np.array_equal(dest, want), (trial, n, m)
        hit = (idx >= 0) & (idx < n)
        assert a == m - int(hit.sum()) and len(set(dest[dest >= 0].tolist())) == int((dest >= 0).sum())  # no destination twice
    assert R.plan(np.zeros(0, dtype=np.int64), 7)[1] == 0


def test_the_scale_patterns_equal_the_per_cell_replay():
    assert not set(R.SCALE_PATTERNS) & set(R.PATTERNS)
    for pattern in R.SCALE_PATTERNS:
        for keys, types in ((1, [R.I64, R.F64, R.I64, R.TS]), (2, [R.I64, R.TS, R.F64, R.I64])):
            c = dict(name=f"{pattern}_keys{keys}", verb="upsert", keys=keys, form="list", types=types, n=4097, m=4097, pattern=pattern, given=[0, 1, 2, 3])
            counts = {}
            for (tp, attrs, cells), want in zip(R.answer(c, counts), R.replay(c)):
                D.same_column(c["name"], tp, attrs, cells, want)
            refs = R.batch_refs(pattern, 4097, 4097)
            assert counts["matched"] == int((refs < 4097).sum()) and 0 < counts["matched"] < 4097
            assert len(set(refs[refs < 4097].tolist())) == {"hot": 1000, "one": 1}[pattern]


def test_every_golden_case_is_rebuilt_from_plan_place_and_fill():
    ran = 0
    for c in CASES:
        if c.get("host"):
            continue
        counts, again = {}, {}
        got = R.rebuilt(c, again)
        for (tp, attrs, cells), want in zip(got, R.answer(c, counts)):
            D.same_column(c["name"], tp, attrs, cells, want)
        assert counts == again and len(got) == len(c["out"]), c["name"]
        for (tp, attrs, cells), want in zip(got, c["out"]):
            D.same_column(c["name"], tp, attrs, cells, want)
        ran += 1
    assert ran >= 60


def test_the_verb_rows_are_bound_by_name(ops):
    for name in ("upsert", "insert"):
        fn = ops.rfx_host_fn(name.encode())
        assert fn and H.header(fn).type == 103 and H.header(fn).attrs == 0
        addr = C.c_int64.from_address(H.payload(fn) - 8).value
        assert addr == C.cast(getattr(ops, "rfx_" + name), C.c_void_p).value, name
        ops.rfx_host_drop(fn)


def test_every_reason_reachable_without_a_device(ops):
    hosts = [c for c in CASES if c.get("host")]
    assert len(hosts) == len(R.HOST_SHAPES)
    for c in hosts:
        if c["shape"] not in R.DEVICE_DECIDED:
            D.check_refused(ops, c)


def test_ctypes_mirror_the_headers():
    assert C.sizeof(L.UpsertCol) == 24 and C.sizeof(L.UpsertXCol) == 40
    assert (L.RFX_XSTAT_UPSERTS, L.RFX_XSTAT_UPSERT_MATCHED, L.RFX_XSTAT_UPSERT_APPENDED, L.RFX_XSTAT_INSERTS) == (44, 45, 46, 47)
    assert (L.RFX_XSTAT_NS_UPSERT_INDEX, L.RFX_XSTAT_NS_UPSERT_PLAN, L.RFX_XSTAT_NS_UPSERT_PLACE) == (48, 49, 50)
