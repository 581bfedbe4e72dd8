"""Helpers of the upsert / insert tests: a golden case (tests/upsert_ref.py load_cases) through the C operator door over standalone host objects and
through the Engine over device tensors, and the `host_` shapes as objects.  Also imported by the child processes of the residency and sharded runs."""
import ctypes as C

import numpy as np

import upsert_ref as R
from concat_door import TORCH_OF, cells_of, host_atom, host_vector, same_column  # noqa: F401
from rayforce_amd import hostobj as H


def names_of(c):
    return [f"c{i}" for i in range(len(c["types"]))]


def atom_of(ops, cells, tp):
    return host_atom(ops, int(R.as_bits(np.asarray(cells[:1]))[0]), tp)


def table_obj(ops, c, table):
    return ops.rfx_host_table(H.symbols(names_of(c)), H.list_of([host_vector(ops, cells, tp) for cells, tp in zip(table, c["types"])]))


def batch_obj(ops, c, batch):
    record = c["form"] in ("record", "dict_record")
    vals = [atom_of(ops, cells, c["types"][i]) if record else host_vector(ops, cells, c["types"][i]) for cells, i in zip(batch, c["given"])]
    bnames = [names_of(c)[i] for i in c["given"]]
    if c["form"] in ("list", "record"):
        return H.list_of(vals)
    if c["form"] == "table":
        return ops.rfx_host_table(H.symbols(bnames), H.list_of(vals))
    return ops.rfx_host_dict(H.symbols(bnames), H.list_of(vals))


def vary(ops, verb, args):
    arr = (C.c_void_p * len(args))(*args)
    return (ops.rfx_upsert if verb == "upsert" else ops.rfx_insert)(arr, len(args))


def call(ops, c):
    """-> (the answer, the operands to drop)"""
    table, batch = R.inputs(c)
    t, b = table_obj(ops, c, table), batch_obj(ops, c, batch)
    if c["verb"] == "insert":
        return vary(ops, "insert", [t, b]), [t, b]
    k = ops.rfx_host_i64(c["keys"])
    return vary(ops, "upsert", [t, k, b]), [t, k, b]


def check_door(ops, c):
    r, drop = call(ops, c)
    assert r and not H.is_error(r), (c["name"], H.error_text(r) if r else "null", ops.rfx_ops_last_error().decode())
    assert ops.rfx_last_upsert_on_gpu() == 1, c["name"]
    assert H.header(r).type == H.T_TABLE, c["name"]
    keys, vals = H.list_items(r)
    assert [ops.rfx_host_symbol_name(int(i)).decode() for i in H.to_numpy(keys)] == names_of(c), c["name"]
    cols = H.list_items(vals)
    assert len(cols) == len(c["out"]), c["name"]
    got = [(H.header(o).type, H.header(o).attrs, cells_of(o)) for o in cols]
    for (tp, attrs, cells), want in zip(got, c["out"]):
        same_column(c["name"], tp, attrs, cells, want)
    for o in [r] + drop:
        ops.rfx_host_drop(o)
    return got


def host_call(ops, shape):
    """a `host_` case's call -> the answer (the operands are left alone: some carry type codes the standalone host could not drop)"""
    i64 = lambda n=5, mul=3: host_vector(ops, np.arange(n, dtype=np.int64) * mul + 7, R.I64)  # noqa: E731
    f64 = lambda n=5: host_vector(ops, np.arange(n, dtype=np.float64), R.F64)  # noqa: E731
    typed = lambda tp, n=5: host_vector(ops, np.arange(n).astype(R.DTYPE[tp]), tp)  # noqa: E731
    coded = lambda code: host_vector(ops, np.arange(5, dtype=np.int64), code)  # noqa: E731
    tab = lambda names, cols: ops.rfx_host_table(H.symbols(names), H.list_of(cols))  # noqa: E731
    lst = H.list_of
    k = lambda v=1: ops.rfx_host_i64(v)  # noqa: E731
    t2 = lambda: tab(["a", "b"], [i64(), f64()])  # noqa: E731
    up = lambda *a: vary(ops, "upsert", list(a))  # noqa: E731
    ins = lambda *a: vary(ops, "insert", list(a))  # noqa: E731
    sym = lambda: host_atom(ops, ops.rfx_host_intern(b"t", 1), R.SYMBOL)  # noqa: E731
    sparse = lambda cells: host_vector(ops, np.array(cells, dtype=np.int64), R.I64)  # noqa: E731
    return {
        "quoted_symbol": lambda: up(sym(), k(), lst([i64(), f64()])),
        "insert_quoted_symbol": lambda: ins(sym(), lst([i64(), f64()])),
        "arity": lambda: up(t2(), k()),
        "keys_not_i64": lambda: up(t2(), host_atom(ops, 0, R.F64), lst([i64(), f64()])),
        "keys_zero": lambda: up(t2(), k(0), lst([i64(), f64()])),
        "keys_nine": lambda: up(t2(), k(9), lst([i64(), f64()])),
        "keys_beyond_table": lambda: up(t2(), k(3), lst([i64(), f64()])),
        "key_f64": lambda: up(tab(["a", "b"], [f64(), i64()]), k(), lst([f64(), i64()])),
        "key_i32": lambda: up(tab(["a", "b"], [typed(R.I32), i64()]), k(), lst([typed(R.I32), i64()])),
        "negative_key_hash": lambda: up(tab(["a", "b"], [sparse([5, 1 << 40, 9, 11, 13]), f64()]), k(), lst([sparse([-3, 1 << 40]), f64(2)])),
        "null_key_hash": lambda: up(tab(["a", "b"], [sparse([5, 1 << 40, 9, 11, 13]), f64()]), k(), lst([sparse([R.NULL_I64, 1 << 40]), f64(2)])),
        "f64_into_i64": lambda: up(tab(["a", "b"], [i64(), i64()]), k(), lst([i64(), f64()])),
        "f64_atom_into_i64": lambda: up(tab(["a", "b"], [i64(), i64()]), k(), lst([host_atom(ops, 7, R.I64), host_atom(ops, 0, R.F64)])),
        "list_column": lambda: up(tab(["a", "b"], [i64(), lst([i64(1) for _ in range(5)])]), k(), lst([i64(), f64()])),
        "c8_column": lambda: up(tab(["a", "b"], [i64(), coded(R.C8)]), k(), lst([i64(), f64()])),
        "guid_column": lambda: up(tab(["a", "b"], [i64(), coded(R.GUID)]), k(), lst([i64(), f64()])),
        "enum_column": lambda: up(tab(["a", "b"], [i64(), coded(R.ENUM)]), k(), lst([i64(), f64()])),
        "maplist_column": lambda: up(tab(["a", "b"], [i64(), coded(R.MAPLIST)]), k(), lst([i64(), f64()])),
        "parted": lambda: up(tab(["a", "b"], [coded(77 + R.I64), coded(77 + R.F64)]), k(), lst([i64(), f64()])),
        "matched_i32": lambda: up(tab(["a", "b"], [i64(), typed(R.I32)]), k(), lst([i64(2), typed(R.I32, 2)])),
        "matched_b8_dict_missing": lambda: up(tab(["a", "b", "c"], [i64(), f64(), typed(R.B8)]), k(), ops.rfx_host_dict(H.symbols(["b", "a"]), lst([f64(2), i64(2)]))),
        "date_column": lambda: up(tab(["a", "b"], [i64(), typed(R.DATE)]), k(), lst([i64(2, 100), typed(R.DATE, 2)])),
        "insert_time_column": lambda: ins(tab(["a", "b"], [i64(), typed(R.TIME)]), lst([i64(2), typed(R.TIME, 2)])),
        "u8_column": lambda: up(tab(["a", "b"], [i64(), typed(R.U8)]), k(), lst([i64(2, 100), typed(R.U8, 2)])),
        "insert_record_u8": lambda: ins(tab(["a", "b"], [i64(), typed(R.U8)]), lst([host_atom(ops, 1, R.I64), host_atom(ops, 1, R.U8)])),
        "record_keys2": lambda: up(tab(["a", "b", "c"], [i64(), i64(), f64()]), k(2), lst([host_atom(ops, 7, R.I64), host_atom(ops, 7, R.I64), host_atom(ops, 0, R.F64)])),
        "absent_i32": lambda: up(tab(["a", "b"], [i64(), typed(R.I32)]), k(), lst([i64(2, 100)])),
        "record_dict_absent_i16": lambda: up(tab(["a", "b"], [i64(), typed(R.I16)]), k(), ops.rfx_host_dict(H.symbols(["a"]), lst([host_atom(ops, 1, R.I64)]))),
        "too_many_columns": lambda: up(t2(), k(), lst([i64(), f64(), f64()])),
        "unequal_lengths": lambda: up(t2(), k(), lst([i64(3), f64(2)])),
        "unknown_name": lambda: up(t2(), k(), ops.rfx_host_dict(H.symbols(["a", "z"]), lst([i64(), f64()]))),
        "dict_keys_not_symbols": lambda: up(t2(), k(), ops.rfx_host_dict(i64(2), lst([i64(), f64()]))),
        "batch_vector": lambda: up(t2(), k(), i64()),
        "empty_batch": lambda: up(t2(), k(), lst([i64(0), f64(0)])),
        "not_a_table": lambda: up(i64(), k(), lst([i64(), f64()])),
        "insert_short_list": lambda: ins(t2(), lst([i64()])),
        "insert_empty": lambda: ins(t2(), lst([i64(0), f64(0)])),
        "insert_arity": lambda: ins(t2(), lst([i64(), f64()]), i64()),
        "insert_type": lambda: ins(t2(), lst([i64(), typed(R.I32)])),
    }[shape]()


def check_refused(ops, c):
    """the shape is handed to the host -- there is none behind the standalone door: an error naming the reason"""
    r = host_call(ops, c["shape"])
    assert r and H.is_error(r), c["name"]
    assert ops.rfx_last_upsert_on_gpu() == 0, c["name"]
    assert c["host"] in ops.rfx_ops_last_error().decode(), (c["name"], c["host"], ops.rfx_ops_last_error().decode())
    assert c["verb"] + ":" in ops.rfx_ops_last_error().decode() and "no host function" in H.error_text(r), c["name"]
    ops.rfx_host_drop(r)


def engine_answer(eng, c):
    import torch

    table, batch = R.inputs(c)
    dev = lambda a: torch.from_numpy(np.array(a)).to(eng.device)  # noqa: E731
    t = {nm: dev(cells) for nm, cells in zip(names_of(c), table)}
    if c["form"] in ("list", "record"):
        b = [dev(cells) for cells in batch]
    else:
        b = {names_of(c)[i]: dev(cells) for cells, i in zip(batch, c["given"])}
    got = eng.insert(t, b) if c["verb"] == "insert" else eng.upsert(t, c["keys"], b)
    assert list(got) == names_of(c), c["name"]
    return list(got.values())


def check_engine(eng, c):
    got = engine_answer(eng, c)
    assert len(got) == len(c["out"]), c["name"]
    for g, (wt, _wa, wc) in zip(got, c["out"]):
        assert str(g.dtype) == "torch." + TORCH_OF[wt], (c["name"], g.dtype, wt)
        gb, wb = R.as_bits(g.cpu().numpy()), R.as_bits(wc)
        assert gb.dtype == wb.dtype and gb.shape == wb.shape, (c["name"], gb.dtype, wb.dtype, gb.shape, wb.shape)
        bad = np.flatnonzero(gb != wb)
        assert bad.size == 0, (c["name"], bad[:5], gb[bad[:5]], wb[bad[:5]])
