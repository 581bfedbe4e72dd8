#!/usr/bin/env python
"""What the operator door decides before it touches a device, recorded from the tree's own librfx.so over the standalone host object model.

    python tests/golden/make_handoff_golden.py     # writes tests/golden/handoff_golden.json

The fixture is the project's own recorded behaviour (tests/test_handoff_cpu.py replays it byte for byte): for every name rfx_host_fn knows the function
object's type code, attribute byte and the exported entry point its pointer equals (names outside the table answer NULL); and a list of calls, in order,
that end before ensure_ctx() -- every verb of the sort, asof, window, set, bucket, rows and cast families and med / dev, every reason of theirs that a call
can reach without a device, the null-argument failures and the answers that need no device -- each with its arguments as plain data
(tests/handoff_door.py), the error text or the answer's type code, attribute byte, length and cells, rfx_ops_last_error(), the family's
rfx_last_*_on_gpu() and the family's own counters.  The calls run in the fixture's order in one process: a call that leaves rfx_ops_last_error() or a
flag alone shows what the call before it left.

Not reachable without a device (they follow ensure_ctx()): every "... over a sharded table / column", "1- and 2-byte keys over shards", "more sort columns
than a sort over shards takes", "device memory" (but take's count past 2^59), "more rows than the device sort takes", "a limit of the sort over shards",
"row-hash collision between two key tuples", asof's second "too many columns", the set verbs' planner messages (the only reasons long enough for their
%.300s), filter's and take's scratch / upload / planner limits, the cast's "a column the residency cache does not take", and med / dev's "sharded columns",
"parted / window index", "group ids", "source column", "empty key table", "group count of the index does not match its rows".  No reason reachable here is
longer than the smallest message buffer (256 bytes): they are all short literals."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import handoff_door as D  # noqa: E402
from rayforce_amd import hostobj as H  # noqa: E402

B8, U8, I16, I32, I64, SYM, DATE, TIME, TS, F64 = range(1, 11)
ASC, DESC, DISTINCT = 2, 4, 1
NAMES = ["sum", "avg", "min", "max", "count", "first", "==", "!=", "<", ">", "<=", ">=", "and", "or", "select", "+", "-", "*", "div", "/", "%", "xbar", "update",
         "med", "dev", "iasc", "idesc", "asc", "desc", "rank", "xasc", "xdesc", "asof-join", "bin", "binr", "window-join", "window-join1", "last", "distinct",
         "find", "in", "sect", "except", "union", "xrank", "floor", "ceil", "round", "neg", "filter", "take", "reverse", "as"]
UNKNOWN = ["within", "not", "left-join", "inner-join", "where", "at", "group", "pin", "nosuchverb", "", "SUM", "ray_sum", "rfx_sum", "fdiv"]


def vec(tp, cells=(), attrs=0):
    return {"vec": tp, "cells": list(cells), "attrs": attrs}


def atom(tp, v):
    return {"atom": tp, "v": v}


def sym(name, attrs=0):
    return {"sym": name, "attrs": attrs}


def table(*cols):
    return {"table": [[n, c] for n, c in cols]}


def lst(*items, **kw):
    return {"list": list(items), **kw}


def cases():
    out = []

    def add(name, verb, *args, **kw):
        out.append({"name": name, "verb": verb, "args": None if kw.get("null_args") else list(args), **({"n": kw["n"]} if "n" in kw else {})})

    i64 = vec(I64, [3, 1, 2])
    parted = table(("k", lst(vec(I64, [1]), type=77 + I64)))
    # ---- the sort's five vector verbs ----
    for v in ("iasc", "idesc", "asc", "desc", "rank"):
        add(f"{v}_key_type_symbol", v, vec(SYM, [0, 1]))
        add(f"{v}_null", v, None)
        add(f"{v}_key_type_atom", v, atom(I64, 5))
        add(f"{v}_key_type_list", v, lst(i64))
        add(f"{v}_device_i32", v, {"device": I32, "len": 4})
        add(f"{v}_device_i16", v, {"device": I16, "len": 4})
        for tp in (B8, U8, I16, I32, I64, DATE, TIME, TS, F64):
            add(f"{v}_empty_{tp}", v, vec(tp))
        add(f"{v}_empty_distinct", v, vec(I64, [], DISTINCT))
        for nm, attrs in (("asc", ASC), ("desc", DESC), ("asc_distinct", ASC | DISTINCT), ("both", ASC | DESC)):
            add(f"{v}_of_{nm}_i64", v, vec(I64, [1, 2, 5], attrs))
            add(f"{v}_of_{nm}_i16", v, vec(I16, [1, 2, 5], attrs))
        add(f"{v}_of_asc_f64", v, vec(F64, [0.5, 1.5], ASC))
        add(f"{v}_of_desc_u8", v, vec(U8, [9, 7, 200], DESC))
        add(f"{v}_of_desc_i32", v, vec(I32, [9, 7, -2], DESC))
        add(f"{v}_of_asc_empty", v, vec(TS, [], ASC))
    # ---- xasc / xdesc ----
    t2 = table(("a", i64), ("b", vec(F64, [1.0, 2.0, 3.0])))
    for v in ("xasc", "xdesc"):
        add(f"{v}_not_a_table", v, i64, sym("a"))
        add(f"{v}_null_table", v, None, sym("a"))
        add(f"{v}_null_names", v, t2, None)
        add(f"{v}_empty_symbols", v, t2, {"syms": []})
        add(f"{v}_empty_i64", v, t2, vec(I64))
        add(f"{v}_names_not_symbols", v, t2, vec(I64, [1]))
        add(f"{v}_names_are_a_list", v, t2, lst(sym("a")))
        add(f"{v}_parted", v, parted, sym("k"))
        add(f"{v}_17_names", v, t2, {"syms": ["a"] * 17})
        add(f"{v}_65_columns", v, table(*[(f"c{i}", vec(I64, [i])) for i in range(65)]), sym("c0"))
        add(f"{v}_no_columns", v, table(), sym("a"))
        add(f"{v}_i32_column", v, table(("a", i64), ("n", vec(I32, [1, 2, 3]))), sym("a"))
        add(f"{v}_unequal_columns", v, table(("a", i64), ("b", vec(I64, [1]))), sym("a"))
        add(f"{v}_no_such_column", v, t2, sym("zz"))
        add(f"{v}_no_such_column_2", v, t2, {"syms": ["a", "zz"]})
        add(f"{v}_symbol_key", v, table(("s", vec(SYM, [0, 1, 0])), ("a", i64)), sym("s"))
    # ---- asof-join ----
    lt = table(("s", vec(I64, [1, 2])), ("t", vec(I32, [10, 20])), ("p", vec(F64, [1.0, 2.0])))
    rt = table(("s", vec(I64, [1, 2, 1])), ("t", vec(I32, [5, 6, 7])), ("q", vec(I64, [7, 8, 9])))
    keys = {"syms": ["s", "t"]}
    aj = "asof_join"
    add("aj_two_arguments", aj, keys, lt)
    add("aj_null_array", aj, null_args=True, n=3)
    add("aj_null_argument", aj, keys, None, rt)
    add("aj_keys_not_symbols", aj, vec(I64, [1, 2]), lt, rt)
    add("aj_left_not_a_table", aj, keys, i64, rt)
    add("aj_one_key_name", aj, {"syms": ["t"]}, lt, rt)
    add("aj_parted", aj, {"syms": ["k", "k"]}, parted, rt)
    add("aj_ten_keys", aj, {"syms": ["s"] * 9 + ["t"]}, lt, rt)
    add("aj_asof_column_missing", aj, {"syms": ["s", "zz"]}, lt, rt)
    add("aj_asof_types_differ", aj, keys, lt, table(("s", vec(I64, [1])), ("t", vec(I64, [5]))))
    add("aj_asof_column_f64", aj, {"syms": ["s", "p"]}, lt, table(("s", vec(I64, [1])), ("p", vec(F64, [5.0]))))
    add("aj_key_missing", aj, {"syms": ["zz", "t"]}, lt, rt)
    add("aj_key_f64", aj, {"syms": ["p", "t"]}, lt, table(("p", vec(F64, [1.0])), ("t", vec(I32, [5]))))
    add("aj_key_types_differ", aj, keys, lt, table(("s", vec(TS, [1])), ("t", vec(I32, [5]))))
    add("aj_left_passenger_i32", aj, keys, table(("s", vec(I64, [1])), ("t", vec(I32, [10])), ("n", vec(I32, [1]))), rt)
    add("aj_right_passenger_b8", aj, keys, lt, table(("s", vec(I64, [1])), ("t", vec(I32, [5])), ("m", vec(B8, [1]))))
    add("aj_left_lengths", aj, keys, table(("s", vec(I64, [1, 2])), ("t", vec(I32, [10, 20])), ("p", vec(F64, [1.0]))), rt)
    add("aj_right_lengths", aj, keys, lt, table(("s", vec(I64, [1, 2])), ("t", vec(I32, [5, 6])), ("q", vec(I64, [7]))))
    add("aj_column_types_differ", aj, keys, lt, table(("s", vec(I64, [1])), ("t", vec(I32, [5])), ("p", vec(I64, [7]))))
    add("aj_64_columns", aj, keys, table(("s", vec(I64, [1])), ("t", vec(I32, [10])), *[(f"c{i}", vec(I64, [i])) for i in range(62)]), rt)
    # ---- bin / binr ----
    for v in ("bin", "binr"):
        add(f"{v}_types_differ", v, i64, vec(TS, [1]))
        add(f"{v}_null", v, None, i64)
        add(f"{v}_f64", v, vec(F64, [1.0]), vec(F64, [1.0]))
        add(f"{v}_atom", v, i64, atom(I64, 2))
        add(f"{v}_empty_right", v, i64, vec(I64))
        add(f"{v}_empty_right_ts", v, vec(TS, [1]), vec(TS))
    # ---- window-join / window-join1 ----
    wl = table(("s", vec(I64, [1, 2])), ("t", vec(TIME, [10, 20])))
    wr = table(("s", vec(I64, [1, 2, 1])), ("t", vec(TIME, [5, 6, 7])), ("q", vec(I64, [7, 8, 9])), ("f", vec(F64, [0.5, 1.5, 2.5])), ("n", vec(I32, [1, 2, 3])))
    wins = lst(vec(TIME, [0, 10]), vec(TIME, [15, 25]))

    def aggs(*pairs):
        return {"dict": [{"syms": [n for n, _ in pairs]}, lst(*[e for _, e in pairs])]}

    ok = aggs(("m", lst({"fn": "max"}, sym("q"))), ("c", lst(sym("count"), sym("f"))))
    for v in ("window_join", "window_join1"):
        w = "wj" if v == "window_join" else "wj1"
        add(f"{w}_four_arguments", v, keys, wins, wl, wr)
        add(f"{w}_null_array", v, null_args=True, n=5)
        add(f"{w}_null_argument", v, keys, wins, wl, wr, None)
        add(f"{w}_windows_not_a_list", v, keys, i64, wl, wr, ok)
        add(f"{w}_aggregates_not_a_dict", v, keys, wins, wl, wr, wl)
        add(f"{w}_one_key_name", v, {"syms": ["t"]}, wins, wl, wr, ok)
        add(f"{w}_parted", v, {"syms": ["k", "k"]}, wins, parted, wr, ok)
        add(f"{w}_ten_keys", v, {"syms": ["s"] * 9 + ["t"]}, wins, wl, wr, ok)
        add(f"{w}_window_column_missing", v, {"syms": ["s", "zz"]}, wins, wl, wr, ok)
        add(f"{w}_window_types_differ", v, keys, wins, wl, table(("s", vec(I64, [1])), ("t", vec(I32, [5]))), ok)
        add(f"{w}_window_column_i64", v, {"syms": ["t", "s"]}, wins, wl, wr, ok)
        add(f"{w}_key_missing", v, {"syms": ["zz", "t"]}, wins, wl, wr, ok)
        add(f"{w}_key_f64", v, {"syms": ["f", "t"]}, wins, table(("f", vec(F64, [1.0])), ("t", vec(TIME, [1]))), wr, ok)
        add(f"{w}_left_lengths", v, keys, wins, table(("s", vec(I64, [1, 2])), ("t", vec(TIME, [10, 20])), ("x", vec(I64, [1]))), wr, ok)
        add(f"{w}_right_lengths", v, keys, wins, wl, table(("s", vec(I64, [1, 2])), ("t", vec(TIME, [5, 6])), ("q", vec(I64, [7]))), ok)
        add(f"{w}_three_windows", v, keys, lst(vec(TIME, [0, 10]), vec(TIME, [15, 25]), vec(TIME, [1, 2])), wl, wr, ok)
        add(f"{w}_windows_i64", v, keys, lst(vec(I64, [0, 10]), vec(I64, [15, 25])), wl, wr, ok)
        add(f"{w}_windows_short", v, keys, lst(vec(TIME, [0]), vec(TIME, [15])), wl, wr, ok)
        add(f"{w}_dict_keys_not_symbols", v, keys, wins, wl, wr, {"dict": [vec(I64, [1]), lst(lst({"fn": "max"}, sym("q")))]})
        add(f"{w}_dict_lengths", v, keys, wins, wl, wr, {"dict": [{"syms": ["m", "c"]}, lst(lst({"fn": "max"}, sym("q")))]})
        add(f"{w}_65_aggregates", v, keys, wins, wl, wr, aggs(*[(f"a{i}", lst({"fn": "sum"}, sym("q"))) for i in range(65)]))
        add(f"{w}_raw_column", v, keys, wins, wl, wr, aggs(("m", sym("q"))))
        add(f"{w}_three_cell_expression", v, keys, wins, wl, wr, aggs(("m", lst({"fn": "max"}, sym("q"), sym("f")))))
        add(f"{w}_med_aggregate", v, keys, wins, wl, wr, aggs(("m", lst({"fn": "med"}, sym("q")))))
        add(f"{w}_dev_by_name", v, keys, wins, wl, wr, aggs(("m", lst(sym("dev"), sym("q")))))
        add(f"{w}_aggregate_of_an_expression", v, keys, wins, wl, wr, aggs(("m", lst({"fn": "max"}, lst({"fn": "+"}, sym("q"), atom(I64, 1))))))
        add(f"{w}_aggregate_of_a_quoted_symbol", v, keys, wins, wl, wr, aggs(("m", lst({"fn": "max"}, sym("q", 8)))))
        add(f"{w}_aggregate_of_a_missing_column", v, keys, wins, wl, wr, aggs(("m", lst({"fn": "last"}, sym("zz")))))
        add(f"{w}_aggregate_of_an_i32_column", v, keys, wins, wl, wr, aggs(("m", lst({"fn": "first"}, sym("n")))))
        wide = table(("s", vec(I64, [1])), ("t", vec(TIME, [5])), *[(f"v{i}", vec(I64, [i])) for i in range(17)])
        add(f"{w}_17_aggregated_columns", v, keys, wins, wl, wide, aggs(*[(f"a{i}", lst({"fn": "avg"}, sym(f"v{i}"))) for i in range(17)]))
        empty_left = table(("s", vec(I64)), ("t", vec(TIME)))
        add(f"{w}_empty_left", v, keys, lst(vec(TIME), vec(TIME)), empty_left, wr,
            aggs(("m", lst({"fn": "max"}, sym("q"))), ("c", lst(sym("count"), sym("f"))), ("a", lst({"fn": "avg"}, sym("q"))), ("l", lst({"fn": "last"}, sym("f")))))
    # ---- the set verbs ----
    add("distinct_f64", "distinct", vec(F64, [1.0]))
    add("distinct_null", "distinct", None)
    add("distinct_atom", "distinct", atom(I64, 1))
    add("distinct_i32", "distinct", vec(I32, [1]))
    for v in ("find", "in", "sect", "except", "union"):
        add(f"{v}_first_f64", v, vec(F64, [1.0]), i64)
        add(f"{v}_null_x", v, None, i64)
        add(f"{v}_null_y", v, i64, None)
        add(f"{v}_types_differ", v, i64, vec(SYM, [0]))
        add(f"{v}_atom_y", v, i64, atom(I64, 1))  # (except takes the atom: its call goes on to the device)
        add(f"{v}_timestamps_i64", v, vec(TS, [1]), i64)
        if v in ("sect", "except"):
            add(f"{v}_timestamps", v, vec(TS, [1]), vec(TS, [1]))
    out[:] = [c for c in out if c["name"] != "except_atom_y"]
    # ---- the bucket verbs ----
    add("xrank_count_f64", "xrank", i64, atom(F64, 2.0))
    add("xrank_null", "xrank", None, atom(I64, 2))
    add("xrank_null_count", "xrank", i64, None)
    add("xrank_count_vector", "xrank", i64, vec(I64, [2]))
    for tp, nm in ((I64, "i64"), (I32, "i32"), (I16, "i16"), (U8, "u8")):
        add(f"xrank_zero_{nm}", "xrank", i64, atom(tp, 0))
        add(f"xrank_i32_keys_count_{nm}", "xrank", vec(I32, [1, 2]), atom(tp, 2))
        add(f"xrank_empty_count_{nm}", "xrank", vec(F64), atom(tp, 3))
    add("xrank_negative", "xrank", i64, atom(I64, -4))
    add("xrank_symbol_keys", "xrank", vec(SYM, [0, 1]), atom(I64, 2))
    add("xrank_atom_keys", "xrank", atom(I64, 1), atom(I64, 2))
    add("xrank_63_bits", "xrank", i64, atom(I64, 2**62))
    add("xbar_atoms", "xbar", atom(I64, 7), atom(I64, 2))
    add("xbar_null_x", "xbar", None, atom(I64, 2))
    add("xbar_null_y", "xbar", i64, None)
    add("xbar_symbol", "xbar", vec(SYM, [0]), atom(I64, 2))
    add("xbar_b8_atom", "xbar", i64, atom(B8, 1))
    add("xbar_lengths", "xbar", i64, vec(I64, [1, 2]))
    add("xbar_device_i32", "xbar", {"device": I32, "len": 3}, atom(I64, 2))
    add("xbar_device_time_y", "xbar", atom(I64, 2), {"device": TIME, "len": 3})
    for v in ("floor", "ceil", "round"):
        add(f"{v}_atom", v, atom(F64, 1.5))
        add(f"{v}_null", v, None)
        add(f"{v}_i64", v, i64)
        add(f"{v}_i64_atom", v, atom(I64, 1))
    add("neg_atom", "neg", atom(I64, 1))
    add("neg_null", "neg", None)
    add("neg_timestamp", "neg", vec(TS, [1]))
    add("neg_device_i32", "neg", {"device": I32, "len": 3})
    add("within_f64", "within", vec(F64, [1.0]), vec(I64, [0, 2]))
    add("within_null", "within", None, vec(I64, [0, 2]))
    add("within_null_y", "within", i64, None)
    add("within_three_bounds", "within", i64, vec(I64, [0, 2, 3]))
    add("within_atom", "within", atom(I64, 1), vec(I64, [0, 2]))
    add("within_device_bounds", "within", i64, {"device": I64, "len": 2})
    # ---- the row verbs ----
    mask = vec(B8, [1, 0, 1])
    add("filter_u8", "filter", vec(U8, [1, 2, 3]), mask)
    add("filter_null", "filter", None, mask)
    add("filter_null_mask", "filter", i64, None)
    add("filter_parted", "filter", parted, mask)
    add("filter_no_columns", "filter", table(), mask)
    add("filter_table_i16_column", "filter", table(("a", i64), ("h", vec(I16, [1, 2, 3]))), mask)
    add("filter_atom", "filter", atom(I64, 1), mask)
    add("filter_device_i32", "filter", {"device": I32, "len": 3}, mask)
    add("filter_unequal_columns", "filter", table(("a", i64), ("b", vec(I64, [1]))), mask)
    add("filter_mask_i64", "filter", i64, i64)
    add("filter_mask_length", "filter", i64, vec(B8, [1]))
    for tp in (B8, I32, I64, SYM, DATE, TIME, TS, F64):
        add(f"filter_empty_{tp}", "filter", vec(tp, [], ASC if tp == I64 else 0), vec(B8))
    add("filter_empty_table", "filter", table(("a", vec(I64)), ("f", vec(F64)), ("d", vec(DATE)), ("m", vec(B8))), vec(B8))
    add("take_negative_amount", "take", i64, vec(I64, [0, -1]))
    add("take_null", "take", None, atom(I64, 1))
    add("take_null_count", "take", i64, None)
    add("take_range_overflows", "take", i64, vec(I64, [2**63 - 1, 5]))
    add("take_clamped_range_overflows", "take", i64, vec(I64, [-1, 2**63 - 1]))
    add("take_count_f64", "take", i64, atom(F64, 1.0))
    add("take_count_u8", "take", i64, atom(U8, 1))
    add("take_count_three_cells", "take", i64, vec(I64, [0, 1, 2]))
    add("take_count_int64_min", "take", i64, atom(I64, -2**63))
    add("take_u8_atom", "take", atom(U8, 1), atom(I64, 2))
    add("take_atom_too_many", "take", atom(I64, 1), atom(I64, 2**60))
    for tp in (B8, I32, I64, F64):
        add(f"take_atom_none_{tp}", "take", atom(tp, 1), atom(I32 if tp == B8 else I16 if tp == I32 else I64, 0))
    add("take_atom_empty_range", "take", atom(TS, 1), vec(I64, [4, 0]))
    add("take_from_u8", "take", vec(U8, [1]), atom(I64, 1))
    add("take_from_parted", "take", parted, atom(I64, 1))
    add("take_from_table_with_a_list", "take", table(("a", lst(i64))), atom(I64, 1))
    add("take_from_device_date", "take", {"device": DATE, "len": 3}, atom(I64, 1))
    add("take_from_empty_vector", "take", vec(I64), atom(I64, 2))
    add("take_from_empty_table", "take", table(("a", vec(I64))), atom(I64, -2))
    add("take_none_of_a_vector", "take", i64, atom(I64, 0))
    add("take_none_of_a_table", "take", table(("a", i64), ("d", vec(DATE, [1, 2, 3]))), atom(I16, 0))
    add("take_empty_range_of_a_vector", "take", vec(F64, [1.0, 2.0], ASC), vec(I64, [5, 3]))
    add("take_empty_range_of_an_empty_table", "take", table(("a", vec(I64))), vec(I64, [0, 3]))
    add("take_too_many", "take", i64, atom(I64, 2**60))
    add("reverse_table", "reverse", table(("a", i64)))
    add("reverse_null", "reverse", None)
    add("reverse_u8", "reverse", vec(U8, [1]))
    add("reverse_atom", "reverse", atom(I64, 1))
    add("reverse_device_time", "reverse", {"device": TIME, "len": 3})
    for tp, attrs in ((I64, ASC), (F64, DESC | DISTINCT), (B8, 0), (DATE, ASC | DESC), (SYM, DISTINCT)):
        add(f"reverse_empty_{tp}", "reverse", vec(tp, [], attrs))
    # ---- as ----
    add("as_name_not_a_symbol", "as", atom(I64, 5), i64)
    add("as_null_name", "as", None, i64)
    add("as_null_x", "as", sym("i64"), None)
    add("as_name_vector", "as", {"syms": ["i64"]}, i64)
    add("as_unknown_name", "as", sym("nosuchtype"), i64)
    add("as_guid_name", "as", sym("guid"), i64)
    add("as_symbol_name", "as", sym("symbol"), i64)
    add("as_atom", "as", sym("f64"), atom(I64, 5))
    add("as_symbol_vector", "as", sym("I64"), vec(SYM, [0]))
    add("as_list", "as", sym("I64"), lst(i64))
    add("as_device_i32", "as", sym("I64"), {"device": I32, "len": 3})
    add("as_device_u8", "as", sym("I64"), {"device": U8, "len": 3})
    add("as_same_type", "as", sym("I64"), vec(I64, [3, 1, 2], ASC))
    add("as_same_type_atom_spelling", "as", sym("f64"), vec(F64, [0.5]))
    add("as_same_type_empty", "as", sym("date"), vec(DATE, [], DESC))
    add("as_same_type_device", "as", sym("I64"), {"device": I64, "len": 3})
    for st, name in ((I64, "F64"), (F64, "i16"), (B8, "U8"), (U8, "b8"), (I16, "timestamp"), (TIME, "DATE")):
        add(f"as_empty_{st}_{name}", "as", sym(name), vec(st, [], ASC))
    add("as_b8_to_u8", "as", sym("U8"), vec(B8, [1, 0]))
    add("as_u8_to_b8", "as", sym("b8"), vec(U8, [1, 0]))
    # ---- med / dev ----
    mf = lst(i64, vec(F64, [0.0]), type=71)
    add("med_f64", "med", vec(F64, [1.0]))
    add("med_null", "med", None)
    add("med_timestamp", "med", vec(TS, [1]))
    add("med_mapfilter_f64_values", "med", lst(vec(F64, [1.0]), vec(I64, [0]), type=71))
    add("med_mapfilter_f64_ids", "med", mf)
    add("med_mapgroup_symbol_values", "med", lst(vec(SYM, [0]), lst(), type=72))
    add("dev_symbol", "dev", vec(SYM, [0]))
    add("dev_null", "dev", None)
    add("dev_timestamp", "dev", vec(TS, [1]))
    add("dev_mapfilter_timestamp_values", "dev", lst(vec(TS, [1]), vec(I64, [0]), type=71))
    add("dev_mapfilter_f64_ids", "dev", mf)
    add("dev_mapgroup_b8_values", "dev", lst(vec(B8, [1]), lst(), type=72))
    return out


def main():
    ops = H.lib()
    ops.rfx_host_bind()
    by_address = D.exported(ops)
    fns = {n: D.fn_record(ops, n, by_address) for n in NAMES}
    assert all(r and r[2] for r in fns.values()), [n for n, r in fns.items() if not (r and r[2])]
    unknown = {n: D.fn_record(ops, n, by_address) for n in UNKNOWN}
    assert all(r is None for r in unknown.values()), unknown
    calls = []
    for c in cases():
        rec = D.run_case(ops, c)
        text = json.dumps(rec)
        assert "no usable MI355X" not in text and "HIP" not in text, (c["name"], rec)  # a case that reached ensure_ctx() does not belong here
        calls.append({**c, "record": rec})
    assert len({c["name"] for c in calls}) == len(calls)
    path = os.path.join(HERE, "handoff_golden.json")
    with open(path, "w") as f:
        f.write('{"functions": ' + json.dumps(fns) + ',\n "unknown": ' + json.dumps(unknown) + ',\n "calls": [\n  ' + ",\n  ".join(json.dumps(c) for c in calls) + "\n ]}\n")
    reasons = sorted({c["record"]["answer"].get("error", "") for c in calls})
    print("wrote", len(fns), "names,", len(calls), "calls,", len(reasons), "distinct error texts,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2**20


if __name__ == "__main__":
    main()
