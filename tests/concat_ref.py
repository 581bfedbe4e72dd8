"""concat (ray_concat, core/compose.c:465-823) and raze (ray_raze, core/compose.c:1096-1164) restated in numpy, and the loader of
tests/golden/concat_golden.npz, the compiled reference's own answers.  These are copies: cells, type code and attributes must agree bit for bit.
Test infrastructure only.

A fixture case: name, verb ("concat" | "raze" | "table"), cols -- per result column its type code and its parts in order, each part a vector's cells or
{"atom": cell} -- names / ynames (a table's column names in x's and in y's order), out -- per result column (type, attrs, cells) as the reference answered
-- or, a `host_` case, `shape` (what to build: HOST_SHAPES) and `host`, the reason the device path names when it hands the shape to the host."""
import json
import os

import numpy as np

B8, U8, I16, I32, I64, SYMBOL, DATE, TIME, TS, F64 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
GUID, C8, ENUM, MAPLIST, LIST, DICT, TABLE = 11, 12, 20, 75, 0, 99, 98
DTYPE = {B8: np.int8, U8: np.uint8, I16: np.int16, I32: np.int32, I64: np.int64, SYMBOL: np.int64, DATE: np.int32, TIME: np.int32, TS: np.int64, F64: np.float64}
TYPES = (B8, U8, I16, I32, DATE, TIME, I64, SYMBOL, TS, F64)
ADOPTED = (I64, SYMBOL, TS, F64, B8)  # result columns that stay resident (rfx_ops_concat.c)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "concat_golden.npz")


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def planes(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return np.ascontiguousarray(a.view(np.uint8).reshape(-1, a.dtype.itemsize).T)


def unplanes(p, tp):
    return np.ascontiguousarray(p.T).reshape(-1).view(DTYPE[tp]).copy()


def part_cells(part, tp):
    """a part's cells: a vector's as they are, an atom's one cell"""
    if isinstance(part, dict):
        return np.array([part["atom"]], dtype=as_bits(np.zeros(1, DTYPE[tp])).dtype).view(DTYPE[tp])
    return np.asarray(part, dtype=DTYPE[tp])


def answer(c):
    """a fixture case -> the answer's columns [(type, attrs, cells)]: every column its parts' cells end to end, the parts' type, attribute byte 0"""
    out = []
    for tp, parts in c["cols"]:
        cells = [part_cells(p, tp) for p in parts]
        out.append((tp, 0, np.concatenate(cells) if cells else np.empty(0, DTYPE[tp])))
    return out


# what a `host_` case builds (tests/concat_door.py host_operands), by name
HOST_SHAPES = ("atom_atom", "types_differ", "vector_atom_types_differ", "c8", "guid", "enum", "list", "dict", "maplist", "parted", "table_vector",
               "names_differ", "names_extra", "col_types_differ", "table_c8_column", "table_parted", "raze_not_list", "raze_empty_list", "raze_mixed_types",
               "raze_atom_element", "raze_list_element", "raze_c8", "device_i32", "device_i16", "device_u8")


def load_cases():
    npz = np.load(GOLDEN)
    blob = npz["blob"]
    arrays = {}
    for line in npz["index"]:  # "key|dtype|shape|offset|bytes": the arrays, cut out of the one blob
        key, *dt, shape, at, nbytes = str(line).split("|")
        arrays[key] = blob[int(at):int(at) + int(nbytes)].view(np.dtype("|".join(dt))).reshape([int(d) for d in shape.split("x")])
    pools = {}

    def pool(key, tp):
        if (key, tp) not in pools:
            pools[(key, tp)] = unplanes(arrays[key], tp)
        return pools[(key, tp)]

    out = []
    for c in json.loads(bytes(npz["cases"]).decode()):
        if c.get("host"):
            out.append(c)
            continue
        cols = []
        for col in c["cols"]:
            tp, p = col["tp"], pool(col["pool"], col["tp"])
            spans = arrays[col["spans"]].reshape(-1, 2)
            parts = [{"atom": int(as_bits(p[s:s + 1])[0])} if j in col["atoms"] else p[s:s + n] for j, (s, n) in enumerate(spans.tolist())]
            cols.append((tp, parts))
        c["cols"] = cols
        c["out"] = [(o["tp"], o["attrs"], unplanes(arrays[o["key"]], o["tp"])) for o in c["out"]]
        out.append(c)
    return out


def retyped(c, frm, to):
    """the same cells under another type code of the same width (SYMBOL: an interned id cannot travel in a fixture)"""
    return dict(c, name=c["name"] + f"_as{to}", cols=[(to if tp == frm else tp, parts) for tp, parts in c["cols"]],
                out=[(to if tp == frm else tp, a, cells) for tp, a, cells in c["out"]])
