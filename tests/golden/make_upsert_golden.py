#!/usr/bin/env python
"""Golden upsert and insert from the compiled reference -- build container only.

    python tests/golden/make_upsert_golden.py     # writes tests/golden/upsert_golden.npz

Every case is a Rayfall script run by the reference BINARY (oracle/ref.py Session): the table's and the batch's columns go in as column files carrying
their type codes, the table is (table [names] (list columns)), the batch a (list ...) of vectors, a (list ...) of (first v) atoms (one record), a
(dict [names] (list ...)) or a (table ...) in the case's own name order, and (upsert t keys batch) / (insert t batch) is evaluated; every column of the
answer comes back as a column file whose header gives its type code and attributes.  Each case runs with one thread and with eight; only cases on which
the two runs agree (and the reference answers with plain vectors of the columns' types) are kept, the others are printed.  A SYMBOL column cannot travel as
a file: the tests run an I64 case once more under the SYMBOL type code, held to the restatement.  A `host_` case is an input only (tests/upsert_ref.py
HOST_SHAPES).

The inputs are arithmetic in the row number and are made by tests/upsert_ref.py inputs(): the fixture holds the cases' descriptions and the answers' cells
as byte planes in one `blob` that `index` lines "key|dtype|shape|offset|bytes" cut up."""
import json
import os
import struct
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
import upsert_ref as R  # noqa: E402
from upsert_ref import B8, U8, I16, I32, I64, DATE, TIME, TS, F64, DTYPE, BIG  # noqa: E402

WIDE = [I64, F64, I64, TS, F64]  # what a matched row may write: set_idx knows 8-byte cells only (core/rayforce.c:1399-1435)
MIX = [I64, F64, I32, I16, B8]   # a value column of every width class: appended rows only
NINE = [I64, F64, I64, TS, F64, TS, I64, F64, I64]
NINE_MIX = [I64, F64, I32, I16, B8, I64, TS, B8, I32]


def cases():
    out = []

    def case(name, verb="upsert", keys=1, form="list", types=WIDE, n=4097, m=1025, pattern="alt", given=None, **kw):
        out.append(dict(name=name, verb=verb, keys=keys if verb == "upsert" else 0, form=form, types=list(types), n=n, m=m, pattern=pattern,
                        given=list(range(len(types))) if given is None else list(given), **kw))

    # the scan at lane, wave, block and grid edges; the table at nothing, one row, one wave, several tiles and beyond 2^20
    for n in (0, 1, 64, 4097, BIG):
        for m in (1, 63, 64, 65, 1025, 4097):
            case(f"grid_n{n}_m{m}", types=[I64, F64] if n == BIG else (MIX if n == 0 else WIDE), n=n, m=m)
    for pattern in ("all", "none", "runs", "dups", "newdups"):
        case(f"pattern_{pattern}", m=6000 if pattern == "runs" else 4097, pattern=pattern)
    case("none_every_width", types=MIX, m=4097, pattern="none")
    case("table_dups", pattern="all", tdup=1)
    case("sparse_keys", sparse=1)
    case("sparse_keys_dups", sparse=1, m=4097, pattern="dups")
    case("keys2", keys=2, types=[I64, TS, F64, I64], pattern="dups", m=4097)
    case("keys2_ts_first", keys=2, types=[TS, I64, F64, TS])
    case("keys3", keys=3, types=[I64, TS, I64, F64, TS], pattern="dups", m=4097)
    case("keys3_newdups", keys=3, types=[TS, TS, I64, I64], pattern="newdups")
    case("keys2_none_every_width", keys=2, types=[I64, TS, I32, I16, B8, F64], pattern="none")
    case("ts_key", types=[TS, F64, I64])
    case("nine_columns", types=NINE, n=513, m=65)
    case("nine_columns_dups", types=NINE, n=4097, m=4097, pattern="dups")
    case("nine_columns_none_every_width", types=NINE_MIX, n=513, m=4097, pattern="none")
    case("short_list", types=[I64, F64, I64, B8, TS, F64], given=[0, 1])
    case("short_list_keys_only", types=[I64, F64], given=[0])
    case("short_list_dups", types=[I64, F64, I64, F64], given=[0, 1, 2], pattern="dups", m=4097)
    case("dict_shuffled_missing", form="dict", given=[3, 0, 1])
    case("table_shuffled_missing", form="table", given=[4, 1, 0, 2])
    case("dict_keys2_missing", form="dict", keys=2, types=[I64, TS, F64, I64], given=[1, 3, 0])
    case("dict_none_missing_every_width", form="dict", types=MIX, given=[1, 0], pattern="none")
    for pattern in ("all", "none"):
        case(f"record_{pattern}", form="record", types=[I64, F64, I64, TS], m=1, pattern=pattern)
        case(f"record_short_{pattern}", form="record", types=[I64, F64, I64], m=1, pattern=pattern, given=[0, 1])
        case(f"record_dict_{pattern}", form="dict_record", types=[I64, F64, I64], m=1, pattern=pattern, given=[2, 0])
    case("record_none_every_width", form="record", types=MIX, m=1, pattern="none")
    case("insert_list", verb="insert", types=MIX, pattern="none", m=65)
    case("insert_list_big_batch", verb="insert", pattern="none", n=64, m=4097, types=[I64, F64, I32, I16, B8, U8, I64, TS, F64])
    case("insert_into_empty", verb="insert", types=MIX, pattern="none", n=0, m=65)
    case("insert_dict", verb="insert", form="dict", types=MIX + [U8], pattern="none", m=65, given=[2, 0, 4])
    case("insert_table", verb="insert", form="table", types=MIX, pattern="none", m=1025, given=[4, 3, 2, 1, 0])
    case("insert_record", verb="insert", form="record", types=MIX, pattern="none", m=1)
    case("insert_record_dict", verb="insert", form="dict_record", pattern="none", types=[I64, F64, I64, B8], m=1, given=[1, 0])
    return out


def read_file(path, want):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    if tp != want:
        raise ValueError(f"a column of type {want} came back with type code {tp}")
    return np.frombuffer(body, DTYPE[tp], n).copy(), tp, attrs


def run_case(c, threads):
    table, batch = R.inputs(c)
    names = [f"c{i}" for i in range(len(c["types"]))]
    with ref.Session() as s:
        for i, cells in enumerate(table):
            s.put(f"t{i}", cells, tp=c["types"][i])
        for k, (cells, i) in enumerate(zip(batch, c["given"])):
            s.put(f"b{k}", cells, tp=c["types"][i])
        s.eval(f"(set t (table [{' '.join(names)}] (list {' '.join(f't{i}' for i in range(len(names)))})))")
        record = c["form"] in ("record", "dict_record")
        vals = " ".join(f"(first b{k})" if record else f"b{k}" for k in range(len(batch)))
        bnames = " ".join(names[i] for i in c["given"])
        if c["form"] in ("list", "record"):
            s.eval(f"(set b (list {vals}))")
        elif c["form"] == "table":
            s.eval(f"(set b (table [{bnames}] (list {vals})))")
        else:
            s.eval(f"(set b (dict [{bnames}] (list {vals})))")
        s.eval(f"(set r (upsert t {c['keys']} b))" if c["verb"] == "upsert" else "(set r (insert t b))")
        for j, nm in enumerate(names):
            s.out(f"o{j}", f"(at r '{nm})")
        ref.run_script("\n".join(s.lines) + "\n", threads=threads)
        return [read_file(os.path.join(s.dir, f"out_o{j}"), c["types"][j]) for j in range(len(names))]


def record(c):
    try:
        one, eight = run_case(c, 1), run_case(c, 8)
    except (RuntimeError, KeyError, ValueError, FileNotFoundError) as e:
        return None, f"the reference does not answer it: {str(e)[:300]}"
    if any(a[1:] != b[1:] or a[0].tobytes() != b[0].tobytes() for a, b in zip(one, eight)):
        return None, "1 and 8 threads differ"
    return one, None


def main():
    assert ref.build() or ref.available()
    cs = cases()
    with ThreadPoolExecutor(4) as ex:
        got = list(ex.map(record, cs))
    arrays, kept = {}, []
    for k, (c, (outs, why)) in enumerate(zip(cs, got)):
        if outs is None:
            print("dropped", c["name"], "--", why)
            continue
        c["out"] = []
        for j, (a, tp, attrs) in enumerate(outs):
            arrays[f"c{k}_o{j}"] = R.planes(a)
            c["out"].append(dict(tp=int(tp), attrs=int(attrs), key=f"c{k}_o{j}"))
        c["threads"] = "1,8"
        kept.append(c)
    kept += [dict(name=f"host_{sh}", verb=v, shape=sh, host=why) for sh, (v, why) in R.HOST_SHAPES.items()]
    index, parts, at = [], [], 0
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        index.append(f"{key}|{a.dtype.str}|{'x'.join(str(d) for d in a.shape)}|{at}|{a.nbytes}")
        parts.append(a.reshape(-1).view(np.uint8))
        at += a.nbytes
    path = os.path.join(HERE, "upsert_golden.npz")
    np.savez_compressed(path, cases=np.frombuffer(json.dumps(kept).encode(), np.uint8), index=np.array(index), blob=np.concatenate(parts))
    print("wrote", len(kept), "cases of", len(cs) + len(R.HOST_SHAPES), ",", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2**20


if __name__ == "__main__":
    main()
