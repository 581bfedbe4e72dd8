#!/usr/bin/env python
"""Golden nested select columns from the compiled reference -- build container only.

    python tests/golden/make_collect_golden.py     # writes tests/golden/collect_golden.npz

Every case of tests/collect_ref.py cases() is a Rayfall script run by the reference BINARY (oracle/ref.py Session): the table's columns go in as column
files carrying their type codes, the query is (select {... by: k from: t [where: ...]}) with bare columns, (row vi) and sum / count / first side by side, and
the answer comes back column by column: the key and the aggregates as they are; a LIST column cannot travel as a column file, so it comes back as
(raze (at r 'p)), its cells laid end to end, with the groups' lengths as (map count ...) of it -- and, where the query has aggregates, the grouped count
beside it.  A query that selects no row answers a table of no rows: its LIST columns have nothing to raze, the key column alone is read.
Each case runs with one thread and with eight.  Both reference functions are sequential, so every group's vectors must agree; the ORDER of the groups is
the group index's, and the reference's multi-threaded grouping orders many groups under where: by its workers' chunks: where the two runs differ in that
order alone (every key's cells, rows and aggregates equal -- checked here), the one-thread answer is kept, as the other fixtures keep the one-executor
order, and the case is flagged `order_differs_with_8_threads`.  Inputs are arithmetic in the row number
(collect_ref.case_table) and are not stored; of every answer column the fixture keeps dtype, length and sha-256 (collect_ref.digest) -- data only.  Every
case of the list is kept: one the reference does not answer, or answers differently with 1 and 8 threads, is recorded under `failed` with what happened."""
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
import collect_ref as R  # noqa: E402

DTYPE = {1: np.int8, 2: np.uint8, 3: np.int16, 4: np.int32, 5: np.int64, 6: np.int64, 7: np.int32, 8: np.int32, 9: np.int64, 10: np.float64}


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    return np.frombuffer(body, DTYPE[tp], n).copy(), int(tp), int(attrs)


def run_case(c, threads):
    t = R.case_table(c)
    empty = c["n"] == 0 or c["where"] == "none"
    with ref.Session() as s:
        for name, col in t.items():
            s.put(name, col, tp=R.TYPE_CODE[name[2:]] if name.startswith("v_") else None)
        s.eval(f"(set t (table [{' '.join(t)}] (list {' '.join(t)})))")
        maps = R.case_mappings(c)
        where = f" where: {R.WHERES[c['where']]}" if c["where"] else ""
        s.eval("(set r (select {" + " ".join(f"{n}: {e}" for n, e, _ in maps) + f" by: k from: t{where}" + "}))")
        outs = {"k": "(at r 'k)"}
        for name, _, tup in maps:
            nested = not (isinstance(tup, tuple) and tup[0] != "row")
            if not nested:
                outs[name] = f"(at r '{name})"
            elif not empty:
                outs[name] = f"(raze (at r '{name}))"
                outs["n_" + name] = f"(map count (at r '{name}))"
        for name, e in outs.items():  # (written as Session.out writes them, read here: the answers include U8 and I16 vectors)
            s.eval(f'(set "{os.path.join(s.dir, "out_" + name)}" {e})')
        s.run(threads=threads)
        return {name: read_file(os.path.join(s.dir, f"out_{name}")) for name in outs}


def by_key(ans):
    """an answer as {key: everything the answer says about that key's group}: what must not depend on the pool"""
    keys = ans["k"][0]
    out = {int(k): [] for k in keys}
    for name in sorted(ans):
        if name == "k" or name.startswith("n_"):
            continue
        cells, tp, attrs = ans[name]
        if "n_" + name in ans:  # a razed LIST column: cut by its lengths
            off = np.concatenate([[0], np.cumsum(ans["n_" + name][0])])
            for g, k in enumerate(keys):
                out[int(k)].append((name, tp, attrs, cells[off[g]:off[g + 1]].tobytes()))
        else:
            for g, k in enumerate(keys):
                out[int(k)].append((name, tp, attrs, cells[g:g + 1].tobytes()))
    return out


def main():
    assert ref.available(), "build the reference first: python -c 'import __graft_entry__ as g; g.build()'"
    fixture, names, failed, order_differs = {}, [], {}, []
    for c in R.cases():
        names.append(c["name"])
        try:
            a, b = run_case(c, 1), run_case(c, 8)
        except Exception as e:  # the reference did not answer: a finding, kept under `failed`
            failed[c["name"]] = f"no answer: {str(e)[-300:]}"
            print("FAILED", c["name"], failed[c["name"]])
            continue
        same = a.keys() == b.keys() and all(np.array_equal(a[k][0].view(np.uint8), b[k][0].view(np.uint8)) and a[k][1:] == b[k][1:] for k in a)
        if not same and not (a.keys() == b.keys() and by_key(a) == by_key(b)):
            failed[c["name"]] = "1 and 8 threads disagree in more than the order of the groups"
            print("FAILED", c["name"], failed[c["name"]])
            continue
        fixture[c["name"]] = {k: dict(digest=R.digest(v[0]), type=v[1], attrs=v[2]) for k, v in a.items()}
        if not same:
            order_differs.append(c["name"])
        print("ok", c["name"], {k: (v[1], len(v[0])) for k, v in a.items()})
    text = json.dumps(dict(cases=names, answers=fixture, failed=failed, order_differs_with_8_threads=order_differs), sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "collect_golden.npz"), json=np.frombuffer(text.encode(), dtype=np.uint8))
    print(len(fixture), "answered,", len(failed), "failed; group order differs with 8 threads:", order_differs)


if __name__ == "__main__":
    main()
