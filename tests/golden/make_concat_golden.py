#!/usr/bin/env python
"""Golden concat and raze from the compiled reference -- build container only.

    python tests/golden/make_concat_golden.py     # writes tests/golden/concat_golden.npz

Every case is a Rayfall script run by the reference BINARY (oracle/ref.py Session): every part goes in as a column file carrying its type code (1 B8, 2 U8,
3 I16, 4 I32, 5 I64, 7 DATE, 8 TIME, 9 TIMESTAMP, 10 F64), an atom is (first v) of a one-cell vector of its type, a table is (table [names] (list
columns)), and (concat x y) or (raze (list parts...)) is evaluated; every column of the answer comes back as a column file whose header gives its type code
and attributes.  Each case runs with one thread and with eight; only cases on which the two runs agree (and the reference answers at all) are kept, the
others are printed.  A SYMBOL column cannot travel as a file (its cells are interned ids): the tests run every I64 case once more under the SYMBOL type
code, held to the restatement.  A `host_` case is an input only: a shape the device path hands to the host, named by tests/concat_ref.py HOST_SHAPES,
with the reason the door gives -- which shapes those are is read off ray_concat / ray_raze (core/compose.c:465-823, 1096-1164): whatever is not the
plain memcpy arms of one of the ten types.

The fixture is data only (tests/concat_ref.py load_cases reads it): `cases`, a JSON text, and the cells as byte planes in one `blob` of bytes that `index`
lines "key|dtype|shape|offset|bytes" cut up.  A part is a (start, cells) span of its column's pool of cells; the pools are arithmetic in the row number
(every 16th cell a null / a NaN), so their planes compress."""
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
from concat_ref import B8, U8, I16, I32, I64, DATE, TIME, TS, F64, DTYPE, planes  # noqa: E402

RECORDED = (B8, U8, I16, I32, DATE, TIME, I64, TS, F64)  # (SYMBOL: see above)
XLENS = {1: (0, 1, 15, 16, 17), 2: (0, 7, 8, 9), 4: (0, 3, 4, 5), 8: (0, 1, 2, 3)}  # the second span at every misalignment class of a 16-byte access
YLENS = (0, 1, 5, 64, 4097)
BIG = 2**20 + 5
BIG_X = 700001  # odd, and far beyond the first 16 KB tile of any width
RAZE_LENS, RAZE_P = (0, 1, 3, 17, 4097), (0.3, 0.25, 0.25, 0.198, 0.002)
POOL = 4097 + 400


def cells(n, tp, period=0):
    """period: the long pools repeat every `period` rows -- a prime, so that no whole number of periods is a whole number of 16-byte accesses or tiles"""
    i = np.arange(n, dtype=np.int64)
    if period:
        i %= period
    if tp == B8:
        return (i % 3 == 0).astype(np.int8)
    if tp == U8:
        return ((i * 7 + 3) % 251).astype(np.uint8)
    if tp == F64:
        return np.where(i % 16 == 5, np.nan, i * 0.5 - 1000.0)
    null = {2: -2**15, 4: -2**31, 8: -2**63}[np.dtype(DTYPE[tp]).itemsize]
    return np.where(i % 16 == 5, null, i * 7 - 3000).astype(DTYPE[tp])


def cases():
    rng = np.random.default_rng(20261020)
    out = []

    def col(tp, pool, spans, atoms=()):
        return dict(tp=tp, pool=pool, spans=[[int(a), int(b)] for a, b in spans], atoms=list(atoms))

    for tp in RECORDED:
        w = np.dtype(DTYPE[tp]).itemsize
        pool = f"pool_t{tp}"
        for xl in XLENS[w]:
            for yl in YLENS:
                out.append(dict(name=f"concat_vv_t{tp}_x{xl}_y{yl}", verb="concat", cols=[col(tp, pool, [(300, xl), (7, yl)])]))
        for n in sorted(set(XLENS[w]) | set(YLENS)):
            out.append(dict(name=f"concat_va_t{tp}_len{n}", verb="concat", cols=[col(tp, pool, [(300, n), (5, 1)], atoms=[1])]))  # (cell 5: the null)
            out.append(dict(name=f"concat_av_t{tp}_len{n}", verb="concat", cols=[col(tp, pool, [(22, 1), (300, n)], atoms=[0])]))
    for tp in (B8, I16, I32, I64):  # a span boundary inside a workgroup's tile that is not the first
        out.append(dict(name=f"concat_big_t{tp}", verb="concat", cols=[col(tp, f"big_t{tp}", [(BIG - BIG_X, BIG_X), (0, BIG - BIG_X)])]))
    kinds = [I64, I32, B8, F64, DATE, TS, TIME, I16, U8]
    for ncols in (1, 3, 9):
        for tag, xr, yr in (("", 513, 65),) + ((("_x0", 0, 65), ("_y0", 513, 0), ("_both0", 0, 0)) if ncols == 3 else ()):
            names = [f"c{j}" for j in range(ncols)]
            out.append(dict(name=f"table{ncols}{tag}", verb="table", names=names, ynames=names[::-1],
                            cols=[col(kinds[j], f"pool_t{kinds[j]}", [(11 + j, xr), (1000 + 3 * j, yr)]) for j in range(ncols)]))
    for tp in (B8, I16, I32, I64, F64):
        pool = f"pool_t{tp}"
        for ns in (1, 2, 7, 1000, 5000):
            lens = rng.choice(RAZE_LENS, size=ns, p=RAZE_P)
            if ns == 1:
                lens[:] = 17
            if ns >= 2:
                lens[0] = 0 if ns > 2 else 3
                lens[-1] = 0
            if ns >= 7:
                lens[2:5] = 0   # a run of empties
                lens[5] = 4097  # ... then a long span from an odd cell
            out.append(dict(name=f"raze_t{tp}_n{ns}", verb="raze", cols=[col(tp, pool, [(int(rng.integers(0, POOL - n + 1)), n) for n in lens.tolist()])]))
        out.append(dict(name=f"raze_t{tp}_all_empty", verb="raze", cols=[col(tp, pool, [(5, 0)] * 7)]))
    return out


HOST = (("host_concat_atom_atom", "concat", "atom_atom", "an atom with an atom"), ("host_concat_types_differ", "concat", "types_differ", "operands of different types"),
        ("host_concat_vector_atom_types_differ", "concat", "vector_atom_types_differ", "operands of different types"),
        ("host_concat_c8", "concat", "c8", "not a vector of a concat type"), ("host_concat_guid", "concat", "guid", "not a vector of a concat type"),
        ("host_concat_enum", "concat", "enum", "not a vector of a concat type"), ("host_concat_maplist", "concat", "maplist", "not a vector of a concat type"),
        ("host_concat_list", "concat", "list", "a LIST, a DICT, or a table with something else"), ("host_concat_dict", "concat", "dict", "a LIST, a DICT, or a table with something else"),
        ("host_concat_table_vector", "concat", "table_vector", "a LIST, a DICT, or a table with something else"), ("host_concat_parted", "concat", "parted", "a parted column"),
        ("host_concat_names_differ", "concat", "names_differ", "tables whose name sets differ"), ("host_concat_names_extra", "concat", "names_extra", "tables whose name sets differ"),
        ("host_concat_col_types_differ", "concat", "col_types_differ", "paired columns of different types"),
        ("host_concat_table_c8_column", "concat", "table_c8_column", "not a vector of a concat type"), ("host_concat_table_parted", "concat", "table_parted", "a parted table"),
        ("host_raze_not_list", "raze", "raze_not_list", "not a list"), ("host_raze_empty_list", "raze", "raze_empty_list", "an empty list"),
        ("host_raze_mixed_types", "raze", "raze_mixed_types", "elements that are not all vectors of one type"),
        ("host_raze_atom_element", "raze", "raze_atom_element", "elements that are not all vectors of one type"),
        ("host_raze_list_element", "raze", "raze_list_element", "elements that are not all vectors of one type"), ("host_raze_c8", "raze", "raze_c8", "not a vector of a concat type"),
        ("host_concat_device_i32", "concat", "device_i32", "a device column that is not I64 / F64 / TIMESTAMP / B8"),
        ("host_concat_device_i16", "concat", "device_i16", "a device column that is not I64 / F64 / TIMESTAMP / B8"),
        ("host_concat_device_u8", "concat", "device_u8", "a device column that is not I64 / F64 / TIMESTAMP / B8"))


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    if tp not in DTYPE:
        raise ValueError(f"its answer has type code {tp} (an atom made by (first v) of this type is not the type's atom)")
    return np.frombuffer(body, DTYPE[tp], n).copy(), tp, attrs


def run_case(c, pools, threads):
    with ref.Session() as s:
        colvars = []
        for k, col in enumerate(c["cols"]):
            parts = []
            for j, (a, n) in enumerate(col["spans"]):
                s.put(f"p{k}_{j}", pools[col["pool"]][a:a + n], tp=col["tp"])
                parts.append(f"(first p{k}_{j})" if j in col["atoms"] else f"p{k}_{j}")
            colvars.append(parts)
        if c["verb"] == "table":
            order = [c["names"].index(nm) for nm in c["ynames"]]
            s.eval(f"(set x (table [{' '.join(c['names'])}] (list {' '.join(colvars[k][0] for k in range(len(colvars)))})))")
            s.eval(f"(set y (table [{' '.join(c['ynames'])}] (list {' '.join(colvars[k][1] for k in order)})))")
            s.eval("(set r (concat x y))")
            for j, nm in enumerate(c["names"]):
                s.out(f"o{j}", f"(at r '{nm})")
        else:
            if c["verb"] == "concat":
                s.eval(f"(set r (concat {colvars[0][0]} {colvars[0][1]}))")
            else:  # (a list of thousands of parts is put together 200 at a time: LIST with LIST is the reference's plain list concat)
                s.eval(f"(set l (list {' '.join(colvars[0][:200])}))")
                for at in range(200, len(colvars[0]), 200):
                    s.eval(f"(set l (concat l (list {' '.join(colvars[0][at:at + 200])})))")
                s.eval("(set r (raze l))")
            s.out("o0", "r")
        ref.run_script("\n".join(s.lines) + "\n", threads=threads)  # (Session.run reads the answers back by dtype: it knows no U8 / I16)
        return [read_file(os.path.join(s.dir, f"out_o{j}")) for j in range(len(c["cols"]))]


def record(c, pools):
    try:
        one, eight = run_case(c, pools, 1), run_case(c, pools, 8)
    except (RuntimeError, KeyError, ValueError) as e:
        return None, f"the reference does not answer it: {str(e)[:200]}"
    if any(a[1:] != b[1:] or a[0].tobytes() != b[0].tobytes() for a, b in zip(one, eight)):
        return None, "1 and 8 threads differ"
    return one, None


def main():
    assert ref.build() or ref.available()
    pools = {f"pool_t{tp}": cells(POOL, tp) for tp in RECORDED}
    pools.update({f"big_t{tp}": cells(BIG, tp, period=4093) for tp in (B8, I16, I32, I64)})
    cs = cases()
    with ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda c: record(c, pools), cs))
    arrays = {k: planes(v) for k, v in pools.items()}
    kept = []
    for k, (c, (outs, why)) in enumerate(zip(cs, got)):
        if outs is None:
            print("dropped", c["name"], "--", why)
            continue
        for j, col in enumerate(c["cols"]):
            key = f"c{k}_s{j}"
            arrays[key] = np.array(col["spans"], dtype=np.int64).reshape(-1, 2)
            col["spans"] = key
        c["out"] = []
        for j, (a, tp, attrs) in enumerate(outs):
            arrays[f"c{k}_o{j}"] = planes(a)
            c["out"].append(dict(tp=int(tp), attrs=int(attrs), key=f"c{k}_o{j}"))
        c["threads"] = "1,8"
        kept.append(c)
    used = {col["pool"] for c in kept for col in c["cols"]}
    arrays = {k: v for k, v in arrays.items() if not (k.startswith("pool_") or k.startswith("big_")) or k in used}
    kept += [dict(name=n, verb=v, shape=sh, host=why) for n, v, sh, why in HOST]
    index, parts, at = [], [], 0
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        index.append(f"{key}|{a.dtype.str}|{'x'.join(str(d) for d in a.shape)}|{at}|{a.nbytes}")
        parts.append(a.reshape(-1).view(np.uint8))
        at += a.nbytes
    path = os.path.join(HERE, "concat_golden.npz")
    np.savez_compressed(path, cases=np.frombuffer(json.dumps(kept).encode(), np.uint8), index=np.array(index), blob=np.concatenate(parts))
    print("wrote", len(kept), "cases of", len(cs) + len(HOST), ",", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2**20


if __name__ == "__main__":
    main()
