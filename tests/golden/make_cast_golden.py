#!/usr/bin/env python
"""Golden `as` over vectors from the compiled reference -- build container only.

    python tests/golden/make_cast_golden.py     # writes tests/golden/cast_golden.npz

Every case is a Rayfall script run by the reference BINARY (oracle/ref.py Session): B8, I32, DATE, TIME, I64, TIMESTAMP and F64 inputs go in as column
files carrying their type code; I16 and U8 inputs cannot travel as column files, so the script makes them by casting the I32 file, and their cells are
recorded as the reference produced them.  One script per length and thread count evaluates (as 'name x) for every (source, target) pair of the nine types
under both spellings of the name ('i32 and 'I32) and writes each answer to a column file, which this maker reads with a reader of its own (16-byte header:
type code, attribute byte, length; oracle/ref.py's read_col knows no U8 / I16 payloads).  Each script runs with one thread and with eight, and the maker stops
where the two -- or the two spellings -- differ.  The arms the reference answers with an error (B8 <-> U8 over a non-empty vector, an unknown type name, an
atom name of a type outside the nine) would end a script: each runs alone, and is recorded as a `host_` case with the reason the device door gives.

The fixture is data only (tests/cast_ref.py load_cases reads it): `cases` lines
"name|source type|target type|spelling|length|x key|x attrs|out key|out type|out attrs|host reason|reference errors|threads" and the cells as byte planes,
all of them in one `blob` of bytes that `index` lines "key|dtype|shape|offset|bytes" cut up.  Cells repeat with a period coprime to 8 (29 integer cells, 37 f64
cells), so that the reference's vector body and its scalar tail both see every value, and the planes compress."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
from cast_ref import B8, U8, I16, I32, I64, DATE, TIME, TS, F64, TYPES, DTYPE, VECTOR_NAME, ATOM_NAME, NULL32, NULL64, LENS, BIG, planes, has_arm  # noqa: E402

INTS = [0, 1, -1, 255, 256, 32768, -32768, 2**31, NULL32, 2**31 - 1, NULL64, 2**63 - 1, 127, 128, -128, -129, 65535, 65536, 32767, -32769, 2**32 + 5,
        -(2**32) - 5, 2**53 + 1, -(2**53) - 1, 1234567890123, -987654321, 2, -2, 2**63 - 2]
FLOATS = [0.0, -0.0, 0.5, -0.5, 1.9, -1.9, 255.0, 256.0, 300.7, 32767.9, 32768.0, -32769.0, 2147483647.0, 2147483648.0, -2147483648.5, -2147483649.0,
          2.0**32 + 5, 9.3e18, -9.3e18, float("nan"), float("inf"), float("-inf"), 5e-324, 1e10, -1e10, 65535.5, -255.5, 127.5, -128.9, 4294967295.0,
          -4294967296.0, 2.0**63, -(2.0**63), 2.0**53 + 2, 1.0, -1.0, -2147483648.0]
assert len(INTS) == 29 and len(FLOATS) == 37
FILE_TYPES = (B8, I32, DATE, TIME, I64, TS, F64)  # what travels as a column file; U8 and I16 are cast from the I32 file inside the script
# the long cases: one per source cell class and the arms the bench names, vector spelling
BIG_ARMS = ((I64, F64), (F64, I64), (I64, I32), (I32, I64), (F64, U8), (I16, I64), (U8, I32), (B8, F64), (F64, I16))


def cells(n, tp):
    """n cells of the type, the specials rotated by the length (the short lengths see different ones)"""
    if tp == F64:
        base = np.array(FLOATS, dtype=np.float64)
    else:
        base = np.array([v & (2**64 - 1) for v in INTS], dtype=np.uint64).astype(DTYPE[I64 if tp in (U8, I16) else tp])  # (the low bytes of each special)
    return np.resize(np.roll(base, -(n % len(base))), n)


def read_file(path):
    with open(path, "rb") as f:
        _, _, tp, attrs, _, n = struct.unpack("<BBbBIq", f.read(16))
        body = f.read()
    return np.frombuffer(body, DTYPE[tp], n).copy(), tp, attrs


def inputs(s, n):
    for tp in FILE_TYPES:
        s.put(f"x{tp}", cells(n, tp), tp=tp)
    s.eval(f"(set x{I16} (as 'I16 x{I32}))")
    s.eval(f"(set x{U8} (as 'U8 x{I32}))")


def out(s, name, expr):
    """(Session.out would have Session.run read the file back with read_col)"""
    s.eval(f'(set "{os.path.join(s.dir, "out_" + name)}" {expr})')


def run_length(n, threads, arms):
    """-> {(st, dt, spelling): (cells, type, attrs)}, {st: the source's cells as the reference held them}"""
    with ref.Session() as s:
        inputs(s, n)
        for st in (U8, I16):
            out(s, f"x{st}", f"x{st}")
        for st, dt in arms:
            for sp, names in (("atom", ATOM_NAME), ("vector", VECTOR_NAME)):
                out(s, f"o{st}_{dt}_{sp}", f"(as '{names[dt]} x{st})")
        s.run(threads=threads)
        got = {(st, dt, sp): read_file(os.path.join(s.dir, f"out_o{st}_{dt}_{sp}")) for st, dt in arms for sp in ("atom", "vector")}
        xs = {tp: cells(n, tp) for tp in FILE_TYPES}
        for st in (U8, I16):
            xs[st], tp, _ = read_file(os.path.join(s.dir, f"out_x{st}"))
            assert tp == st
        return got, xs


def reference_errors(n, expr):
    try:
        with ref.Session() as s:
            inputs(s, n)
            out(s, "e", expr)
            s.run(threads=1)
        return False
    except RuntimeError:
        return True


def attribute_cases():
    """a same-type cast keeps the argument's attributes (clone_obj), a converting one answers a fresh vector without them: over (asc x), which carries ATTR_ASC"""
    res = {}
    for threads in (1, 8):
        with ref.Session() as s:
            s.put("x", cells(65, I64), tp=I64)
            s.eval("(set sx (asc x))")
            out(s, "sx", "sx")
            out(s, "same", "(as 'I64 sx)")
            out(s, "conv", "(as 'F64 sx)")
            s.run(threads=threads)
            res[threads] = [read_file(os.path.join(s.dir, "out_" + k)) for k in ("sx", "same", "conv")]
    for a, b in zip(res[1], res[8]):
        assert same(a, b), "attribute cases: 1 and 8 threads differ"
    return res[1]


def same(a, b):
    return a[0].dtype == b[0].dtype and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


def main():
    assert ref.build() or ref.available()
    arrays, lines = {}, []

    def keep(key, a):
        if a.size and key not in arrays:
            arrays[key] = planes(a)
        return key

    pairs = [(st, dt) for st in TYPES for dt in TYPES]
    for n in LENS + (BIG,):
        arms = [(st, dt) for st, dt in (pairs if n != BIG else BIG_ARMS) if n == 0 or has_arm(st, dt)]
        (one, xs), (eight, xs8) = run_length(n, 1, arms), run_length(n, 8, arms)
        for st in TYPES:
            assert xs[st].tobytes() == xs8[st].tobytes(), (n, st)
        for st, dt in arms:
            a = one[(st, dt, "vector")]
            for other in (one[(st, dt, "atom")], eight[(st, dt, "vector")], eight[(st, dt, "atom")]):
                assert same(a, other), f"len {n} {st} -> {dt}: the spellings or 1 and 8 threads differ"
            assert a[1] == dt and len(a[0]) == n, (n, st, dt, a[1], len(a[0]))
            for sp in ("atom", "vector"):
                if n == BIG and sp == "atom":
                    continue
                lines.append(f"as_{VECTOR_NAME[st]}_{VECTOR_NAME[dt]}_{sp}_len{n}|{st}|{dt}|{sp}|{n}|{keep(f'x{st}_{n}', xs[st])}|0|{keep(f'o{st}_{dt}_{n}', a[0])}|{a[1]}|{a[2]}||0|1,8")
        print(n, len(lines))
    sx, same_type, conv = attribute_cases()
    assert sx[2] == 2, sx[2]
    for nm, (a, tp, attrs), dt in (("same_type_keeps_attrs", same_type, I64), ("converted_drops_attrs", conv, F64)):
        lines.append(f"as_{nm}|{I64}|{dt}|vector|65|{keep('xs_asc', sx[0])}|{sx[2]}|{keep('o_' + nm, a)}|{tp}|{attrs}||0|1,8")
    # the shapes the door hands to the host; the reference answers each of them with an error of its own
    why_arm = "the reference has no cast between B8 and U8 vectors"
    why_name = "a type name outside the nine numeric and temporal types"
    for st, dt in ((B8, U8), (U8, B8)):
        for sp, names in (("atom", ATOM_NAME), ("vector", VECTOR_NAME)):
            assert reference_errors(17, f"(as '{names[dt]} x{st})")
            xs = run_length(17, 1, [])[1]
            lines.append(f"host_{VECTOR_NAME[st]}_{VECTOR_NAME[dt]}_{sp}|{st}|{dt}|{sp}|17|{keep(f'x{st}_17', xs[st])}|0||||{why_arm}|1|1")
    assert reference_errors(17, f"(as 'nosuchtype x{I64})")
    lines.append(f"host_unknown_name|{I64}|0|nosuchtype|17|{keep(f'x{I64}_17', cells(17, I64))}|0||||{why_name}|1|1")
    assert reference_errors(17, f"(as 'guid x{I64})")
    lines.append(f"host_guid_name|{I64}|0|guid|17|{keep(f'x{I64}_17', cells(17, I64))}|0||||{why_name}|1|1")
    # one blob and an index instead of a few thousand members: the archive's per-member headers would outweigh the cells
    index, parts, at = [], [], 0
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        index.append(f"{key}|{a.dtype.str}|{'x'.join(str(d) for d in a.shape)}|{at}|{a.nbytes}")
        parts.append(a.reshape(-1).view(np.uint8))
        at += a.nbytes
    path = os.path.join(HERE, "cast_golden.npz")
    np.savez_compressed(path, cases=np.array(lines), index=np.array(index), blob=np.concatenate(parts) if parts else np.empty(0, np.uint8))
    print("wrote", len(lines), "cases,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 2**20


if __name__ == "__main__":
    main()
