"""C-ABI checks that need no GPU: the library loads, exports every symbol the headers declare, the structs have the
agreed layout, the standalone host object model round-trips, and every compute entry point FAILS LOUDLY without a
device (there is no CPU fallback behind the product path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rfx_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(built):
    from rayforce_amd import _lib, hostobj
    lib = _lib.load_library()
    names = declared("rfx_hip.h") + declared("rfx_ops.h") + declared("rfx_exec.h")
    assert len(names) > 100
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # the python prototypes cover the headers one to one
    proto = set(_lib.PROTOTYPES) | set(hostobj.OPS_PROTOTYPES)
    assert set(names) <= proto, sorted(set(names) - proto)
    # ... and NOTHING else is exported (round 6: -fvisibility=hidden, the headers push default visibility): the reference dlopens plugins
    # RTLD_GLOBAL (core/dynlib.c:131) -- C++-mangled internals and __device_stub__ kernel stubs must not land in the host's namespace
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-2] in "TtDdBbRrWwVvi"}
    extra = sorted(exported - set(names))
    assert not extra, extra[:40]


def test_struct_layouts(built):
    from rayforce_amd import _lib as L
    assert C.sizeof(L.Pred) == 40 and L.Pred.op.offset == 24 and L.Pred.u.offset == 32
    assert C.sizeof(L.Agg) == 56 and L.Agg.xop.offset == 16 and L.Agg.d_xrhs_col.offset == 24 and L.Agg.nxnodes.offset == 36 and L.Agg.xu.offset == 40
    assert L.Agg.xnodes.offset == 48 and C.sizeof(L.XNode) == 56 and L.XNode.r.offset == 32
    assert C.sizeof(L.Partial) == 64 and C.sizeof(L.Value) == 16
    assert C.sizeof(L.GroupTables) == 8 + 8 + 8 + 8 + 64 + 64
    # include/rfx_exec.h: the planner's structures as the C compiler lays them out (a small program prints the sizes)
    import subprocess, tempfile
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "rfx_exec.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rfx_query_t), '
                             'sizeof(rfx_groups_t), sizeof(rfx_ids_t), sizeof(rfx_qcol_t), sizeof(rfx_transport_t), offsetof(rfx_query_t, key_scope), offsetof(rfx_groups_t, d_block));return 0;}\n')
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(td, "s")], check=True)
        sizes = [int(x) for x in subprocess.run([os.path.join(td, "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(L.Query), C.sizeof(L.Groups), C.sizeof(L.Ids), C.sizeof(L.QCol), C.sizeof(L.Transport), L.Query.key_scope.offset, L.Groups.d_block.offset], sizes
    from rayforce_amd.hostobj import Header
    assert C.sizeof(Header) == 16 and Header.type.offset == 2 and Header.rc.offset == 4 and Header.len.offset == 8


def test_abi_header_compiles_as_c_and_cxx(built, tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "rfx_abi.h"\n#include "rfx_hip.h"\n#include "rfx_exec.h"\n#include "rfx_ops.h"\nint main(void){return (sizeof(rfx_obj_t)==16 && sizeof(rfx_agg_t)==56 && sizeof(rfx_xnode_t)==56 && sizeof(rfx_pred_t)==40 && sizeof(rfx_partial_t)==64)?0:1;}\n')
    for cc, std in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        exe = tmp_path / ("a_" + cc)
        subprocess.run([cc, std, "-x", "c" if cc == "gcc" else "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        assert subprocess.run([str(exe)]).returncode == 0


def test_no_device_means_loud_failure(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    from rayforce_amd import RfxError, _lib
    from rayforce_amd.engine import Engine
    lib = _lib.load_library()
    assert lib.rfx_hip_device_count() == 0
    ctx = C.c_void_p()
    assert lib.rfx_hip_ctx_create(0, None, C.byref(ctx)) == -1  # RFX_ENODEV
    assert b"no CPU fallback" in lib.rfx_hip_last_error()
    with pytest.raises(RfxError):
        Engine(0)
    # operator layer: builds the query objects, then refuses to compute without a device
    from rayforce_amd import hostobj as H
    ops = H.lib()
    tab = H.table({"k": np.array([1, 2, 1], np.int64), "v": np.array([1.0, 2.0, 3.0])})
    d = H.select_dict({"s": ("sum", "v"), "by": "k"}, tab)
    r = ops.rfx_select(d)
    assert H.is_error(r) and "MI355X" in H.error_text(r)
    for o in (r, d, tab):
        ops.rfx_host_drop(o)


def test_host_object_model_roundtrip(built):
    from rayforce_amd import hostobj as H
    ops = H.lib()
    a = np.arange(10, dtype=np.int64)
    v = H.vector(a)
    h = H.header(v)
    assert h.type == H.T_I64 and h.len == 10 and h.rc == 1 and (H.payload(v) % 32) == 0  # payload 32-byte aligned like core/heap.c
    assert np.array_equal(H.to_numpy(v), a)
    tab = H.table({"x": a, "y": a.astype(np.float64)})
    back = H.table_to_numpy(tab)
    assert list(back) == ["x", "y"] and back["y"].dtype == np.float64
    e = H.expr(("and", ("<", "x", 5), (">", "y", 1.5)))
    items = H.list_items(e)
    assert H.header(items[0]).type == 103  # TYPE_VARY function object, positive type code (core/env.c:66-74)
    assert H.header(H.list_items(items[1])[0]).type == 102
    for o in (v, tab, e):
        ops.rfx_host_drop(o)


def test_partial_algebra_on_host(built):
    """rfx_partial_merge / rfx_agg_finalize are pure host C: the multi-GPU fold can be checked without a device."""
    from rayforce_amd import _lib as L
    lib = L.load_library()
    a, b = L.Partial(), L.Partial()
    lib.rfx_partial_identity(C.byref(a))
    lib.rfx_partial_identity(C.byref(b))
    a.isum, a.cnt = 2**63 - 1, 3
    b.isum, b.cnt = 5, 2
    lib.rfx_partial_merge(L.RFX_AGG_SUM, L.RFX_I64, C.byref(a), C.byref(b))
    assert a.isum == -(2**63) + 4 and a.cnt == 5  # i64 sums wrap
    v = L.Value()
    lib.rfx_agg_finalize(L.RFX_AGG_SUM, L.RFX_I64, C.byref(a), C.byref(v))
    assert v.type == L.RFX_I64 and v.i == a.isum
    e = L.Partial()
    lib.rfx_partial_identity(C.byref(e))
    for kind, typ, null in ((L.RFX_AGG_MIN, L.RFX_I64, True), (L.RFX_AGG_MAX, L.RFX_F64, True), (L.RFX_AGG_AVG, L.RFX_F64, True),
                            (L.RFX_AGG_SUM, L.RFX_F64, False), (L.RFX_AGG_COUNT, L.RFX_I64, False)):
        lib.rfx_agg_finalize(kind, typ, C.byref(e), C.byref(v))
        assert bool(v.is_null) == null, (kind, typ)  # empty min/max -> null, avg -> NaN, sum -> 0, count -> 0
    # f64 extrema travel as raw bits and are ordered correctly, negative values included
    import struct
    bits = lambda x: struct.unpack("<q", struct.pack("<d", x))[0]
    p, q = L.Partial(), L.Partial()
    lib.rfx_partial_identity(C.byref(p)); lib.rfx_partial_identity(C.byref(q))
    p.ext, p.cnt = bits(-1.5), 1
    q.ext, q.cnt = bits(-2.5), 1
    lib.rfx_partial_merge(L.RFX_AGG_MIN, L.RFX_F64, C.byref(p), C.byref(q))
    assert p.ext == bits(-2.5)


def test_column_file_header_is_read_without_a_device(built, tmp_path):
    """rfx_column_file_stat is host-only: the 16-byte header of core/binary.c:263-311."""
    from oracle import ref
    from rayforce_amd import _lib as L
    lib = L.load_library()
    p = str(tmp_path / "col")
    ref.write_col(p, np.arange(12345, dtype=np.float64))
    t, n = C.c_int32(), C.c_int64()
    assert lib.rfx_column_file_stat(p.encode(), C.byref(t), C.byref(n)) == 0 and t.value == 10 and n.value == 12345
    (tmp_path / "junk").write_bytes(b"x" * 40)
    assert lib.rfx_column_file_stat(str(tmp_path / "junk").encode(), C.byref(t), C.byref(n)) == -2
    assert b"not a RayforceDB column file" in lib.rfx_hip_last_error()


def test_bench_launch_contract_dry_run():
    """`python bench.py --gpus 2` must start two ranks by itself (no launcher), shard the workload's BASELINE rows over them
    (strong scaling) and report n_gpus == 2 -- checked here without a device (--dry-run: rendezvous over gloo + shard arithmetic)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for wl, total in (("c3w", 1_000_000_000), ("c5", 2_000_000_000)):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", wl, "--dry-run"], env=env, capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["dry_run"] is True
        assert line["config"]["total_rows"] == total and line["config"]["rows_per_gpu"] == [total // 2, total - total // 2]
    # weak scaling on request: every rank holds the BASELINE row count
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c2", "--scaling", "weak", "--dry-run"], env=env,
                         capture_output=True, text=True, timeout=300)
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["total_rows"] == 2_000_000_000
    # a launcher that started a different number of ranks than --gpus is an error, not a silent 1-GPU run
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"], env={**env, "WORLD_SIZE": "1", "RANK": "0"},
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "refusing" in (bad.stderr + bad.stdout)


def test_plan_kernels_prewarm_into_the_disk_cache_without_a_device(built, tmp_path):
    """rfx_hip_rtc_prewarm_filter_aggr: the plan kernel of C2b is compiled by hiprtc from the headers EMBEDDED in librfx.so (the library
    is loaded from a copy in an empty directory: no source tree beside it), written to RFX_RTC_CACHE; asking again -- in the same
    process and in a new one -- finds the code object and compiles nothing; another plan is another file."""
    import shutil
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lone = tmp_path / "lone"
    lone.mkdir()
    shutil.copy(os.path.join(root, "rayforce_amd", "librfx.so"), lone / "librfx.so")
    cache = tmp_path / "cache"
    prog = (
        "import ctypes as C, sys\n"
        f"sys.path.insert(0, {root!r})\n"
        "from rayforce_amd import _lib as L, prewarm\n"
        "lib = L.load_library()\n"
        "r = [prewarm.filter_aggr(*prewarm.BASELINE_PLANS['c2b']) for _ in range(2)]\n"
        "if len(sys.argv) > 1: r.append(prewarm.filter_aggr(*prewarm.BASELINE_PLANS['c5']))\n"
        "a, b = C.c_int64(), C.c_int64()\n"
        "lib.rfx_hip_rtc_stats(C.byref(a), C.byref(b))\n"
        "import json; print('RESULT', json.dumps([r, b.value, prewarm.cache_stats()[1]]))\n")
    env = dict(os.environ, RFX_RTC_CACHE=str(cache), RFX_LIB=str(lone / "librfx.so"))

    def run(*args):
        out = subprocess.run([sys.executable, "-c", prog, *args], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][0]
        import json
        return json.loads(line[len("RESULT "):])  # [[plan in the cache? ...], compilations, files written]

    first = run()
    if first[0] == [False, False]:
        pytest.skip("libhiprtc.so is not loadable here: the prebuilt kernels are what runs")
    assert first == [[True, True], 1, 1], first  # compiled once, the second call read the file
    files = sorted(os.listdir(cache))
    assert len(files) == 1 and files[0].endswith(".co") and open(cache / files[0], "rb").read(4) == b"\x7fELF"
    again = run("more")
    assert again == [[True, True, True], 1, 1], again  # a new process: C2b from disk, only C5 compiled
    assert len(os.listdir(cache)) == 2


def test_phase_handover_probe_runs_without_a_device(built):
    """rfx_exec_probe_handover_us: the planner's phase hand-over over a bare worker pool (what bench.py's predicted T(N) charges per phase)."""
    from rayforce_amd import _lib
    lib = _lib.load_library()
    assert lib.rfx_exec_probe_handover_us(1, 10) == 0.0 or lib.rfx_exec_probe_handover_us(1, 10) < 5.0
    for n in (2, 4, 8):
        us = lib.rfx_exec_probe_handover_us(n, 500)
        assert 0.0 < us < 5000.0, (n, us)
    assert lib.rfx_exec_probe_handover_us(0, 10) < 0 and lib.rfx_exec_probe_handover_us(99, 10) < 0


def test_bench_dump_outputs_float64_and_a_seeded_sample_past_the_budget(tmp_path):
    """bench.py --dump-outputs: every array as <name>.npy in float64; when they exceed the budget, every array of a length keeps the same
    seeded rows, so that two runs (two builds) compare output for output, and the files stay within 64 MB."""
    import torch
    import bench
    small = {"k": np.arange(5, dtype=np.int64), "s": np.linspace(0.0, 1.0, 5), "values": [1.5, float("nan")], "mask": torch.tensor([0, 1, 1], dtype=torch.int8)}
    bench.dump_outputs(str(tmp_path / "a"), small)
    for name, v in small.items():
        got = np.load(tmp_path / "a" / f"{name}.npy")
        want = v.double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), name
    n = 6_000_000  # two columns of 48 MB each as float64
    big = {"keys": np.arange(n, dtype=np.int64), "sums": np.arange(n, dtype=np.float64) * 0.5}
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    assert sum(f.stat().st_size for f in (tmp_path / "b").iterdir()) <= 64_000_000
    keys, sums = np.load(tmp_path / "b" / "keys.npy"), np.load(tmp_path / "b" / "sums.npy")
    assert keys.dtype == np.float64 and n // 4 < len(keys) < n and np.array_equal(sums, keys * 0.5)  # the same rows of both
    assert np.array_equal(keys, np.load(tmp_path / "c" / "keys.npy"))  # and the same rows again
