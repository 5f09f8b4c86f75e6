"""CPU-side checks: the C-ABI library loads and exports every symbol include/*.h declares, fails
loudly without a GPU, and the C++ host mirror's parsing / decimal-typing rules match the
reference's rules.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lingodb_amd import capi
import tpch_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ldb_gpu_\w+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = capi.gpu_lib()
    names = declared("lingodb_gpu.h") + [n for n in declared("ldb_tpchgen.h") if n.startswith("ldb_gpu_")]
    assert len(names) >= 45
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ but not exported by liblingodb_gpu.so"
        assert n in capi.GPU_API, f"{n} not bound in lingodb_amd.capi"
    assert set(capi.GPU_API) <= set(names)


def test_host_library_exports():
    lib = capi.host_lib()
    for n in capi.HOST_API:
        assert hasattr(lib, n)


def test_no_cpu_fallback_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    st = capi.gpu_lib().ldb_gpu_ctx_create(0, None, C.byref(h))
    assert st == capi.LDB_ERR_NO_DEVICE
    assert b"no HIP device" in capi.gpu_lib().ldb_gpu_last_error()


def test_struct_sizes_match_header():
    # compile-time layout of the descriptor structs as the C compiler sees them
    import subprocess
    import tempfile

    prog = r'''
#include "lingodb_gpu.h"
#include <stdio.h>
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ldb_coltype), sizeof(ldb_colref), sizeof(ldb_filter_desc), sizeof(ldb_factor),
  sizeof(ldb_term), sizeof(ldb_expr), sizeof(ldb_agg_spec), sizeof(ldb_sort_spec)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [C.sizeof(t) for t in (capi.ColType, capi.ColRef, capi.FilterDesc, capi.Factor, capi.Term, capi.Expr, capi.AggSpec, capi.SortSpec)]
    assert sizes == want


# ---------------------------------------------------------------- host mirror (Restrictions::create helpers, SQLTypeUtils)
def parse_date(s):
    out = C.c_int32()
    st = capi.host_lib().ldb_host_parse_date32(s.encode(), C.byref(out))
    return st, out.value


def test_parse_date32():
    assert parse_date("1970-01-01") == (0, 0)
    assert parse_date("1998-09-02") == (0, 10471)
    assert parse_date("1995-03-15") == (0, 9204)
    assert parse_date("2020-06-11") == (0, 18424)
    assert parse_date("1994-1-01") == (0, 8766)  # the regex of Restrictions.cpp:18-19 pads a 1-digit month
    assert parse_date("1969-12-31") == (0, -1)
    assert parse_date("not a date")[0] != 0  # reference: throws "could not parse date"


def parse_dec(s, scale):
    lo, hi = C.c_int64(), C.c_int64()
    st = capi.host_lib().ldb_host_parse_decimal(s.encode(), scale, C.byref(lo), C.byref(hi))
    return st, (hi.value << 64) | (lo.value & 0xFFFFFFFFFFFFFFFF)


def test_parse_decimal_rescale():
    assert parse_dec("0.05", 2) == (0, 5)
    assert parse_dec("24", 2) == (0, 2400)
    assert parse_dec("-1.5", 3) == (0, -1500)
    assert parse_dec("100.01", 2) == (0, 10001)
    assert parse_dec("12345678901234567890.12", 2) == (0, 1234567890123456789012)
    assert parse_dec("0.055", 2)[0] != 0  # rescale would lose precision (Arrow Rescale error → ValueOrDie)


def dec_type(op, a, b=(19, 0)):
    p, s = C.c_int32(), C.c_int32()
    capi.host_lib().ldb_host_decimal_type(op, a[0], a[1], b[0], b[1], C.byref(p), C.byref(s))
    return p.value, s.value


def test_decimal_typing_rules_q1_worked_example():
    # SURVEY §9.1 worked example, from sql_analyzer.cpp:3058-3159
    one_minus_disc = dec_type(2, (19, 0), (12, 2))
    assert one_minus_disc == (21, 2)
    disc_price = dec_type(0, (12, 2), one_minus_disc)
    assert disc_price == (33, 4)
    charge = dec_type(0, disc_price, (21, 2))
    assert charge == (38, 6)  # raw (54,6) clamped, scale kept
    assert dec_type(3, (12, 2)) == (31, 21)  # avg(decimal(12,2))
    assert dec_type(0, (12, 2), (12, 2)) == (24, 4)  # Q6 revenue
    assert dec_type(0, (38, 6), (38, 6)) == (38, 6)  # scale clamp: s > 6 and p - s > 32
    assert dec_type(1, (12, 2), (12, 2)) == (26, 14)
    # Q14: 100.00 * sum(rev) / sum(rev); Q8: sum / sum; Q11: ps_supplycost * ps_availqty (int → decimal(19,0))
    assert dec_type(0, (5, 2), (33, 4)) == (38, 6)
    assert dec_type(1, (38, 6), (33, 4)) == (38, 6)  # raw (75,39): p - s = 36 > 32 and s > 6
    assert dec_type(1, (33, 4), (33, 4)) == (38, 6)
    assert dec_type(0, (12, 2), (19, 0)) == (31, 2)


# ---------------------------------------------------------------- host generator invariants (include/ldb_tpchgen.h)
def test_host_generator_shape_invariants():
    n_orders = 7000
    li = tpch_data.host_table(tpch_data.LINEITEM, n_orders)
    od = tpch_data.host_table(tpch_data.ORDERS, n_orders)
    assert li.num_rows == 4 * n_orders  # period-7 pattern, mean 4 lines per order
    ok = np.asarray(li.column("l_orderkey"))
    assert set(np.unique(ok)) == set(np.asarray(od.column("o_orderkey")).tolist())
    ship = np.asarray(li.column("l_shipdate").cast("int32"))
    rec = np.asarray(li.column("l_receiptdate").cast("int32"))
    assert (rec > ship).all() and ship.min() >= 8036
    flags = set(li.column("l_returnflag").to_pylist())
    assert flags == {b"A\0\0\0", b"N\0\0\0", b"R\0\0\0"}
    # slices tile the table exactly
    parts = [tpch_data.host_table(tpch_data.LINEITEM, n_orders, p, 3, cols=[0, 3]) for p in range(3)]
    assert sum(p.num_rows for p in parts) == li.num_rows
    assert np.array_equal(np.concatenate([np.asarray(p.column("l_orderkey")) for p in parts]), ok)


def test_runtime_specialiser_compiles_without_a_device():
    """the hiprtc specialisation of the group-by kernel (same source as the AOT kernel) compiles for gfx950"""
    buf = C.create_string_buffer(16000)
    st = capi.gpu_lib().ldb_gpu_jit_compile_check(buf, 16000)
    assert st == 0, buf.value.decode(errors="replace")


def test_like_planner_classifies_patterns():
    """which LIKE patterns get the position-parallel matcher (ASCII literals separated by '%', <= 4 segments
    of <= 16 bytes) and which stay with the general one ('_', escapes, non-ASCII, only wildcards)"""
    lib = capi.gpu_lib()

    def plan(pat):
        b = pat.encode()
        n, anchors = C.c_int32(), C.c_int32()
        seg = (C.c_int32 * 8)()
        assert lib.ldb_gpu_like_plan(b, len(b), C.byref(n), seg, C.byref(anchors)) == 0
        return n.value, [(seg[2 * j], seg[2 * j + 1]) for j in range(n.value)], anchors.value

    assert plan("%special%requests%") == (2, [(1, 7), (9, 8)], 0)  # TPC-H Q13
    assert plan("%Customer%Complaints%") == (2, [(1, 8), (10, 10)], 0)  # Q16: a 10-byte segment (two-word compare)
    assert plan("PROMO%") == (1, [(0, 5)], 1) and plan("%BRASS") == (1, [(1, 5)], 2) and plan("%green%") == (1, [(1, 5)], 0)
    assert plan("MEDIUM POLISHED%") == (1, [(0, 15)], 1)
    assert plan("abc") == (1, [(0, 3)], 3)  # no wildcard: equality, anchored at both ends
    assert plan("a%%b%c%d") == (4, [(0, 1), (3, 1), (5, 1), (7, 1)], 3)  # consecutive '%' collapse
    for general in ("", "%", "%%", "_o%", "%a_c%", "%\\%%", "a\\", "%é", "a%b%c%d%e", "%" + "x" * 17 + "%"):
        assert plan(general)[0] == 0, general
    n = C.c_int32()
    assert lib.ldb_gpu_like_plan(b"x" * 49, 49, C.byref(n), None, None) != 0  # longer than the descriptor's inline constant


def test_jit_compiles_in_the_background_and_caches_code_objects_on_disk(tmp_path):
    """round 6 (verdict r5 #4): a specialisation is compiled on a worker thread — the first request is answered "still compiling" (the operator
    launches its generic kernel), ldb_gpu_jit_wait drains the queue — and the code object is kept on disk under a content hash, so the same
    request in a fresh cache state is answered from the file without hiprtc.  Device-less (hiprtc cross-compiles for gfx950); run in a child
    process so that LDB_JIT_CACHE_DIR is this test's own directory"""
    import subprocess
    import sys

    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from lingodb_amd import capi; lib = capi.gpu_lib(); buf = C.create_string_buffer(4000);"
            "st = lib.ldb_gpu_jit_cache_selftest(buf, 4000); v = (C.c_int64 * 8)(); lib.ldb_gpu_jit_info(v, 8); print(st, list(v), buf.value.decode())") % os.path.join(ROOT, "lingo-db_amd")
    env = dict(os.environ, LDB_JIT_CACHE_DIR=str(tmp_path / "jit"), LDB_JIT_ASYNC="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("0 "), r.stdout + r.stderr
    files = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / "jit")) for f in fs]
    assert len(files) == 1 and files[0].endswith(".co") and "gfx950" in files[0] and os.path.getsize(files[0]) > 1000
    with open(files[0], "rb") as f:
        assert f.read(4) == b"\x7fELF"
    # a second process: the same request is a disk hit at once (the self-test then reports a non-empty cache for its key)
    r2 = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and "cache directory not empty" in r2.stdout, r2.stdout + r2.stderr
    info = eval(r2.stdout.split(" ", 1)[1].split("]")[0] + "]")
    assert info[2] == 1 and info[0] == 0 and info[3] == 0, info  # one disk hit, nothing compiled, nothing written
    # with the disk cache off nothing is written
    env3 = dict(env, LDB_JIT_CACHE_DIR=str(tmp_path / "off"), LDB_JIT_DISK_CACHE="0")
    r3 = subprocess.run([sys.executable, "-c", code], env=env3, capture_output=True, text=True, timeout=600)
    assert r3.returncode == 0 and "disk cache is disabled" in r3.stdout and not os.path.exists(str(tmp_path / "off")), r3.stdout + r3.stderr


def test_jit_compiles_in_a_compiler_process_and_gets_the_same_code_object(tmp_path):
    """hiprtc serialises the compilations of one process, so a compile worker hands its translation unit to `ldb_jitc` (built beside the library: the
    same embedded headers, the same compile()).  With the helper there the compilation is counted as done in a child (ldb_gpu_jit_info vals[9]);
    with LDB_JIT_CHILD=0 the worker thread compiles itself and the counter stays 0; the code object in the disk cache has the same name and the
    same bytes on both paths.  A unit hiprtc refuses is reported once, with the compiler's log, by the child alone.  Device-less."""
    import subprocess
    import sys

    assert os.access(os.path.join(ROOT, "lingo-db_amd", "ldb_jitc"), os.X_OK), "ldb_jitc was not built beside liblingodb_gpu.so"
    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from lingodb_amd import capi; lib = capi.gpu_lib(); buf = C.create_string_buffer(4000);"
            "st = lib.ldb_gpu_jit_cache_selftest(buf, 4000); v = (C.c_int64 * 10)(); lib.ldb_gpu_jit_info(v, 10); print(st, list(v), buf.value.decode())") % os.path.join(ROOT, "lingo-db_amd")

    def run(d, **extra):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LDB_JIT_CACHE_DIR=str(d), LDB_JIT_ASYNC="1", TMPDIR=str(tmp_path), **extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("0 "), r.stdout + r.stderr
        info = eval(r.stdout.split(" ", 1)[1].split("]")[0] + "]")
        files = sorted(os.path.join(p, f) for p, _, fs in os.walk(str(d)) for f in fs)
        assert len(files) == 1
        with open(files[0], "rb") as f:
            return info, os.path.relpath(files[0], str(d)), f.read()

    info_child, name_child, code_child = run(tmp_path / "child")
    info_thread, name_thread, code_thread = run(tmp_path / "thread", LDB_JIT_CHILD="0")
    assert info_child[9] == 1 and info_child[3] == 1 and info_child[5] == 0, info_child
    assert info_thread[9] == 0 and info_thread[3] == 1 and info_thread[5] == 0, info_thread
    assert name_child == name_thread and code_child == code_thread and code_child[:4] == b"\x7fELF"
    assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("ldb_jitc_")], "the compiler process's exchange directory was left behind"
    # the helper's own verdict on a unit that does not compile: exit status 1 and the compiler's log, nothing else written
    bad = tmp_path / "bad.hip"
    bad.write_text("#include \"ldb_gb_kernel.h\"\nthis is not C++;\n")
    r = subprocess.run([os.path.join(ROOT, "lingo-db_amd", "ldb_jitc"), str(bad), "gfx950", str(tmp_path / "bad.co"), str(tmp_path / "bad.log")], capture_output=True, timeout=600)
    assert r.returncode == 1 and not os.path.exists(str(tmp_path / "bad.co")) and "error" in (tmp_path / "bad.log").read_text()


def test_processes_sharing_a_jit_cache_compile_a_shape_once(tmp_path):
    """round 6: the ranks of a multi-GPU run meet the same kernel shapes at the same time and share one disk cache — a worker claims a shape
    (`<hash>.co.lock`) before compiling it, a worker of another process that finds the claim waits for the code object instead of compiling it again;
    a claim left behind by a dead process (older than five minutes) is ignored.  Without a device: hiprtc only."""
    import shutil
    import subprocess
    import sys
    import time

    code = ("import ctypes as C, sys; sys.path.insert(0, %r); from lingodb_amd import capi; lib = capi.gpu_lib(); buf = C.create_string_buffer(4000);"
            "st = lib.ldb_gpu_jit_cache_selftest(buf, 4000); v = (C.c_int64 * 9)(); lib.ldb_gpu_jit_info(v, 9); print(st, list(v), buf.value.decode())") % os.path.join(ROOT, "lingo-db_amd")

    def env_for(d):
        return dict(os.environ, LDB_JIT_CACHE_DIR=str(d), LDB_JIT_ASYNC="1")

    # a process of its own compiles the shape: the code object a "peer" will deliver below
    r = subprocess.run([sys.executable, "-c", code], env=env_for(tmp_path / "a"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("0 "), r.stdout + r.stderr
    made = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / "a")) for f in fs]
    assert len(made) == 1 and made[0].endswith(".co")
    rel = os.path.relpath(made[0], str(tmp_path / "a"))
    # a peer holds the claim: this process must wait for the peer's code object and compile nothing
    target = os.path.join(str(tmp_path / "b"), rel)
    os.makedirs(os.path.dirname(target))
    open(target + ".lock", "w").close()
    p = subprocess.Popen([sys.executable, "-c", code], env=env_for(tmp_path / "b"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    time.sleep(4.0)
    assert p.poll() is None, "the process did not wait for the peer's claim: " + p.stdout.read()
    shutil.copy(made[0], target + ".part")
    os.rename(target + ".part", target)
    os.unlink(target + ".lock")
    out, err = p.communicate(timeout=300)
    info = eval(out.split(" ", 1)[1].split("]")[0] + "]")
    assert info[8] == 1 and info[3] == 0 and info[5] == 0, (info, out, err)  # one code object taken from the peer, nothing written, nothing failed
    # a stale claim (its owner died): ignored, the shape is compiled here
    target_c = os.path.join(str(tmp_path / "c"), rel)
    os.makedirs(os.path.dirname(target_c))
    open(target_c + ".lock", "w").close()
    old = time.time() - 1000
    os.utime(target_c + ".lock", (old, old))
    r = subprocess.run([sys.executable, "-c", code], env=env_for(tmp_path / "c"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("0 "), r.stdout + r.stderr
    left = sorted(f for _, _, fs in os.walk(str(tmp_path / "c")) for f in fs)
    assert len(left) == 1 and left[0].endswith(".co"), left
