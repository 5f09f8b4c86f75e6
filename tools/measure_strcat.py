"""usage: python tools/measure_strcat.py [out.json] [rows]
ldb_gpu_map_strcat / ldb_gpu_map_strlen (csrc/ldb_strfn.hip) over two generated utf8 columns of 64 M rows each:
  phone    15 bytes per row, "NN-NNN-NNN-NNNN" — the shape of Q22's c_phone
  comment  20–120 bytes per row, and one 1 MB string per million rows
Per column four calls: a plain copy (one COL part), upper(col), 'store' || col || cast(k as varchar) with an int64 column k,
and length(col); and the BASELINE, the code the parent commit offers for a whole-string computed column:
ldb_gpu_map_substr(col, 1, 1 << 30), the row-per-lane kernels k_substr_lens / k_substr_fill.  Baseline and copy run in the
same process in three alternating rounds (baseline, copy, baseline, copy, …); every figure of a round is the median of 3
calls after 1 warm-up call, timed with HIP events around the whole call (lengths, scan, the read-back of the total, the
allocation of the result, the fill; the result is released outside the timed region).  Rates are bytes read + written
per second — value bytes in and out, 8 B of input offsets and 8 B of output offsets per row, 8 B per row of an integer
part — next to the copy ceiling measured in this run with the method of bench.py's hbm_ceiling (a device-to-device copy
of 4 GB, read + write)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lingo-db_amd"))
import numpy as np
import pyarrow as pa
import torch

import lingodb_amd as ldb
from lingodb_amd import capi

N = int(sys.argv[2]) if len(sys.argv) > 2 else 64 * 1024 * 1024
lib = capi.gpu_lib()
try:
    ctx = ldb.Context(0)
except capi.LdbError as e:
    sys.exit("measure_strcat: no GPU (%s): nothing measured, no file written" % e)
rng = np.random.default_rng(1)
med = lambda v: float(np.median(v))  # noqa: E731


def copy_ceiling(reps=5):
    n = 1 << 30
    a = torch.empty(n, dtype=torch.int32, device="cuda")
    b = torch.empty_like(a)
    a.fill_(1)
    b.copy_(a)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        b.copy_(a)
    ev1.record()
    torch.cuda.synchronize()
    return 2 * 4 * n * reps / (ev0.elapsed_time(ev1) * 1e-3)


def utf8(data, lens):
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    assert offs[-1] == len(data)
    return pa.Array.from_buffers(pa.large_utf8(), len(lens), [None, pa.py_buffer(offs), pa.py_buffer(data)])


def phone_column():
    block = rng.integers(48, 58, (1 << 20, 15), dtype=np.uint8)  # a million distinct rows, repeated
    block[:, [2, 6, 10]] = ord("-")
    data = np.resize(block.reshape(-1), N * 15)
    return utf8(data, np.full(N, 15, dtype=np.int64))


def comment_column():
    lens = rng.integers(20, 121, N).astype(np.int64)
    lens[np.arange(1 << 19, N, 1 << 20)] = 1 << 20  # one 1 MB string per million rows
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ ,.-", dtype=np.uint8)
    block = letters[rng.integers(0, len(letters), 1 << 26)]
    return utf8(np.resize(block, int(lens.sum())), lens)


def timed_once(run):
    run().release()  # warm-up
    ctx.sync()
    tm = ctx.timer()
    ms = []
    for _ in range(3):
        ctx.timer_start(tm)
        t = run()
        ctx.timer_stop(tm)
        ms.append(ctx.timer_ms(tm))
        t.release()
    return med(ms)


def kernels(run):
    ctx.prof_enable(True)
    ctx.prof_reset()
    run().release()
    ctx.sync()
    k = {name: round(v[1], 4) for name, v in ctx.prof_all().items() if v[0]}
    ctx.prof_enable(False)
    return k


ceiling = copy_ceiling()
out = {"rows": N, "device": ctx.device_info()["name"], "copy_ceiling_gbs": ceiling / 1e9,
       "method": "HIP events around the whole call, median of 3 after 1 warm-up per round; baseline (map_substr(col, 1, 1 << 30)) and the plain copy in three alternating rounds in "
                 "one process; bytes = value bytes read + written, 8 B input offsets + 8 B output offsets per row, 8 B per row of an integer part; kernel_ms = one profiled call"}
print("copy ceiling %.0f GB/s" % (ceiling / 1e9), flush=True)
lib.ldb_gpu_set_option(b"dict_encode", 0)
kvals = rng.integers(-(10 ** 9), 10 ** 12, N).astype(np.int64)
keys = ctx.register("m_keys", pa.table({"k": pa.array(kvals)}))
sample = kvals[: 1 << 20]
klen = int(round(float(np.char.str_len(sample.astype(str)).sum()) * N / len(sample)))  # bytes of the integer text (scaled from a sample of the column)
del kvals
for name, make in (("phone", phone_column), ("comment", comment_column)):
    col = make()
    vbytes = int(col.buffers()[2].size)
    t = ctx.register("m_" + name, pa.table({"s": col}))
    del col
    base_rel = t.rel()
    rel = base_rel.zip(keys)
    rec = {"value_bytes": vbytes}
    base = lambda: rel.map_substr((0, 0), 1, 1 << 30)  # noqa: E731
    copy = lambda: rel.map_strcat([{"col": (0, 0)}])  # noqa: E731
    rounds = []
    for _ in range(3):
        rounds.append({"baseline_substr_ms": timed_once(base), "strcat_copy_ms": timed_once(copy)})
        print(name, rounds[-1], flush=True)
    rec["rounds"] = rounds
    b, c = [r["baseline_substr_ms"] for r in rounds], [r["strcat_copy_ms"] for r in rounds]
    io = 2 * vbytes + 16 * N
    rec["baseline_substr"] = {"ms_median": med(b), "ms_min": min(b), "ms_max": max(b), "bytes": io, "gbs": io / (med(b) * 1e-3) / 1e9, "kernel_ms": kernels(base)}
    rec["copy"] = {"ms_median": med(c), "ms_min": min(c), "ms_max": max(c), "bytes": io, "gbs": io / (med(c) * 1e-3) / 1e9, "fraction_of_copy_ceiling": io / (med(c) * 1e-3) / ceiling,
                   "kernel_ms": kernels(copy)}
    rec["baseline_over_copy"] = med(b) / med(c)
    upper = lambda: rel.map_upper((0, 0))  # noqa: E731
    ms = timed_once(upper)
    rec["upper"] = {"ms": ms, "bytes": io, "gbs": io / (ms * 1e-3) / 1e9, "fraction_of_copy_ceiling": io / (ms * 1e-3) / ceiling, "kernel_ms": kernels(upper)}
    three = lambda: rel.map_strcat(["store", {"col": (0, 0)}, {"int": (1, 0)}])  # noqa: E731
    ms = timed_once(three)
    io3 = 2 * vbytes + 5 * N + klen + 24 * N
    rec["const_col_int"] = {"ms": ms, "bytes": io3, "gbs": io3 / (ms * 1e-3) / 1e9, "fraction_of_copy_ceiling": io3 / (ms * 1e-3) / ceiling, "kernel_ms": kernels(three)}
    length = lambda: rel.map_strlen((0, 0))  # noqa: E731
    ms = timed_once(length)
    iol = vbytes + 16 * N
    rec["length"] = {"ms": ms, "bytes": iol, "gbs": iol / (ms * 1e-3) / 1e9, "fraction_of_copy_ceiling": iol / (ms * 1e-3) / ceiling, "kernel_ms": kernels(length)}
    out[name] = rec
    print(name, json.dumps(rec), flush=True)
    rel.release()
    base_rel.release()
    t.release()
lib.ldb_gpu_set_option(b"dict_encode", 1)
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strcat_64m.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
keys.release()
ctx.close()
