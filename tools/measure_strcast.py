"""usage: python tools/measure_strcast.py [out.json] [rows] [a]
The casts between text and int / decimal / date (csrc/ldb_strcast.h, ldb_strcast.hip, the number parts of ldb_strfn.hip) over
generated columns of 64 M rows, with the method of tools/measure_strcat.py: HIP events around whole calls, the median of 3
calls after 1 warm-up, one process, and the copy ceiling of the same run (a device-to-device copy of 4 GB, read + write).
  (a) 'store' || phone || cast(k as varchar) — phone 15 bytes per row, k an int64 column: the INT part, whose digits now
      come from the shared helper; three rounds.  With a third argument `a` ONLY this is measured and printed, through calls
      the parent commit has too: run the tool that way from a checkout of each commit, alternating, to compare the two.
  (b) to_varchar of a decimal(12,2) column and of a date column (one DECIMAL / DATE part), next to the plain copy of `phone`
      (one COL part) of the same run: time, and GB/s of OUTPUT value bytes.
  (c) the three parses over valid text — INT64 over 15 digits, DECIMAL(14,2) over "NNNNNNNNNNNN.NN" (15 bytes), DATE over
      "YYYY-MM-DD" (a valid date has 10 bytes) — next to ldb_gpu_map_strlen (k_strlen, the read-bound yardstick) on the same
      column: call time, kernel time of one profiled call, and bytes (value bytes + 8 B offsets in, values + validity out) per
      second of kernel time as a fraction of the copy ceiling."""
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
ONLY_A = len(sys.argv) > 3 and sys.argv[3] == "a"
lib = capi.gpu_lib()
try:
    ctx = ldb.Context(0)
except capi.LdbError as e:
    sys.exit("measure_strcast: no GPU (%s): nothing measured, no file written" % e)
rng = np.random.default_rng(1)
med = lambda v: float(np.median(v))  # noqa: E731
BLOCK = 1 << 20  # distinct rows, repeated


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
    del a, b
    torch.cuda.empty_cache()
    return 2 * 4 * n * reps / (ev0.elapsed_time(ev1) * 1e-3)


def fixed_utf8(block):
    """a utf8 column of N rows from a (BLOCK, width) array of bytes, repeated"""
    w = block.shape[1]
    data = np.resize(block.reshape(-1), N * w)
    offs = np.arange(N + 1, dtype=np.int64) * w
    return pa.Array.from_buffers(pa.large_utf8(), N, [None, pa.py_buffer(offs), pa.py_buffer(data)]), N * w


def digits(width):
    b = rng.integers(48, 58, (BLOCK, width), dtype=np.uint8)
    b[:, 0] = rng.integers(49, 58, BLOCK, dtype=np.uint8)  # no leading zero
    return b


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
       "method": "HIP events around the whole call, median of 3 after 1 warm-up; one process; kernel_ms = one profiled call"}
print("copy ceiling %.0f GB/s" % (ceiling / 1e9), flush=True)
lib.ldb_gpu_set_option(b"dict_encode", 0)

# ---------------------------------------------------------------- (a) the INT part
phone_block = rng.integers(48, 58, (BLOCK, 15), dtype=np.uint8)
phone_block[:, [2, 6, 10]] = ord("-")
col, phone_bytes = fixed_utf8(phone_block)
phone = ctx.register("m_phone", pa.table({"s": col}))
del col
kvals = rng.integers(-(10 ** 9), 10 ** 12, N).astype(np.int64)
keys = ctx.register("m_keys", pa.table({"k": pa.array(kvals)}))
klen = int(round(float(np.char.str_len(kvals[:BLOCK].astype(str)).sum()) * N / BLOCK))  # bytes of the integer text (scaled from a sample)
del kvals
base_rel = phone.rel()
rel = base_rel.zip(keys)
three = lambda: rel.map_strcat(["store", {"col": (0, 0)}, {"int": (1, 0)}])  # noqa: E731
rounds = [timed_once(three) for _ in range(3)]
io3 = 2 * phone_bytes + 5 * N + klen + 24 * N
out["const_col_int"] = {"rounds_ms": rounds, "ms_median": med(rounds), "bytes": io3, "gbs": io3 / (med(rounds) * 1e-3) / 1e9, "kernel_ms": kernels(three)}
print("const_col_int", json.dumps(out["const_col_int"]), flush=True)
if ONLY_A:
    sys.stdout.flush()
    rel.release(), base_rel.release(), keys.release(), phone.release()
    ctx.close()
    sys.exit(0)


def text_out(name, run, out_bytes):
    ms = timed_once(run)
    rec = {"ms": ms, "output_value_bytes": out_bytes, "output_gbs": out_bytes / (ms * 1e-3) / 1e9, "kernel_ms": kernels(run)}
    out[name] = rec
    print(name, json.dumps(rec), flush=True)


# ---------------------------------------------------------------- (b) numbers and dates as text, next to the plain copy
text_out("copy_phone", lambda: rel.map_strcat([{"col": (0, 0)}]), phone_bytes)
rel.release(), base_rel.release(), keys.release()
unscaled = rng.integers(-(10 ** 9), 10 ** 12, BLOCK).astype(np.int64)  # decimal(12,2): -10 000 000.00 … 10 000 000 000.00
dec_len = int(sum(len("%d.%02d" % divmod(abs(int(v)), 100)) + (v < 0) for v in unscaled[: 1 << 16])) * (N >> 16)
words = np.empty((BLOCK, 2), dtype=np.int64)
words[:, 0] = unscaled
words[:, 1] = unscaled >> 63
dec = pa.Array.from_buffers(pa.decimal128(12, 2), N, [None, pa.py_buffer(np.resize(words.reshape(-1), 2 * N))])
days = np.resize(rng.integers(-25000, 25000, BLOCK).astype(np.int32), N)
nums = ctx.register("m_nums", pa.table({"d": dec, "e": pa.array(days).cast(pa.date32())}))
del dec, days, words
nrel = nums.rel()
text_out("to_varchar_decimal_12_2", lambda: nrel.map_strcat([{"dec": (0, 0)}]), dec_len)
text_out("to_varchar_date", lambda: nrel.map_strcat([{"date": (0, 1)}]), 10 * N)
nrel.release(), nums.release(), phone.release()

# ---------------------------------------------------------------- (c) the parses, next to k_strlen on the same column
dec_block = digits(15)
dec_block[:, 12] = ord(".")
date_block = np.frombuffer("".join(np.datetime_as_string((np.arange(BLOCK) - 300000).astype("datetime64[D]"))).encode(), dtype=np.uint8).reshape(BLOCK, 10)
for name, block, kind, p, s, width in (("to_int", digits(15), capi.PARSE_INT64, 0, 0, 8), ("to_decimal_14_2", dec_block, capi.PARSE_DECIMAL, 14, 2, 16), ("to_date", date_block, capi.PARSE_DATE, 0, 0, 4)):
    col, vbytes = fixed_utf8(np.ascontiguousarray(block))
    t = ctx.register("m_" + name, pa.table({"s": col}))
    del col
    r = t.rel()
    bad = r.map_strparse((0, 0), kind, p, s)
    assert bad[1] == 0, (name, bad[1])  # (valid text only)
    bad[0].release()
    parse = lambda: r.map_strparse((0, 0), kind, p, s, count_bad=False)[0]  # noqa: E731
    length = lambda: r.map_strlen((0, 0))  # noqa: E731
    rec = {"value_bytes": vbytes}
    for what, run, kname, io in (("parse", parse, "k_strparse", vbytes + 8 * N + width * N + N // 8), ("strlen", length, "k_strlen", vbytes + 8 * N + 8 * N)):
        ms, k = timed_once(run), kernels(run)
        rec[what] = {"ms": ms, "kernel_ms": k, "bytes": io, "kernel_gbs": io / (k[kname] * 1e-3) / 1e9, "kernel_fraction_of_copy_ceiling": io / (k[kname] * 1e-3) / ceiling}
    rec["parse_kernel_over_strlen_kernel"] = rec["parse"]["kernel_ms"]["k_strparse"] / rec["strlen"]["kernel_ms"]["k_strlen"]
    out[name] = rec
    print(name, json.dumps(rec), flush=True)
    r.release(), t.release()
lib.ldb_gpu_set_option(b"dict_encode", 1)
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strcast_64m.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
ctx.close()
