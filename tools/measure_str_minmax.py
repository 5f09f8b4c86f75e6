"""usage: python tools/measure_str_minmax.py [out.json] [rows]
key-less MIN + MAX over one utf8 column (k_str_minmax_prefix + k_str_minmax_resolve, csrc/ldb_strminmax.hip) at 64 M generated rows:
  random   — random 8–40-byte strings
  prefix12 — every row shares a 12-byte prefix (all rows tie in the prefix pass: each is a candidate of the resolve pass)
  dict     — a dictionary-encoded column (the kernels compare the 4-byte codes)
Per case: HIP-event time around the whole call and the two kernels' own times (ldb_gpu_prof_*), median of 10 after 3 warm-ups; the bytes
the prefix pass must read for BOTH aggregates (each reads 8 B of offsets plus one 64-byte line per row; 4 B per row over codes) and the
fraction of 8 TB/s that is."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lingo-db_amd"))
import numpy as np
import pyarrow as pa

import lingodb_amd as ldb
from lingodb_amd import api, capi

N = int(sys.argv[2]) if len(sys.argv) > 2 else 64 * 1024 * 1024
PEAK = 8e12  # bytes / s
lib = capi.gpu_lib()
try:
    ctx = ldb.Context(0)
except capi.LdbError as e:
    sys.exit("measure_str_minmax: no GPU (%s): nothing measured, no file written" % e)
rng = np.random.default_rng(1)


def utf8(lengths, data):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return pa.Array.from_buffers(pa.large_utf8(), len(lengths), [None, pa.py_buffer(off), pa.py_buffer(data)])


def random_strings():
    lengths = rng.integers(8, 41, N).astype(np.int64)
    return utf8(lengths, rng.integers(97, 123, int(lengths.sum()), dtype=np.uint8))


def shared_prefix():
    lengths = rng.integers(12, 41, N).astype(np.int64)
    off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    for j, ch in enumerate(b"twelve bytes"):
        data[off[:-1] + j] = ch
    return utf8(lengths, data)


def dictionary():
    words = np.frombuffer(b"".join(b"word%04d-xyz" % i for i in range(1000)), dtype=np.uint8).reshape(1000, 12)  # 1000 distinct 12-byte strings
    return utf8(np.full(N, 12, dtype=np.int64), words[rng.integers(0, 1000, N)].ravel())


out = {"rows": N, "device": ctx.device_info()["name"], "peak_Bps": PEAK,
       "method": "one groupby call with MIN and MAX: HIP events around the call and ldb_gpu_prof_* per kernel, median of 10 after 3 warm-ups, same process"}
for name, make, encode, bpr in (("random", random_strings, False, 72), ("prefix12", shared_prefix, False, 72), ("dict", dictionary, True, 4)):
    lib.ldb_gpu_set_option(b"dict_encode", 0)
    t = ctx.register("m_" + name, pa.table({"s": make()}))
    lib.ldb_gpu_set_option(b"dict_encode", 1)
    if encode:
        assert t.dict_encode(0) > 0
    rel = t.rel()
    aggs = [api.str_minmax(capi.AGG_MIN, (0, 0)), api.str_minmax(capi.AGG_MAX, (0, 0))]
    for _ in range(3):
        rel.groupby([], aggs).release()
    ctx.sync()
    tm = ctx.timer()
    ctx.prof_enable(True)
    ms, pre, res = [], [], []
    for _ in range(10):
        ctx.prof_reset()
        ctx.timer_start(tm)
        rel.groupby([], aggs).release()
        ctx.timer_stop(tm)
        ms.append(ctx.timer_ms(tm))
        allp = ctx.prof_all()
        pre.append(allp["k_str_minmax_prefix"][1])
        res.append(allp["k_str_minmax_resolve"][1])
    ctx.prof_enable(False)
    med = lambda v: float(np.median(v))  # noqa: E731
    must = 2 * bpr * N  # two aggregates, each a pass of its own over the column
    out[name] = {"ms_call_median": med(ms), "ms_call_min": min(ms), "ms_call_max": max(ms), "ms_prefix_median": med(pre), "ms_resolve_median": med(res),
                 "prefix_bytes": must, "prefix_fraction_of_peak": must / (med(pre) * 1e-3) / PEAK}
    print(name, out[name], flush=True)
    del rel
    t.release()
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "str_minmax_64m.json")
json.dump(out, open(dest, "w"), indent=1)
ctx.close()
