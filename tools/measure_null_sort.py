"""usage: python tools/measure_null_sort.py [out.json] [rows]
What the NULL flag byte of a sort key costs (csrc/ldb_sort.hip): ldb_gpu_sort of 10 M rows by ONE int64 key with LDB_NULLS_LARGEST,
  null_free — the key holds no NULL (a validity bitmap with every bit set): no flag byte, an 8-byte record = one 64-bit word,
  nullable  — the same values, one row in a hundred NULL: flag byte + 8 value bytes = a 9-byte record = two 64-bit words, and one more
              4-bit radix pass (the flag's nibble varies).
HIP-event time around the whole call, median of 10 after 3 warm-ups, same process."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lingo-db_amd"))
import numpy as np
import pyarrow as pa

import lingodb_amd as ldb
from lingodb_amd import api, capi

N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
try:
    ctx = ldb.Context(0)
except capi.LdbError as e:
    sys.exit("measure_null_sort: no GPU (%s): nothing measured, no file written" % e)
rng = np.random.default_rng(1)
values = rng.integers(-(2 ** 63), 2 ** 63 - 1, N, endpoint=True)
valid = {"null_free": np.ones(N, dtype=bool), "nullable": rng.random(N) >= 0.01}
out = {"rows": N, "device": ctx.device_info()["name"], "cmd": "python tools/measure_null_sort.py",
       "method": "ldb_gpu_sort by one int64 key, nulls = LDB_NULLS_LARGEST: HIP events around the call, median of 10 after 3 warm-ups, same process"}
for name in ("null_free", "nullable"):
    bitmap = np.packbits(valid[name], bitorder="little").tobytes()
    key = pa.Array.from_buffers(pa.int64(), N, [pa.py_buffer(bitmap), pa.py_buffer(values)], null_count=int(N - valid[name].sum()))
    t = ctx.register("ns_" + name, pa.table({"k": key}))
    rel = t.rel()
    specs = [api.sort_spec((0, 0), False, capi.NULLS_LARGEST)]
    for _ in range(3):
        rel.sort(specs).release()
    ctx.sync()
    tm = ctx.timer()
    ms = []
    for _ in range(10):
        ctx.timer_start(tm)
        s = rel.sort(specs)
        ctx.timer_stop(tm)
        ms.append(ctx.timer_ms(tm))
        s.release()
    out[name] = {"nulls": int(N - valid[name].sum()), "ms_call_median": float(np.median(ms)), "ms_call_min": min(ms), "ms_call_max": max(ms)}
    print(name, out[name], flush=True)
    del rel
    t.release()
out["nullable_over_null_free"] = out["nullable"]["ms_call_median"] / out["null_free"]["ms_call_median"]
print("ratio", out["nullable_over_null_free"], flush=True)
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "null_sort_10m.json")
json.dump(out, open(dest, "w"), indent=1)
ctx.close()
