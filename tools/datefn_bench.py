"""usage: python tools/datefn_bench.py [out.json] [rows]
ldb_gpu_map_datefn (csrc/ldb_datefn.hip) over a dense date32 column and a dense int64 ns column of 2^28 rows, against the
BASELINE, code this kernel does not touch: ldb_gpu_map_column's extract(year) (k_map_column in csrc/ldb_hash.hip, one row
per lane, 64-bit divisions).  Five calls:
  a  map_column  extract year   date32 → int64     (the baseline)
  b  map_datefn  EXTRACT year   date32 → int64
  c  map_datefn  EXTRACT month  date32 → int64
  d  map_datefn  TRUNC month    date32 → date32
  e  map_datefn  EXTRACT month  int64 ns → int64
One process, ROUNDS rounds, the five interleaved in every round (a b c d e, a b c d e, …); the figure of a call in a round is
the median of 20 calls after one warm-up, each timed with device events around the whole call (allocation of the result
and the launch; the result is released outside the timed region).  A call's figure is the median of its round medians;
the SPREAD of the baseline is the distance between its largest and smallest round median, and b and c pass when their
figure is no larger than the baseline's plus that spread.  Rates are bytes read + written per second (4 or 8 B in, 4 or
8 B out per row) beside the copy ceiling measured in this run with the method of bench.py's hbm_ceiling (a device-to-device
copy of 4 GB, read + write).  Without a GPU nothing is measured and no file is written."""
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

N = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 28
ROUNDS, CALLS = 5, 20
try:
    ctx = ldb.Context(0)
except capi.LdbError as e:
    sys.exit("datefn_bench: no GPU (%s): nothing measured, no file written" % e)
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


def timed(run):
    run().release()  # warm-up
    ctx.sync()
    tm = ctx.timer()
    ms = []
    for _ in range(CALLS):
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
print("copy ceiling %.0f GB/s" % (ceiling / 1e9), flush=True)
rng = np.random.default_rng(1)
block = rng.integers(-25567, 47482, 1 << 22, dtype=np.int32)  # 1900 … 2099, a few million distinct rows, repeated
days = np.resize(block, N)
t = ctx.register("datefn_bench", pa.table({"d": pa.array(days).cast(pa.date32()), "t": pa.array(days.astype(np.int64) * 86_400_000_000_000 + np.resize(rng.integers(0, 86_400_000_000_000, 1 << 22), N))}))
del days
rel = t.rel()
calls = [("a_map_column_extract_year", lambda: rel.map_column((0, 0)), 12), ("b_datefn_extract_year", lambda: rel.map_datefn((0, 0), capi.DF_EXTRACT, capi.DP_YEAR), 12),
         ("c_datefn_extract_month", lambda: rel.map_datefn((0, 0), capi.DF_EXTRACT, capi.DP_MONTH), 12), ("d_datefn_trunc_month", lambda: rel.map_datefn((0, 0), capi.DF_TRUNC, capi.DP_MONTH), 8),
         ("e_datefn_extract_month_ns", lambda: rel.map_datefn((0, 1), capi.DF_EXTRACT, capi.DP_MONTH), 16)]
# the two ways to a year agree before anything is timed (a sample: the full columns are 2 GB each)
ya, yb = rel.map_column((0, 0)), rel.map_datefn((0, 0), capi.DF_EXTRACT, capi.DP_YEAR)
assert np.array_equal(ya.read_fixed(0)[: 1 << 20], yb.read_fixed(0)[: 1 << 20])
ya.release(), yb.release()
rounds = {name: [] for name, _, _ in calls}
for r in range(ROUNDS):
    for name, run, _ in calls:
        rounds[name].append(timed(run))
    print("round %d: %s" % (r, " ".join("%s=%.3f" % (name[0], rounds[name][-1]) for name, _, _ in calls)), flush=True)
out = {"rows": N, "device": ctx.device_info()["name"], "copy_ceiling_gbs": round(ceiling / 1e9, 1), "rounds": ROUNDS, "calls_per_round": CALLS,
       "method": "device events around the whole call; per round the median of 20 calls after 1 warm-up, the five calls interleaved in every round of one process; ms = median of the round "
                 "medians; baseline spread = max - min of the baseline's round medians; bytes = values read + written; kernel_ms = one profiled call"}
for name, run, per_row in calls:
    m = med(rounds[name])
    out[name] = {"ms": round(m, 4), "round_ms": [round(x, 4) for x in rounds[name]], "bytes": per_row * N, "gbs": round(per_row * N / (m * 1e-3) / 1e9, 1),
                 "fraction_of_copy_ceiling": round(per_row * N / (m * 1e-3) / ceiling, 3), "kernel_ms": kernels(run)}
base = out["a_map_column_extract_year"]
spread = max(base["round_ms"]) - min(base["round_ms"])
out["baseline_spread_ms"] = round(spread, 4)
for name in ("b_datefn_extract_year", "c_datefn_extract_month"):
    out[name]["no_slower_than_baseline"] = bool(out[name]["ms"] <= base["ms"] + spread)
    out[name]["baseline_over_this"] = round(base["ms"] / out[name]["ms"], 3)
print(json.dumps(out), flush=True)
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "datefn_map.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
rel.release()
t.release()
ctx.close()
