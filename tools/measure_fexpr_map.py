"""usage: python tools/measure_fexpr_map.py [out.json]
k_map_fexpr (f32 / f64 a*b+c) against k_map_expr (int64 a*b+c) at 64 M dense rows, specialised kernels: median of 10 after 3 warm-ups"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lingo-db_amd"))
import numpy as np
import pyarrow as pa

import lingodb_amd as ldb
from lingodb_amd import capi

N = 64 * 1024 * 1024
lib = capi.gpu_lib()
lib.ldb_gpu_set_option(b"jit_min_rows", 0)
lib.ldb_gpu_set_option(b"jit_async", 0)
ctx = ldb.Context(0)
base = np.arange(N, dtype=np.int64)
out = {"rows": N, "device": ctx.device_info()["name"], "method": "ldb_gpu_prof_*: median of 10 launches after 3 warm-ups, specialised kernels, same process"}
progs = {"f32": (pa.float32(), np.float32, capi.T_FLOAT32, ("fmul",), ("fadd",), "k_map_fexpr", 16),
         "f64": (pa.float64(), np.float64, capi.T_FLOAT64, ("fmul",), ("fadd",), "k_map_fexpr", 32),
         "int64": (pa.int64(), np.int64, capi.T_INT64, ("mul",), ("add",), "k_map_expr", 32)}
for name, (ty, dt, ot, mul, add, kern, bpr) in progs.items():
    t = ctx.register("m_" + name, pa.table({"a": pa.array((base % 1000).astype(dt), ty), "b": pa.array((base % 77).astype(dt), ty), "c": pa.array((base % 13).astype(dt), ty)}))
    rel = t.rel()
    prog = [("col", (0, 0)), ("col", (0, 1)), mul, ("col", (0, 2)), add]
    for _ in range(3):
        rel.map_expr(prog, ot).release()
    pend = C.c_int64()
    lib.ldb_gpu_jit_wait(60000, C.byref(pend))
    ctx.prof_enable(True)
    ms = []
    packs = 0
    for _ in range(10):
        ctx.prof_reset()
        rel.map_expr(prog, ot).release()
        allp = ctx.prof_all()
        ms.append(allp[kern][1])
    ctx.prof_enable(False)
    ms.sort()
    med = (ms[4] + ms[5]) / 2
    out[name] = {"kernel": kern, "ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "bytes_per_row": bpr, "GBps": bpr * N / med / 1e6, "prof_names": sorted(allp)}
    print(name, out[name], flush=True)
    del rel
    t.release()
a, b, msj = C.c_int64(), C.c_int64(), C.c_double()
lib.ldb_gpu_jit_stats(C.byref(a), C.byref(b), C.byref(msj))
out["jit"] = {"compiled": a.value, "hits": b.value}
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fexpr_map_64m.json")
json.dump(out, open(dest, "w"), indent=1)
ctx.close()
