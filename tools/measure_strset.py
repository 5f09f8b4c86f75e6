"""usage: python tools/measure_strset.py [out.json] [rows]
`s IN (constants)` over one utf8 column of 64 M generated rows (random 8–40-byte strings drawn from a vocabulary of 100 000), through
ldb_gpu_scan_filter:
  inline8_generic / inline8_spec — the inline descriptor's 8-constant list in k_scan_bitmap, generic and specialised at run time (the path
                                   every list of <= 8 constants takes by default; unchanged by the string-set kernel)
  strset8                        — the same 8 constants through k_strset_bitmap_lds, forced by scan_strset_min_in = 1
  strset10 … strset10000         — 10, 100, 1 000 and 10 000 constants (the last one is searched in global memory: k_strset_bitmap_glb)
  strset1000_long                — 1 000 constants whose members are all >= 32 bytes long: every member row compares >= 24 bytes behind the eighth,
                                   one byte at a time, against the blob
  cmp_gte_100                    — `s >= c` with a 100-byte constant that starts with a 40-byte member of the vocabulary (rows equal to that member
                                   walk their whole tail)
Half of every list is drawn from the vocabulary, half are non-members; the membership rate of the rows is stated per case.
Per case: HIP-event time around the whole call and the bitmap kernel's own time (ldb_gpu_prof_*), median of 10 after 3 warm-ups, and that
kernel's rate over the bytes it must read — 8 B of offsets per row, the first min(8, length) bytes of every row, the bytes behind the eighth
of the member rows — as a fraction of a scan ceiling measured IN THIS RUN: the library's count-only scan (k_scan_count, specialised) over an
8-byte column of 8 x as many rows (4 GB at the default size).  That is the kernel and the method of hbm_ceiling.scan_count_gbs of
bench.py --full, but not that figure itself, which is taken over the 9.6 GB of SF100's l_extendedprice in another process; the record
names the last committed bench figure beside its own (`bench_full_scan_count_gbs_recorded`), so both can be read."""
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
VOCAB = 100_000
lib = capi.gpu_lib()
try:
    ctx = ldb.Context(0)
except capi.LdbError as e:
    sys.exit("measure_strset: no GPU (%s): nothing measured, no file written" % e)
rng = np.random.default_rng(1)

vlen = rng.integers(8, 41, VOCAB)
vocab = sorted({bytes(rng.integers(97, 123, int(n), dtype=np.uint8)) for n in vlen})
idx = rng.integers(0, len(vocab), N)
col = pa.array(vocab, pa.large_binary()).take(pa.array(idx)).view(pa.large_utf8())
lens = np.array([len(v) for v in vocab], dtype=np.int64)
row_len = lens[idx]
lib.ldb_gpu_set_option(b"dict_encode", 0)
t = ctx.register("m_strset", pa.table({"s": col}))
big = ctx.register("m_ceiling", pa.table({"v": pa.array(np.arange(8 * N, dtype=np.int64))}))
lib.ldb_gpu_set_option(b"dict_encode", 1)
del col
rel = t.rel()
med = lambda v: float(np.median(v))  # noqa: E731


def timed(run, kernel):
    for _ in range(3):
        run()
    ctx.sync()
    tm = ctx.timer()
    ctx.prof_enable(True)
    ms, kms = [], []
    for _ in range(10):
        ctx.prof_reset()
        ctx.timer_start(tm)
        run()
        ctx.timer_stop(tm)
        ms.append(ctx.timer_ms(tm))
        kms.append(ctx.prof_all()[kernel][1])
    ctx.prof_enable(False)
    return {"ms_call_median": med(ms), "ms_call_min": min(ms), "ms_call_max": max(ms), "ms_kernel_median": med(kms), "kernel": kernel}


# the ceiling: count-only scan over the 8-byte column (specialised, as in bench.py's hbm_ceiling)
lib.ldb_gpu_set_option(b"jit_async", 0)  # a specialisation is compiled before the first launch of its shape, not beside it
lib.ldb_gpu_set_option(b"lazy_filter", 0)  # every filter is evaluated where it is called (a dense 64 M-row input would otherwise carry the inline conjunct along unevaluated)
brel = big.rel()
ceil = timed(lambda: brel.scan_count([api.pred((0, 0), capi.F_GTE, 0)]), "k_scan_count")
ceiling_bps = 8 * 8 * N / (ceil["ms_kernel_median"] * 1e-3)
del brel
big.release()
out = {"rows": N, "vocabulary": len(vocab), "device": ctx.device_info()["name"], "scan_ceiling": dict(ceil, rows=8 * N, bytes=8 * 8 * N, gbs=ceiling_bps / 1e9),
       "bench_full_scan_count_gbs_recorded": {"gbs": 5768.1, "source": "profiles/r06_bench_sf100_second_process_start.json (hbm_ceiling.scan_count_gbs; not measured in this run)"},
       "method": "one scan_filter call: HIP events around the call and ldb_gpu_prof_* for the bitmap kernel, median of 10 after 3 warm-ups, same process; "
                 "bytes = 8 B offsets + min(8, length) per row + the tail bytes of member rows"}
print("ceiling", out["scan_ceiling"], flush=True)


def constants(k):
    """half members, half not; the 8-constant list must fit the inline descriptor's 128 bytes: members of <= 20 bytes, 8-byte non-members"""
    pool = np.nonzero(lens <= 20)[0] if k <= 8 else np.arange(len(vocab))
    pick = rng.choice(pool, k // 2, replace=False)
    miss = b"#%07d" if k <= 8 else b"#%07d not in the vocabulary"
    return [vocab[int(j)] for j in pick] + [miss % i for i in range(k - k // 2)], pick


def case(name, k, min_in, jit, kernel, consts=None, pick=None, cmp=None):
    """cmp = (op, constant, numpy predicate over the vocabulary index → passes, → walks its tail): a comparison instead of a list"""
    if consts is None and cmp is None:
        consts, pick = constants(k)
    if cmp is None:
        member = np.zeros(len(vocab), dtype=bool)
        member[pick] = True
        is_member = walks = member[idx]
        plist = lambda: [api.pred((0, 0), capi.F_IN, values=consts)]  # noqa: E731
    else:
        is_member, walks = cmp[2][idx], cmp[3][idx]
        plist = lambda: [api.pred((0, 0), cmp[0], cmp[1])]  # noqa: E731
    must = 8 * N + int(np.minimum(row_len, 8).sum()) + int(np.maximum(row_len[walks] - 8, 0).sum())
    lib.ldb_gpu_set_option(b"scan_strset_min_in", min_in)
    lib.ldb_gpu_set_option(b"jit", jit)
    try:
        r = timed(lambda: rel.scan_filter(plist()).release(), kernel)
        rows = rel.scan_filter(plist()).rows
    finally:
        lib.ldb_gpu_set_option(b"scan_strset_min_in", 9)
        lib.ldb_gpu_set_option(b"jit", 1)
    assert rows == int(is_member.sum()), (name, rows, int(is_member.sum()))
    r.update({"constants": k, "passing_rows": rows, "membership_rate": rows / N, "bytes": must, "gbs": must / (r["ms_kernel_median"] * 1e-3) / 1e9,
              "fraction_of_scan_ceiling": must / (r["ms_kernel_median"] * 1e-3) / ceiling_bps})
    out[name] = r
    print(name, r, flush=True)
    return consts, pick


c8, p8 = case("inline8_generic", 8, 9, 0, "k_scan_bitmap")
case("inline8_spec", 8, 9, 1, "k_scan_bitmap", c8, p8)
case("strset8", 8, 1, 1, "k_strset_bitmap_lds", c8, p8)
for k in (10, 100, 1000, 10000):
    case("strset%d" % k, k, 9, 1, "k_strset_bitmap_lds" if k <= 5376 else "k_strset_bitmap_glb")
# long tails: 1 000 constants, the members among them all >= 32 bytes
long_pool = np.nonzero(lens >= 32)[0]
lp = rng.choice(long_pool, 500, replace=False)
case("strset1000_long", 1000, 9, 1, "k_strset_bitmap_lds", [vocab[int(j)] for j in lp] + [b"#%07d not in the vocabulary, and long" % i for i in range(500)], lp)
# a comparison with a 100-byte constant: a 40-byte member + 60 bytes (every row equal to that member is a proper prefix: smaller, after walking its tail)
j40 = int(np.nonzero(lens == 40)[0][len(vocab) // 40])
c100 = vocab[j40] + b"z" * 60
vi = np.arange(len(vocab))
case("cmp_gte_100", 1, 9, 1, "k_strset_bitmap_lds", cmp=(capi.F_GTE, c100, vi > j40, vi == j40))  # (the vocabulary is sorted: index order is string order)
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strset_64m.json")
json.dump(out, open(dest, "w"), indent=1)
del rel
t.release()
ctx.close()
