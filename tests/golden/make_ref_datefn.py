"""Generates tests/golden/ref_datefn.json by calling the REFERENCE'S OWN date runtime — DateRuntime::extractYear … extractSecond,
dateTrunc, addMonths, subtractMonths and dateDiffDay / Hour / Minute / Second, as compiled unmodified into
oracle/_ref/libldb_ref.so — on seeded and hand-picked instants (int64 ns since the epoch, the reference's representation of
dates and timestamps alike).  A few lines of glue of our own (below) are compiled against the reference's headers into
oracle/_ref/ at generation time; nothing of it is committed.  The fixture is data only: the inputs and the recorded outputs.
tests/test_datefn_api.py pins the Python restatement (tests/datefn_eval.py) to it, tests/test_gpu_datefn.py the device kernels.

Outside the reference's own domain nothing is recorded: dateTrunc of an instant before 1678-01-01 and a month shift or a
difference that leaves int64 are signed overflow there (`trunc` holds null for such an instant; the month shifts and the
differences are taken where they fit).

Run from the repo root where oracle/_ref has been built:  python tests/golden/make_ref_datefn.py"""
import ctypes as C
import datetime
import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("LDB_REFERENCE_DIR", "/root/reference")

GLUE = r"""
#include "lingodb/runtime/DateRuntime.h"
#include "lingodb/runtime/helpers.h"
#include <cstdint>
using namespace lingodb;
extern "C" {
int64_t glue_extract(int32_t part, int64_t ns) {
   switch (part) {
      case 0: return runtime::DateRuntime::extractYear(ns);
      case 1: return runtime::DateRuntime::extractMonth(ns);
      case 2: return runtime::DateRuntime::extractDay(ns);
      case 3: return runtime::DateRuntime::extractHour(ns);
      case 4: return runtime::DateRuntime::extractMinute(ns);
      default: return runtime::DateRuntime::extractSecond(ns);
   }
}
int64_t glue_trunc(const char* part, int64_t n, int64_t ns) { return runtime::DateRuntime::dateTrunc(runtime::VarLen32::fromDataAndLen(part, (size_t) n, runtime::StorageClass::TRANSIENT), ns); }
int64_t glue_add(int64_t ns, int64_t months) { return runtime::DateRuntime::addMonths(ns, months); }
int64_t glue_sub(int64_t ns, int64_t months) { return runtime::DateRuntime::subtractMonths(ns, months); }
int64_t glue_diff(int32_t unit, int64_t end, int64_t start) {
   switch (unit) {
      case 2: return runtime::DateRuntime::dateDiffDay(end, start);
      case 3: return runtime::DateRuntime::dateDiffHour(end, start);
      case 4: return runtime::DateRuntime::dateDiffMinute(end, start);
      default: return runtime::DateRuntime::dateDiffSecond(end, start);
   }
}
}
"""

PARTS = ("year", "month", "day", "hour", "minute", "second")
NS_PER_DAY = 86_400_000_000_000
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
MONTHS = (0, 1, -1, 11, -11, 12, -12, 13, -13, 25, -120)


def build_glue():
    src = os.path.join(REF_DIR, "datefn_glue.cpp")
    so = os.path.join(REF_DIR, "libdatefn_glue.so")
    with open(src, "w") as f:
        f.write(GLUE)
    ref = os.path.join(REF_DIR, "libldb_ref.so")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-w", "-DENABLE_REFCOUNT=1", "-I" + os.path.join(ROOT, "oracle", "ref_build", "shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + os.path.join(REFERENCE, "vendored"), "-I" + pa.get_include(), src, "-o", so, ref,
                           "-Wl,-rpath," + REF_DIR, "-Wl,-rpath," + pa.get_library_dirs()[0]])
    return C.CDLL(so)


def ns_of(y, m, d, hh=0, mm=0, ss=0, frac=0):
    return (datetime.date(y, m, d) - datetime.date(1970, 1, 1)).days * NS_PER_DAY + (hh * 3600 + mm * 60 + ss) * 1_000_000_000 + frac


def time_of_day(rng):
    return int(rng.integers(0, NS_PER_DAY))


def last_day(y, m):
    return (datetime.date(y + (m == 12), m % 12 + 1, 1) - datetime.timedelta(days=1)).day


def instants(rng):
    v = [0, 1, -1, 1_000_000_000, -1_000_000_000, 1_500_000_000, -1_500_000_000]
    for k in range(-2, 3):  # every day boundary around 1969-12-31 / 1970-01-01
        v += [k * NS_PER_DAY - 1, k * NS_PER_DAY, k * NS_PER_DAY + 1]
    for y in (1900, 2000, 2023, 2024, 2100):  # first and last day of every month, a time of day on each
        for m in range(1, 13):
            v += [ns_of(y, m, 1) + time_of_day(rng), ns_of(y, m, last_day(y, m)) + time_of_day(rng)]
    # the ends of int64 ns: 1677-09-21T00:12:43.145224192 … 2262-04-11T23:47:16.854775807
    v += [INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, ns_of(1678, 1, 1), ns_of(1678, 1, 1) - 1, ns_of(1678, 2, 28, 23, 59, 59, 999_999_999), ns_of(1678, 12, 31, 12, 30, 30),
          ns_of(1677, 12, 31, 23, 59, 59), ns_of(2262, 1, 1), ns_of(2262, 4, 11, 23, 47, 16, 854_775_807), ns_of(2262, 2, 28, 1, 2, 3), ns_of(2261, 12, 31, 23, 59, 59, 5)]
    v += [int(x) for x in rng.integers(INT64_MIN, INT64_MAX, 130, dtype=np.int64, endpoint=True)]
    v += [int(x) for x in rng.integers(ns_of(1900, 1, 1), ns_of(2100, 12, 31), 130, dtype=np.int64)]
    return v


def month_shift_subset(rng):
    """100 instants between 1900 and 2100 (every shift of ±120 months stays inside int64): the issue's worked cases, the 29th – 31st
    of every month, seeded ones"""
    v = [ns_of(2023, 1, 31), ns_of(2024, 1, 31), ns_of(2023, 3, 31), ns_of(2023, 12, 15, 1, 1, 1), ns_of(2023, 1, 15)]
    for m in range(1, 13):
        for d in range(29, last_day(2024, m) + 1):
            v.append(ns_of(2024, m, d) + time_of_day(rng))
    for m in (1, 2, 3):
        for d in range(29, last_day(2023, m) + 1):
            v.append(ns_of(2023, m, d) + time_of_day(rng))
    v += [ns_of(1900, 3, 1), ns_of(2000, 2, 29, 23, 59, 59, 999_999_999), ns_of(2100, 2, 28), ns_of(1969, 12, 31, 23, 59, 59, 999_999_999), ns_of(1970, 1, 31)]
    v += [int(x) for x in rng.integers(ns_of(1900, 1, 1), ns_of(2100, 12, 31), 100 - len(v), dtype=np.int64)]
    assert len(v) == 100
    return v


def main():
    lib = build_glue()
    i32, i64 = C.c_int32, C.c_int64
    for name, args in (("glue_extract", [i32, i64]), ("glue_trunc", [C.c_char_p, i64, i64]), ("glue_add", [i64, i64]), ("glue_sub", [i64, i64]), ("glue_diff", [i32, i64, i64])):
        getattr(lib, name).restype = i64
        getattr(lib, name).argtypes = args
    rng = np.random.default_rng(20261021)
    ts = instants(rng)
    assert -NS_PER_DAY - 1 in ts and -1 in ts and all(INT64_MIN <= t <= INT64_MAX for t in ts)
    doc = {"parts": list(PARTS), "instants": ts, "extract": {}, "trunc": {}}
    trunc_from = ns_of(1678, 1, 1)  # earlier: the truncated instant does not fit int64
    for k, part in enumerate(PARTS):
        doc["extract"][part] = [int(lib.glue_extract(k, t)) for t in ts]
        doc["trunc"][part] = [int(lib.glue_trunc(part.encode(), len(part), t)) if t >= trunc_from else None for t in ts]
    sub = month_shift_subset(rng)
    doc["months"] = list(MONTHS)
    doc["month_instants"] = sub
    doc["add_months"] = [[int(lib.glue_add(t, m)) for m in MONTHS] for t in sub]
    doc["subtract_months"] = [[int(lib.glue_sub(t, m)) for m in MONTHS] for t in sub]
    pairs = [(e, s) for e, s in zip(ts, ts[1:] + ts[:1]) if INT64_MIN <= e - s <= INT64_MAX]
    pairs += [(0, 1_500_000_000), (1_500_000_000, 0), (0, 90_000_000_000), (90_000_000_000, 0), (0, 0)]  # -1.5 s → -1, -90 s → -1 minute
    doc["diff_pairs"] = [list(p) for p in pairs]
    doc["diff"] = {PARTS[u]: [int(lib.glue_diff(u, e, s)) for e, s in pairs] for u in (2, 3, 4, 5)}
    # the case that tells the reference's month arithmetic from PostgreSQL's: no clamping at the end of the month
    i, j = sub.index(ns_of(2023, 1, 31)), MONTHS.index(1)
    assert doc["add_months"][i][j] == ns_of(2023, 3, 3), doc["add_months"][i][j]
    assert doc["add_months"][sub.index(ns_of(2024, 1, 31))][j] == ns_of(2024, 3, 2)
    assert doc["subtract_months"][sub.index(ns_of(2023, 3, 31))][j] == ns_of(2023, 3, 3)
    assert doc["extract"]["second"][ts.index(-1)] == 59 and doc["extract"]["day"][ts.index(-NS_PER_DAY - 1)] == 30
    path = os.path.join(HERE, "ref_datefn.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("ref_datefn.json: %d instants, %d month-shift instants x %d shifts, %d pairs, %d bytes" % (len(ts), len(sub), len(MONTHS), len(pairs), os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
