"""usage: rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_expand.py run [--tree TREE] [--rows N]
       python tools/measure_expand.py summarise DIR/*/*_kernel_trace.csv --label parent|new --out profiles/expand_sweep.json
The bitmap → row-id expansion alone (csrc/ldb_expand.h), in both kernels that use it, over one int32 column of 256 M uniform values in
[0, 1000):
  scan    — scan_filter(x < cut): k_scan_bitmap → count scan → k_scan_expand, at 1 / 2 / 4 / 8 zones per workgroup (`scan_expand_zones`)
  compact — an inner probe of a unique-key table that holds the keys [0, cut): probe kernel → k_bitmap_compact<2|4|8|16> with `match`
            (`compact_wide_tiles`, `compact_max_words`)
at cut = 1, 10, 50, 125, 250, 500, 750, 900, 990: 0.1 %, 1 %, 5 %, 12.5 %, 25 %, 50 %, 75 %, 90 % and 99 % of the rows, and with the word-per-wave path of nearly
full tiles from 50 % of a tile on and switched off (`expand_direct_pct`).  `run` executes every case three times after two warm-ups,
with a marker kernel (grid = case number) in front of each case; the kernel times come from the trace, which `summarise` cuts at the markers:
the median duration of the k_scan_expand / k_bitmap_compact launch of every case, and that time against the bytes the kernel must move
(bitmap + row ids written + for the probe one 64-byte line of `match` per result and the second id) at 5 TB/s.
`--tree` runs the library of another checkout (a build of the parent commit) with the same script: options that build does not know are refused
by it, so its scan variants are runs of the same kernel.  `summarise` adds its label to an existing --out file."""
import argparse
import csv
import glob
import json
import os
import sys
from collections import defaultdict

CUTS = [1, 10, 50, 125, 250, 500, 750, 900, 990]
# (k_bitmap_compact's label, k_scan_expand's label, options): words per thread / zones per workgroup (4 M bitmap words = 16 384 zones), and the
# share of a tile's rows from which the word-per-wave path takes it (default: 50 %, with `match` 85 %)
VARIANTS = [("words_2", "zones_1", {"compact_wide_tiles": 0, "scan_expand_zones": 1}), ("words_4", "zones_2", {"compact_wide_tiles": 4096, "scan_expand_zones": 2}),
            ("words_8", "zones_4", {"scan_expand_zones": 4}), ("words_16", "zones_8", {"compact_wide_tiles": 1024, "compact_max_words": 16, "scan_expand_zones": 8}),
            ("words_8_direct50", "zones_8_direct50", {"scan_expand_zones": 8, "expand_direct_pct": 50}), ("words_8_staged", "zones_8_staged", {"scan_expand_zones": 8, "expand_direct_pct": 101}),
            ("words_4_direct50", "zones_4_direct50", {"compact_wide_tiles": 4096, "scan_expand_zones": 4, "expand_direct_pct": 50}),
            ("words_8_direct25", "zones_4_direct25", {"scan_expand_zones": 4, "expand_direct_pct": 25}), ("words_8_direct75", "zones_4_direct75", {"scan_expand_zones": 4, "expand_direct_pct": 75})]
RESET = {"compact_wide_tiles": 1, "compact_max_words": 8, "scan_expand_zones": 0, "expand_direct_pct": -1}
FLOOR_BPS = 5e12


def case_id(kind, ci, vi):
    return 1000 + 100 * kind + 10 * ci + vi  # kind 0 = scan, 1 = compact


def run(a):
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(tree, "lingo-db_amd"))
    import numpy as np
    import pyarrow as pa

    import lingodb_amd as ldb
    from lingodb_amd import api, capi

    lib = capi.gpu_lib()
    try:
        ctx = ldb.Context(0)
    except capi.LdbError as e:
        sys.exit("measure_expand: no GPU (%s): nothing measured" % e)
    n = a.rows
    u = np.random.default_rng(1).integers(0, 1000, n, dtype=np.int32)
    t = ctx.register("m_expand", pa.table({"x": pa.array(u)}))
    lib.ldb_gpu_set_option(b"lazy_filter", 0)  # the scan where it is called, not fused into a consumer
    lib.ldb_gpu_set_option(b"jit", 0)  # the ahead-of-time scan and probe kernels: what is measured here runs behind them
    rel = t.rel()
    counts = np.bincount(u, minlength=1000).cumsum()
    for ci, cut in enumerate(CUTS):
        want = int(counts[cut - 1])
        b = ctx.register("m_expand_b%d" % cut, pa.table({"k": pa.array(np.arange(cut, dtype=np.int32))}))
        ht = b.rel().join_build([(0, 0)], unique=True)
        for vi, (name, _, opts) in enumerate(VARIANTS):
            for k, v in opts.items():
                lib.ldb_gpu_set_option(k.encode(), v)  # (an option a build does not know is refused by it: that build runs its default)
            for kind, call in ((0, lambda: rel.scan_filter([api.pred((0, 0), capi.F_LT, cut)])), (1, lambda: ht.probe(rel, [(0, 0)], capi.JOIN_INNER))):
                for rep in range(5):
                    if rep == 2:
                        ctx.sync()
                        ctx.prof_marker(case_id(kind, ci, vi))
                    r = call()
                    assert r.rows == want, (cut, name, kind, r.rows, want)
                    r.release()
            for k, v in RESET.items():
                lib.ldb_gpu_set_option(k.encode(), v)
            print("cut", cut, "variant", name, "rows", want, flush=True)
        ht.release(), b.release()
    ctx.prof_marker(9999)
    ctx.sync()
    t.release()
    ctx.close()


def summarise(a):
    files = [f for p in a.trace for f in glob.glob(p)]
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"].split("(")[0]
                name = name[5:] if name.startswith("void ") else name
                grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) // max(int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1), 1)
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, grid))
    rows.sort()
    seg, cur = defaultdict(lambda: defaultdict(list)), None
    for s, e, name, grid in rows:
        if name == "k_ldb_marker":
            cur = grid
        elif cur is not None and (name.startswith("k_scan_expand") or name.startswith("k_bitmap_compact")):
            seg[cur][name].append((e - s) / 1e6)
    n = a.rows
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res = {"scan": {}, "compact": {}}
    for ci, cut in enumerate(CUTS):
        sel = n * cut / 1000.0  # expected passing rows
        floors = {0: (n / 8 + 4 * sel) / FLOOR_BPS * 1e3, 1: (n / 8 + 8 * sel + 64 * min(sel, n / 16)) / FLOOR_BPS * 1e3}
        for kind, key in ((0, "scan"), (1, "compact")):
            entry = {"floor_ms": round(floors[kind], 4)}
            for vi, labels in enumerate(VARIANTS):
                for kname, ms in seg.get(case_id(kind, ci, vi), {}).items():
                    if kname.startswith("k_scan_expand" if kind == 0 else "k_bitmap_compact"):
                        entry[labels[1 - kind]] = {"kernel": kname, "ms": round(med(ms), 4), "launches": len(ms)}
            res[key]["%.1f%%" % (cut / 10)] = entry
    out = {}
    if os.path.exists(a.out):
        out = json.load(open(a.out))
    out.setdefault("rows", n)
    out.setdefault("method", "rocprofv3 --kernel-trace of tools/measure_expand.py run; median kernel duration of three launches per case after two warm-ups; floor = bitmap + row ids "
                             "(+ one 64-byte match line per result, at most every line of match, + the second id) at 5 TB/s; variants of a build that does not know an option repeat its default")
    out[a.label] = res
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "summarise"])
    ap.add_argument("trace", nargs="*")
    ap.add_argument("--tree", default="")
    ap.add_argument("--rows", type=int, default=256 * 1024 * 1024)
    ap.add_argument("--label", default="new")
    ap.add_argument("--out", default="profiles/expand_sweep.json")
    a = ap.parse_args()
    run(a) if a.mode == "run" else summarise(a)


if __name__ == "__main__":
    main()
