"""Pins of the layout choices of ldb_gpu_join_build and ldb_gpu_groupby: for every case of a table of small inputs, each meant to reach one
branch of the host code, the launches per kernel name the profile saw during the one call, the table's slots / bytes (builds), the result's
row count, the device blocks and bytes the result holds, and the blocks left after everything was released — compared with
tests/layout_pins.json.  All figures are integers and must match exactly.  Whether a result is RIGHT is the parity modules' business; this
module says that the host code still takes the same path to it.

The JSON is recorded by this file: LDB_LAYOUT_PINS_RECORD=<path> writes what the cases measure to <path> instead of comparing (and
LDB_LAYOUT_PINS_COMMIT=<id> notes which commit's build produced it).  A refactor records on a build of its parent commit and must then
reproduce the file.  Inputs have at most 100 000 rows: below jit_min_rows, so the generic kernels run.

What the figures cannot tell apart: ordered and hashed slots run the same kernels over a table of the same size, so the group-by cases
"ordered" and "hashed" have equal pins, as have "fused_predicates" / "lazy_predicates" and the builds "ordered" / "int64_key".  The ORDERED
choice itself is pinned by the cases that leave it again: group-by "overflow_retry" (three k_groupby launches: ordered, hashed, larger — two
if the first attempt was hashed already) and the build "ordered_to_hashed" (two k_join_build launches, one if it began hashed); the direct
choice shows in the kernel's profile name (k_groupby_direct) and in the builds' slots / bytes."""
import gc
import json
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "layout_pins.json")
RECORD = os.environ.get("LDB_LAYOUT_PINS_RECORD")
N = 100_000
SEED = 20261019


def _long_run():
    """the run length at which an open-addressing insertion gives up (JOIN_LONG_RUN)"""
    with open(os.path.join(HERE, "..", "lingo-db_amd", "csrc", "ldb_join_kernel.h")) as f:
        return int(re.search(r"#define\s+JOIN_LONG_RUN\s+(\d+)", f.read()).group(1))


CLUSTER = _long_run() + 88  # 600 today: all of them land in one ordered slot, so some insertion walks more than JOIN_LONG_RUN slots


def _rng():
    return np.random.default_rng(SEED)


def _i32(a):
    return pa.array(np.asarray(a, dtype=np.int32), pa.int32())


def _spread(n, hi):
    """n distinct values of [0, hi), both ends among them, shuffled"""
    r = _rng()
    v = r.choice(np.unique(r.integers(1, hi - 1, 2 * n)), n - 2, replace=False)
    v = np.concatenate([[0, hi - 1], v])
    return r.permutation(v)


# ---------------------------------------------------------------- join builds: name → (columns, key columns, unique promise, options)
def _build_inputs():
    r = _rng()
    dup = np.arange(1000)
    dup[999] = 0
    outlier = 1 << 30
    shuffled = r.permutation(1000)
    sh_dup = shuffled.copy()
    sh_dup[999] = sh_dup[0]
    two = {"a": _i32(r.integers(0, 100, 1000)), "b": _i32(r.integers(0, 100, 1000))}
    return {
        "rank_ascending": ({"k": _i32(np.arange(1000))}, [0], True, {}),
        "rank_shuffled": ({"k": _i32(shuffled)}, [0], True, {}),  # k_join_rank_perm: the table holds next[]
        "rank_coarse": ({"k": _i32(np.sort(_spread(100, 1 << 20)))}, [0], True, {}),  # the table holds a coarse filter
        "rank_promise_broken": ({"k": _i32(dup)}, [0], True, {}),  # the rank pass finds a duplicate: direct, chained from the start
        "direct_chained": ({"k": _i32(np.concatenate([[0, 4999], r.integers(0, 5000, 9998)]))}, [0], False, {}),  # 5 000 key values: key bits
        "direct_unique_no_rank": ({"k": _i32(shuffled)}, [0], True, {"join_rank": (0, 1)}),
        "direct_unique_no_rank_dup": ({"k": _i32(sh_dup)}, [0], True, {"join_rank": (0, 1)}),  # flag 1: the retry chains
        "ordered": ({"k": _i32(_spread(2000, 1 << 30))}, [0], False, {}),
        "ordered_to_hashed": ({"k": _i32(np.concatenate([np.arange(CLUSTER), [outlier]]))}, [0], False, {}),
        "hashed_to_chained": ({"k": _i32(np.concatenate([np.full(CLUSTER, 7), [outlier]]))}, [0], False, {}),
        "force_chained": ({"k": _i32(_spread(2000, 1 << 30))}, [0], False, {"join_chained": (1, 0)}),
        "int64_key": ({"k": pa.array(r.permutation(1000).astype(np.int64) * 3, pa.int64())}, [0], False, {}),
        "two_keys_pair32": (two, [0, 1], False, {}),
        "two_keys_no_pair32": (two, [0, 1], False, {"join_pair32": (0, 1)}),
        "empty": ({"k": _i32([])}, [0], False, {}),
    }


# ---------------------------------------------------------------- group-bys: name → (columns, dictionary columns, call, options)
WORDS = [b"word %03d" % i for i in range(40)]


def _sum_count(v=1):
    return [api.agg(capi.AGG_SUM, api.col_expr((0, v))), api.agg(capi.AGG_COUNT_STAR)]


def _in9(col):
    d, keep = api.pred(col, capi.F_IN, values=WORDS[:9])
    d.rhs_kind = capi.RHS_STRING
    return d, keep


def _groupby_inputs():
    r = _rng()
    v = _i32(r.integers(0, 100, N))
    g50k = r.permutation(np.concatenate([np.arange(50000), r.integers(0, 50000, N - 50000)]))  # 50 000 groups, every one present
    wide = _spread(50000, (1 << 31) - 1)[g50k]
    sorted_k = np.arange(N) // 2
    part = r.integers(0, 1 << 21, N)
    part[:2] = [0, (1 << 21) - 1]
    strs = pa.array([WORDS[i] for i in r.integers(0, len(WORDS), N)], pa.binary()).cast(pa.string())
    plain = lambda keys, aggs, est=0, plist=lambda: []: (lambda rel: [rel.groupby(keys, aggs(), plist(), est_groups=est)])  # noqa: E731

    def lazy(keys, aggs, est):
        def run(rel):
            f = rel.scan_filter([api.pred((0, 1), capi.F_LT, 50)])
            return [f.groupby(keys, aggs(), est_groups=est), f]

        return run

    lt50 = lambda: [api.pred((0, 1), capi.F_LT, 50)]  # noqa: E731
    count = lambda: [api.agg(capi.AGG_COUNT_STAR)]  # noqa: E731
    with_any = lambda: _sum_count() + [api.agg(capi.AGG_ANY, api.col_expr((0, 1)))]  # noqa: E731
    partition = {"gb_partition_min_rows": (0, 8 << 20)}
    kv = lambda k: {"k": _i32(k), "v": v}  # noqa: E731
    return {
        "keyless": (kv(g50k), (), plain([], _sum_count), {}),
        "lds_replicas": (kv(g50k % 16), (), plain([(0, 0)], _sum_count, 16), {}),
        "no_estimate": (kv(g50k % 1000), (), plain([(0, 0)], _sum_count, 0), {}),
        "direct": (kv(g50k), (), plain([(0, 0)], _sum_count, 50000), {}),
        "ordered": (kv(wide), (), plain([(0, 0)], _sum_count, 50000), {}),
        "hashed": (kv(wide), (), plain([(0, 0)], _sum_count, 50000), {"gb_ordered": (0, 1)}),
        "two_keys": ({"k": _i32(g50k % 100), "v": v, "k2": _i32(g50k % 50)}, (), plain([(0, 0), (0, 2)], _sum_count, 5000), {}),
        "sorted_dense_keys": (kv(sorted_k), (), plain([(0, 0)], _sum_count, 50000), {}),  # dense_out, dense_keys = 2
        "sorted_with_any": (kv(sorted_k), (), plain([(0, 0)], with_any, 50000), {}),  # dense_keys = 1: representative rows
        "sorted_no_dense_out": (kv(sorted_k), (), plain([(0, 0)], _sum_count, 50000), {"gb_dense_out": (0, 1)}),
        "overflow_retry": (kv(wide), (), plain([(0, 0)], _sum_count, 10000), {}),  # 50 000 groups into 32 768 slots: retried hashed, then larger
        # 2^21 key values: 128 partitions of 2^14 slots (the write-combining partition wants more than 64)
        "partition_count_wc": (kv(part), (), plain([(0, 0)], count, 1 << 20), partition),
        "partition_count_scatter": (kv(part), (), plain([(0, 0)], count, 1 << 20), {**partition, "gb_partition_wc": (0, 1)}),
        "partition_values": (kv(part), (), plain([(0, 0)], _sum_count, 1 << 20), partition),
        "partition_lazy_input": (kv(part), (), lazy([(0, 0)], _sum_count, 1 << 20), {**partition, "lazy_min_rows": (0, 1 << 20)}),  # forced first
        "fused_predicates": (kv(g50k % 100), (), plain([(0, 0)], _sum_count, 100, lt50), {}),
        "lazy_predicates": (kv(g50k % 100), (), lazy([(0, 0)], _sum_count, 100), {"lazy_min_rows": (0, 1 << 20)}),
        "dict_string_min": ({"k": _i32(g50k % 100), "v": v, "s": strs}, (2,), plain([(0, 0)], lambda: [api.str_minmax(capi.AGG_MIN, (0, 2)), api.agg(capi.AGG_COUNT_STAR)], 100), {}),
        "keyless_string_minmax": ({"k": _i32(g50k % 100), "v": v, "s": strs}, (), plain([], lambda: [api.str_minmax(capi.AGG_MIN, (0, 2)), api.str_minmax(capi.AGG_MAX, (0, 2)),
                                                                                                     api.agg(capi.AGG_COUNT_STAR)]), {}),
        "strset_predicate": ({"k": _i32(g50k % 100), "v": v, "s": strs}, (), plain([(0, 0)], _sum_count, 100, lambda: [_in9((0, 2))]), {}),
    }


@pytest.fixture(scope="module")
def inputs():
    return {"build": _build_inputs(), "groupby": _groupby_inputs()}


BUILD_CASES = ["rank_ascending", "rank_shuffled", "rank_coarse", "rank_promise_broken", "direct_chained", "direct_unique_no_rank", "direct_unique_no_rank_dup", "ordered",
               "ordered_to_hashed", "hashed_to_chained", "force_chained", "int64_key", "two_keys_pair32", "two_keys_no_pair32", "empty"]
GROUPBY_CASES = ["keyless", "lds_replicas", "no_estimate", "direct", "ordered", "hashed", "two_keys", "sorted_dense_keys", "sorted_with_any", "sorted_no_dense_out", "overflow_retry",
                 "partition_count_wc", "partition_count_scatter", "partition_values", "partition_lazy_input", "fused_predicates", "lazy_predicates", "dict_string_min",
                 "keyless_string_minmax", "strset_predicate"]


def _live(ctx):
    gc.collect()
    s = ctx.mem_stats()
    return s["live_blocks"], s["live_bytes"]


def _register(ctx, name, cols, dict_cols):
    lib = capi.gpu_lib()
    before = lib.ldb_gpu_get_option(b"dict_encode")  # (-1: never set, the default of 1 holds)
    lib.ldb_gpu_set_option(b"dict_encode", 0)  # only the columns a case names get a dictionary
    try:
        t = ctx.register(name, pa.table(cols))
    finally:
        lib.ldb_gpu_set_option(b"dict_encode", before if before >= 0 else 1)
    for c in dict_cols:
        assert t.dict_encode(c) > 0
    return t


def _measure(ctx, name, cols, dict_cols, options, call, after=None):
    """registers the case's table, runs `call(rel)` → (handles, figures) once under the profile with the case's options set, adds what
    `after(rel, handles)` reads with the defaults back in force, releases everything"""
    lib = capi.gpu_lib()
    base = _live(ctx)
    t = _register(ctx, "pin_" + name, cols, dict_cols)
    rel = t.rel()
    for k, (val, _) in options.items():
        lib.ldb_gpu_set_option(k.encode(), val)
    try:
        before = _live(ctx)
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            handles, got = call(rel)
        finally:
            ctx.prof_enable(False)
        got["launches"] = {k: n for k, (n, _) in sorted(ctx.prof_all().items()) if n}
        held = _live(ctx)
        got["held_blocks"], got["held_bytes"] = held[0] - before[0], held[1] - before[1]
    finally:
        for k, (_, restore) in options.items():
            lib.ldb_gpu_set_option(k.encode(), restore)
    if after:
        got.update(after(rel, handles))
    for h in handles:
        h.release()
    rel.release()
    t.release()
    got["live_blocks_after_release"] = _live(ctx)[0] - base[0]
    return got


def _check(kind, name, got):
    if RECORD:
        pins = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                pins = json.load(f)
        pins["recorded_from_commit"] = os.environ.get("LDB_LAYOUT_PINS_COMMIT", "unknown")
        pins.setdefault(kind, {})[name] = got
        with open(RECORD, "w") as f:
            json.dump(pins, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(PINS) as f:
        want = json.load(f)[kind][name]
    print(f"{kind}/{name}: {json.dumps(got, sort_keys=True)}")
    assert got == want


@pytest.mark.parametrize("name", BUILD_CASES)
def test_join_build_layout(ctx, inputs, name):
    cols, keys, unique, options = inputs["build"][name]
    keys = [(0, k) for k in keys]

    def call(rel):
        ht = rel.join_build(keys, unique=unique)
        return [ht], {"slots": ht.slots, "bytes": ht.table_bytes}

    def self_join(rel, handles):  # the match count of the build side probing its own table: what was built can be probed
        return {"rows": handles[0].probe_count(rel, keys)}

    _check("join_build", name, _measure(ctx, "build_" + name, cols, (), options, call, self_join))


@pytest.mark.parametrize("name", GROUPBY_CASES)
def test_groupby_layout(ctx, inputs, name):
    cols, dict_cols, run, options = inputs["groupby"][name]

    def call(rel):
        handles = run(rel)
        return handles, {"rows": handles[0].rows}

    _check("groupby", name, _measure(ctx, "gb_" + name, cols, dict_cols, options, call))
