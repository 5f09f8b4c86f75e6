"""Selection bitmap → ascending row ids (csrc/ldb_expand.h: d_expand_tile, used by k_scan_expand and k_bitmap_compact<2|4|8>): scans, inner /
semi / anti probes of a unique-key table and the build-side semi join against numpy, bit for bit, at row counts around every tile and word
boundary, at densities on both sides of the former sparse / dense switch (1 bit in 8) and of today's (50 % of a tile's rows, 85 % with `match`: the
all-set inputs and the full third are above it, the halves next to it), with either path forced on every tile, on inputs whose tiles differ, with a tile that holds
exactly one staging chunk (4 096 row ids) and one more / less, and as a prepared plan that replays its counts.

`compact_wide_tiles = 2` and `scan_expand_tiles = 2` put the tile floors at 2, so four and eight words per thread (four zones per workgroup) are
reached from 131 072 and 262 144 rows on, `scan_expand_zones` sets two and eight zones; the library's defaults (two words / one zone at these
sizes) run beside them."""
import json

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

CHUNK = 4096  # EXPAND_CHUNK of csrc/ldb_expand.h
ROWS = [1, 63, 64, 65, 16_383, 16_384, 16_385, 131_073, 262_145, 1_000_003]
N_BUILD = 1000  # build keys 0 … 999 in shuffled order; probe keys >= 5000 have no partner
DEFAULTS = {b"compact_wide_tiles": 1, b"scan_expand_tiles": 2048, b"scan_expand_zones": 0, b"scan_split": 1, b"lazy_filter": 1, b"expand_direct_pct": -1}


def bitmaps(n):
    """name → bool[n]: the densities of the issue, the structured thirds, and tiles that hold a staging chunk exactly"""
    rng = np.random.default_rng(n)
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    out = {"last_row_only": last, "all_set": np.ones(n, dtype=bool), "1_in_1000": rng.random(n) < 0.001, "below_1_in_8": rng.random(n) < 0.12,
           "above_1_in_8": rng.random(n) < 0.13, "half": rng.random(n) < 0.5}
    thirds = np.zeros(n, dtype=bool)
    thirds[n // 3: 2 * (n // 3)] = True
    thirds[2 * (n // 3):] = rng.random(n - 2 * (n // 3)) < 0.03
    out["thirds"] = thirds
    return out


def chunk_bitmaps():
    """65 541 rows: exactly CHUNK − 1 / CHUNK / CHUNK + 1 bits in the first 16 384 rows (the first scan zone, and — the next 16 384 rows being
    empty — the first two-word compaction tile), 3 % behind them"""
    n = 65_541
    rng = np.random.default_rng(7)
    out = {}
    for k in (CHUNK - 1, CHUNK, CHUNK + 1):
        b = np.zeros(n, dtype=bool)
        b[rng.choice(16_384, k, replace=False)] = True
        b[32_768:] = rng.random(n - 32_768) < 0.03
        out["chunk_%d" % k] = b
    return out


def set_options(lib, opts):
    for k, v in opts.items():
        assert lib.ldb_gpu_set_option(k, v) == capi.LDB_OK, k


@pytest.fixture(scope="module")
def build(ctx):
    bk = np.random.default_rng(3).permutation(N_BUILD).astype(np.int32)
    b = ctx.register("expand_b", pa.table({"k": pa.array(bk)}))
    ht = b.rel().join_build([(0, 0)], unique=True)
    yield bk, ht
    ht.release(), b.release()


def check_scan(ctx, lib, name, bits):
    n = len(bits)
    want = np.nonzero(bits)[0]
    t = ctx.register("expand_s", pa.table({"x": pa.array(bits.astype(np.int32))}))
    try:
        # the defaults; the whole-zone form (no gridDim.y); 2 and 4 zones per workgroup from 4 / 8 zones on; two and eight zones per workgroup; every
        # tile staged through LDS (101) and every tile a word per wave iteration (0), whatever it holds
        for opts in ({}, {b"scan_split": 0}, {b"scan_expand_tiles": 2}, {b"scan_expand_tiles": 2, b"scan_split": 0}, {b"scan_expand_zones": 2}, {b"scan_expand_zones": 8},
                     {b"scan_expand_tiles": 2, b"expand_direct_pct": 101}, {b"scan_expand_tiles": 2, b"expand_direct_pct": 0}):
            set_options(lib, {**opts, b"lazy_filter": 0})  # the scan kernel itself, not a consumer's fused filter
            try:
                got = t.rel().scan_filter([api.pred((0, 0), capi.F_GTE, 1)]).rowids(0)
            finally:
                set_options(lib, DEFAULTS)
            assert np.array_equal(got, want), (name, n, opts)
    finally:
        t.release()


def check_probes(ctx, lib, build, name, bits):
    bk, ht = build
    n = len(bits)
    i = np.arange(n, dtype=np.int64)
    pk = np.where(bits, (i * 7) % N_BUILD, 5000 + i % 100).astype(np.int32)
    want, want_anti = np.nonzero(bits)[0], np.nonzero(~bits)[0]
    p = ctx.register("expand_p", pa.table({"k": pa.array(pk)}))
    try:
        # two words per thread at these sizes; 4 / 8 from 131 072 / 262 144 rows on; every tile staged (101) / a word per wave iteration (0)
        for opts in ({}, {b"compact_wide_tiles": 2}, {b"compact_wide_tiles": 2, b"expand_direct_pct": 101}, {b"compact_wide_tiles": 2, b"expand_direct_pct": 0}):
            set_options(lib, opts)
            try:
                out = ht.probe(p.rel(), [(0, 0)], capi.JOIN_INNER)
                rp, rb = out.rowids(0), out.rowids(1)
                semi = ht.probe(p.rel(), [(0, 0)], capi.JOIN_SEMI).rowids(0)
                anti = ht.probe(p.rel(), [(0, 0)], capi.JOIN_ANTI).rowids(0)
            finally:
                set_options(lib, DEFAULTS)
            assert np.array_equal(rp, want), (name, n, opts, "inner")
            assert np.array_equal(bk[rb], pk[rp]), (name, n, opts, "inner: build side")
            assert np.array_equal(semi, want), (name, n, opts, "semi")
            assert np.array_equal(anti, want_anti), (name, n, opts, "anti")
    finally:
        p.release()


@pytest.mark.parametrize("n", ROWS)
def test_scan_row_ids_equal_numpy(ctx, n):
    lib = capi.gpu_lib()
    for name, bits in bitmaps(n).items():
        check_scan(ctx, lib, name, bits)


@pytest.mark.parametrize("n", ROWS)
def test_unique_probe_row_ids_equal_numpy(ctx, build, n):
    lib = capi.gpu_lib()
    for name, bits in bitmaps(n).items():
        check_probes(ctx, lib, build, name, bits)


def test_a_tile_that_fills_the_staging_chunk_exactly(ctx, build):
    lib = capi.gpu_lib()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for name, bits in chunk_bitmaps().items():
            assert int(bits[:32_768].sum()) == int(name.split("_")[1])
            check_scan(ctx, lib, name, bits)
            check_probes(ctx, lib, build, name, bits)
        assert ctx.prof_all().get("k_bitmap_compact", (0, 0.0))[0] >= 3 * 4 * 3, "the probes did not go through the compaction kernel"
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("n", [16_385, 262_145])
def test_build_side_semi_join_row_ids_equal_numpy(ctx, n):
    """JOIN_SEMI_BUILD: the bitmap is over the BUILD rows (keys 0 … n − 1 in order); the probe side holds the keys of the set rows, twice each"""
    lib = capi.gpu_lib()
    b = ctx.register("expand_sb_b", pa.table({"k": pa.array(np.arange(n, dtype=np.int32))}))
    ht = b.rel().join_build([(0, 0)], unique=True)
    try:
        for name, bits in bitmaps(n).items():
            want = np.nonzero(bits)[0]
            keys = np.concatenate([want, want[::-1], np.arange(n, n + 50)]).astype(np.int32)
            p = ctx.register("expand_sb_p", pa.table({"k": pa.array(keys)}))
            try:
                for opts in ({}, {b"compact_wide_tiles": 2}):
                    set_options(lib, opts)
                    try:
                        got = ht.probe(p.rel(), [(0, 0)], capi.JOIN_SEMI_BUILD).rowids(0)
                    finally:
                        set_options(lib, DEFAULTS)
                    assert np.array_equal(got, want), (name, n, opts)
            finally:
                p.release()
    finally:
        ht.release(), b.release()


def test_prepared_plan_replays_the_same_rows(ctx):
    """a filter and a partially matching inner join as a prepared plan: executions two and three size their outputs from replayed counts (`cap`)"""
    rng = np.random.default_rng(12)
    n = 300_007
    x = (rng.random(n) < 0.3).astype(np.int32)
    i = np.arange(n, dtype=np.int64)
    pk = np.where(rng.random(n) < 0.4, (i * 7) % N_BUILD, 5000 + i % 100).astype(np.int32)
    bk = rng.permutation(N_BUILD).astype(np.int32)
    t = ctx.register("expand_rt", pa.table({"x": pa.array(x), "pk": pa.array(pk), "i": pa.array(i)}))
    b = ctx.register("expand_rb", pa.table({"bk": pa.array(bk)}))
    plan = {"steps": [{"op": "filter", "in": "t", "preds": [{"col": "x", "op": "GTE", "value": 1}], "out": "f"},
                      {"op": "join_build", "in": "b", "keys": ["bk"], "unique": True, "index": False, "out": "h"},
                      {"op": "join_probe", "ht": "h", "in": "f", "keys": ["pk"], "kind": "inner", "out": "j"},
                      {"op": "materialize", "in": "j", "cols": ["i", "bk"], "out": "result"}], "result": "result"}
    want = np.nonzero((x == 1) & (pk < N_BUILD))[0]
    assert 0 < len(want) < n
    prepared = ctx.prepare_plan(json.dumps(plan))
    try:
        for _ in range(3):
            got = prepared.execute({"t": t, "b": b}).to_arrow()
            assert np.array_equal(got.column(0).to_numpy(), want)
            assert np.array_equal(got.column(1).to_numpy(), pk[want])
        assert prepared.stats()["replays"] >= 1
    finally:
        prepared.release()
        t.release(), b.release()
