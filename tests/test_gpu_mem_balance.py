"""Device-memory balance of the operators (ldb_gpu_mem_stats): a call whose outputs have been released leaves as many live blocks and bytes
behind as it found, on error returns too.  Inputs are tiny: 5 000 probe rows (more than two 2 048-row join tiles, not a multiple of the
64-row chunk) against 700 build rows, once with unique int32 keys (the unique-key probe) and once with duplicated int64 keys (the pairs probe)."""
import ctypes as C
import gc

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

N_PROBE, N_BUILD = 5000, 700
WORDS = ["alpha", "beta", "gamma", "a considerably longer string value", ""]
ALL_KINDS = [capi.JOIN_INNER, capi.JOIN_SEMI, capi.JOIN_ANTI, capi.JOIN_LEFT_OUTER, capi.JOIN_MARK, capi.JOIN_SINGLE, capi.JOIN_SEMI_BUILD, capi.JOIN_ANTI_BUILD,
             capi.JOIN_RIGHT_OUTER, capi.JOIN_FULL_OUTER]
KIND_NAMES = ["inner", "semi", "anti", "left_outer", "mark", "single", "semi_build", "anti_build", "right_outer", "full_outer"]


@pytest.fixture(scope="module")
def data(ctx):
    rng = np.random.default_rng(20261018)
    uniq = rng.permutation(1000)[:N_BUILD]  # 700 distinct keys out of [0, 1000): some probe keys find no partner
    probe = pa.table({
        "k32": pa.array(rng.integers(0, 1000, N_PROBE), pa.int32()),
        "k64": pa.array(rng.integers(0, 260, N_PROBE), pa.int64()),
        "v": pa.array(rng.integers(0, 100, N_PROBE), pa.int32()),
        "s": pa.array([WORDS[i] for i in rng.integers(0, len(WORDS), N_PROBE)]),
    })
    build_u = pa.table({"k": pa.array(uniq, pa.int32()), "v": pa.array(rng.integers(0, 100, N_BUILD), pa.int32())})
    build_d = pa.table({"k": pa.array(rng.integers(0, 240, N_BUILD), pa.int64()), "v": pa.array(rng.integers(0, 100, N_BUILD), pa.int32())})
    tabs = {"probe": ctx.register("mb_probe", probe), "unique": ctx.register("mb_build_u", build_u), "dup": ctx.register("mb_build_d", build_d)}
    yield tabs
    for t in tabs.values():
        t.release()


def _live(ctx):
    gc.collect()  # (handles other tests dropped without release() go now, not in the middle of a measurement)
    s = ctx.mem_stats()
    return s["live_blocks"], s["live_bytes"]


def _release(*handles):
    for h in handles:
        if isinstance(h, (tuple, list)):
            _release(*h)
        elif h is not None:
            h.release()


def _probe_case(data, build, kind, **kw):
    """one build + probe; every handle it made is released before it returns"""
    p, b = data["probe"].rel(), data[build].rel()
    ht = b.join_build([(0, 0)], unique=(build == "unique"))
    out = ht.probe(p, [(0, 0 if build == "unique" else 1)], kind, **kw)
    _release(out, ht, b, p)


def _assert_balanced(ctx, run):
    run()  # warms the per-table caches (value ranges, indexes, dictionaries)
    run()
    want = _live(ctx)
    run()
    assert _live(ctx) == want


# ---------------------------------------------------------------- error returns
def _mark_without_mark_out(ctx, data, via_nl):
    p, b = data["probe"].rel(), data["unique"].rel()
    ht = None if via_nl else b.join_build([(0, 0)], unique=True)
    before = _live(ctx)
    r = C.c_void_p()
    if via_nl:
        ra = (capi.JoinResidual * 1)()
        ra[0].probe_col, ra[0].op, ra[0].build_col = api.colref(0, 2), capi.F_LT, api.colref(0, 1)
        st = ctx.lib.ldb_gpu_join_nl(ctx.h, p.h, b.h, capi.JOIN_MARK, ra, 1, C.byref(r), None)
    else:
        keys, n = api._refs([(0, 0)])
        st = ctx.lib.ldb_gpu_join_probe(ctx.h, ht.h, p.h, keys, n, capi.JOIN_MARK, C.byref(r), None)
    after = _live(ctx)
    _release(ht, b, p)
    assert st == capi.LDB_ERR_INVALID
    assert not r.value
    assert after == before


def test_mark_without_mark_out_frees_its_bitmap(ctx, data):
    """ldb_gpu_join_probe(kind = MARK, mark_out = NULL) fails after the probe bitmap was allocated"""
    _mark_without_mark_out(ctx, data, via_nl=False)


def test_nl_mark_without_mark_out_frees_everything(ctx, data):
    """the same error reached through ldb_gpu_join_nl, whose key tables, zipped relations and hash table are alive at that point"""
    _mark_without_mark_out(ctx, data, via_nl=True)


# ---------------------------------------------------------------- balance per operator
@pytest.mark.parametrize("build", ["unique", "dup"])
@pytest.mark.parametrize("kind", ALL_KINDS, ids=KIND_NAMES)
def test_join_kinds_balance(ctx, data, build, kind):
    _assert_balanced(ctx, lambda: _probe_case(data, build, kind))


@pytest.mark.parametrize("build", ["unique", "dup"])
def test_probe_with_residual_balance(ctx, data, build):
    _assert_balanced(ctx, lambda: _probe_case(data, build, capi.JOIN_INNER, residual=[((0, 2), capi.F_LT, (0, 1))]))


def test_join_nl_balance(ctx, data):
    def run():
        p, b = data["probe"].rel(), data["dup"].rel()
        few = b.scan_filter([api.pred((0, 1), capi.F_LT, 5)])  # a small build side: the join is |probe| x |build|
        out = p.join_nl(few, residual=[((0, 2), capi.F_LT, (0, 1))])
        _release(out, few, b, p)

    _assert_balanced(ctx, run)


@pytest.mark.parametrize("build", ["unique", "dup"])
def test_probe_semi_anti_build_balance(ctx, data, build):
    def run():
        p, b = data["probe"].rel(), data[build].rel()
        ht = b.join_build([(0, 0)], unique=(build == "unique"))
        out = ht.probe_semi_anti_build(p, [(0, 0 if build == "unique" else 1)], [api.pred((0, 2), capi.F_GT, 50)])
        _release(out, ht, b, p)

    _assert_balanced(ctx, run)


@pytest.mark.parametrize("kind", [capi.JOIN_INNER, capi.JOIN_SEMI, capi.JOIN_LEFT_OUTER], ids=["inner", "semi", "left_outer"])
def test_lazily_filtered_probe_side_balance(ctx, data, kind):
    lib = capi.gpu_lib()

    def run():
        p, b = data["probe"].rel(), data["unique"].rel()
        lazy = p.scan_filter([api.pred((0, 2), capi.F_LT, 60)])
        ht = b.join_build([(0, 0)], unique=True)
        out = ht.probe(lazy, [(0, 0)], kind)
        _release(out, ht, lazy, b, p)

    lib.ldb_gpu_set_option(b"lazy_min_rows", 0)  # filters over dense relations of any size stay lazy
    try:
        _assert_balanced(ctx, run)
    finally:
        lib.ldb_gpu_set_option(b"lazy_min_rows", 1 << 20)


@pytest.mark.parametrize("kind", [capi.JOIN_INNER, capi.JOIN_LEFT_OUTER, capi.JOIN_SEMI_BUILD], ids=["inner", "left_outer", "semi_build"])
def test_radix_clustered_probe_balance(ctx, data, kind):
    lib = capi.gpu_lib()
    lib.ldb_gpu_set_option(b"join_radix", 1)  # cluster the probe side whenever the table layout allows it
    try:
        _assert_balanced(ctx, lambda: _probe_case(data, "unique", kind))
    finally:
        lib.ldb_gpu_set_option(b"join_radix", -1)


@pytest.mark.parametrize("keys", [[(0, 1)], [(0, 3)], []], ids=["int_key", "string_key", "keyless"])
def test_groupby_balance(ctx, data, keys):
    def run():
        p = data["probe"].rel()
        t = p.groupby(keys, [api.agg(capi.AGG_SUM, api.col_expr((0, 2))), api.agg(capi.AGG_COUNT_STAR)], [api.pred((0, 2), capi.F_LT, 90)])
        _release(t, p)

    _assert_balanced(ctx, run)


def test_sort_and_topk_balance(ctx, data):
    def run():
        p = data["probe"].rel()
        specs = [api.sort_spec((0, 2), descending=True), api.sort_spec((0, 0))]
        _release(p.sort(specs), p.topk(specs, 10), p)

    _assert_balanced(ctx, run)


def test_set_op_balance(ctx, data):
    def run():
        a, b = data["unique"].rel(), data["probe"].rel()
        t = a.set_op(b, capi.SET_INTERSECT, cols=[(0, 0)], other_cols=[(0, 0)])
        _release(t, b, a)

    _assert_balanced(ctx, run)


def test_materialize_with_string_column_balance(ctx, data):
    def run():
        p = data["probe"].rel()
        f = p.scan_filter([api.pred((0, 2), capi.F_GTE, 30)])
        t = f.materialize([(0, 3), (0, 0)])
        _release(t, f, p)

    _assert_balanced(ctx, run)
