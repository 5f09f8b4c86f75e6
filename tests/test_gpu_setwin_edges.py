"""Set operations and window functions on the device (csrc/ldb_setops.hip) at the edges: every key type, NULL = NULL with bitmaps merged at odd bit
offsets, every group-by layout a set operation can reach (by profiler name where the profile tells them apart), multiplicity runs, inputs that
are row-id relations and outer-join results; the segment tree at the sizes where its shape and the sort underneath change, every argument and
result type, clamped, unbounded and inverted frames, NULL partitions.  Set operations are compared as multisets with setwin_ref.set_op, window
results as exact row order (setwin_ref.window_order) plus exact values and validity (the oracle's ora_window, which tests/test_setwin_edges.py
checks against plain slices for the same cases without a device).  Everything is integer, decimal or bytes: every comparison is ==.
Inputs come from setwin_ref.set_cases() / window_cases(); tables are registered once per module."""
import collections
import ctypes as C
import gc

import numpy as np
import pyarrow as pa
import pytest

import oracle_bind
import setwin_ref as sw
from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

SET = {c["name"]: c for c in sw.set_cases()}
WIN = {c["name"]: c for c in sw.window_cases()}
SET_REFUSALS = {r[0]: r for r in sw.set_refusals()}
WIN_REFUSALS = {r[0]: r for r in sw.window_refusals()}
F_OPS = {"GTE": capi.F_GTE, "LT": capi.F_LT, "EQ": capi.F_EQ, "NEQ": capi.F_NEQ}
assert (capi.SET_UNION_ALL, capi.SET_EXCEPT_ALL, capi.WIN_RANK, capi.WIN_COUNT_STAR, capi.NULLS_LARGEST) == (sw.UNION_ALL, sw.EXCEPT_ALL, sw.RANK, sw.COUNT_STAR, sw.NULLS_LARGEST)


class World:
    """device tables, each made once (keyed by the identity of the pyarrow table and the form of registration)"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.dev = {}
        self.tables = []

    def register(self, table, form="plain", narrow=False):
        """form 'plain': no dictionaries; 'dict': every utf8 column dictionary-encoded"""
        key = (id(table), form, narrow)
        if key not in self.dev:
            lib = capi.gpu_lib()
            lib.ldb_gpu_set_option(b"dict_encode", 0)
            try:
                t = self.ctx.register("sw_%d" % len(self.dev), table, narrow_decimals=narrow)
            finally:
                lib.ldb_gpu_set_option(b"dict_encode", 1)
            for c, f in enumerate(table.schema):
                if pa.types.is_string(f.type):
                    if form == "dict":
                        assert t.dict_encode(c) > 0 and t.dict_size(c) > 0
                    else:
                        assert t.dict_size(c) == -1
            self.dev[key] = t
            self.tables.append(table)  # (keeps id() unique)
        return self.dev[key]

    def rel(self, spec, form="plain", narrow=False):
        """→ (device relation, [(pyarrow table, row ids or None)], rows) of a relation description of setwin_ref"""
        if spec["kind"] == "table":
            return self.register(spec["table"], form, narrow).rel(), [(spec["table"], None)], spec["table"].num_rows
        if spec["kind"] == "filter":
            rel = self.register(spec["table"], form, narrow).rel().scan_filter([api.pred((0, spec["col"]), F_OPS[spec["op"]], spec["value"])])
            sides, n = sw.rel_sides(spec)  # (the row ids are not read back here: a pending lazy filter stays pending for the operator under test)
            return rel, sides, n
        build, probe = self.register(spec["build"], form, narrow), self.register(spec["probe"], form, narrow)
        rel = build.rel().join_build([(0, spec["bkey"])]).probe(probe.rel(), [(0, spec["pkey"])], capi.JOIN_LEFT_OUTER)
        sides, n = sw.sides_from(spec, [rel.rowids(0), rel.rowids(1)])  # the pairs as the device wrote them are the input order
        assert (sides[1][1] == sw.NULL_ROW).any() and collections.Counter(zip(*[r.tolist() for _, r in sides])) == collections.Counter(zip(*[r.tolist() for _, r in sw.rel_sides(spec)[0]]))
        return rel, sides, n

    def close(self):
        for t in self.dev.values():
            t.release()


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.close()


def live(ctx):
    gc.collect()
    return ctx.mem_stats()["live_blocks"]


def refused(ctx, call, status):
    """`call` must fail with `status` and leave as many live device blocks as it found"""
    before = live(ctx)
    with pytest.raises(capi.LdbError) as e:
        call()
    assert e.value.status == status, e.value
    del e
    assert live(ctx) == before


def jit_launches():
    n, h, ms = C.c_int64(), C.c_int64(), C.c_double()
    capi.gpu_lib().ldb_gpu_jit_stats(C.byref(n), C.byref(h), C.byref(ms))
    return n.value + h.value


class Specialised:
    """jit_min_rows = 0 and lazy_min_rows = 0 inside the block: every launch specialised at run time, every base-table filter pending until its
    consumer; at least one specialised kernel must have been launched"""

    def __enter__(self):
        self.before = jit_launches()
        capi.gpu_lib().ldb_gpu_set_option(b"jit_min_rows", 0)
        capi.gpu_lib().ldb_gpu_set_option(b"lazy_min_rows", 0)

    def __exit__(self, exc_type, exc, tb):
        capi.gpu_lib().ldb_gpu_set_option(b"jit_min_rows", 4000000)
        capi.gpu_lib().ldb_gpu_set_option(b"lazy_min_rows", 1 << 20)
        if exc_type is None:
            assert jit_launches() > self.before, "ran without a single specialised kernel launch"


def column_values(col):
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if pa.types.is_dictionary(arr.type):
        arr = arr.dictionary_decode()
    return sw.column_values(arr), arr.type


# ---------------------------------------------------------------- set operations
def run_set_case(world, ctx, case, ops=None):
    forms = {side: "dict" if case["dict"] == side else "plain" for side in ("left", "right")}
    left, lsides, _ = world.rel(case["left"], forms["left"], case["narrow"])
    right, rsides, _ = world.rel(case["right"], forms["right"], case["narrow"])
    if case["left"]["kind"] == "filter":
        assert np.array_equal(left.rowids(0), lsides[0][1])
    lrows, rrows = sw.rel_rows(lsides, case["lcols"]), sw.rel_rows(rsides, case["rcols"])
    fields = [lsides[s][0].schema.field(c) for s, c in case["lcols"]]
    for op in ops if ops is not None else case["ops"]:
        if case["path"]:
            ctx.prof_reset()
            ctx.prof_enable(True)
        try:
            res = left.set_op(right, op, case["lcols"], case["rcols"])
        finally:
            if case["path"]:
                ctx.prof_enable(False)
        if case["path"] and op != capi.SET_UNION_ALL:
            assert ctx.prof_all().get(case["path"], (0, 0.0))[0] >= 1, (op, case["path"], sorted(ctx.prof_all()))
        got = res.to_arrow()
        cols = [column_values(c) for c in got.columns]
        assert got.column_names == [f.name for f in fields] and [t for _, t in cols] == [f.type for f in fields], op  # the left side's names and types
        assert res.rows == got.num_rows
        rows = collections.Counter(zip(*[v for v, _ in cols])) if got.num_rows else collections.Counter()
        assert rows == sw.set_op(lrows, rrows, op), op
        res.release()
    left.release(), right.release()


@pytest.mark.parametrize("name", list(SET))
def test_set_operations_match_the_plain_counters(world, ctx, name):
    run_set_case(world, ctx, SET[name])


@pytest.mark.parametrize("name", [n for n, c in SET.items() if c["spec"]])
def test_set_operations_on_specialised_kernels(world, ctx, name):
    """one case per group-by layout, every launch specialised"""
    with Specialised():
        run_set_case(world, ctx, SET[name])


@pytest.mark.parametrize("name", list(SET_REFUSALS))
def test_set_operations_refused(world, ctx, name):
    _, lt, lcols, rt, rcols, op, code = SET_REFUSALS[name]
    left, right = world.register(lt).rel(), world.register(rt).rel()
    refused(ctx, lambda: left.set_op(right, op, [(0, c) for c in lcols], [(0, c) for c in rcols]), getattr(capi, code))


# ---------------------------------------------------------------- window functions
def order_specs(order):
    return [api.sort_spec((s, c), bool(d), nl) for s, c, d, nl in order]


def run_window_case(world, ctx, oracle, case):
    rel, sides, n = world.rel(case["rel"], "plain", case["narrow"])
    own = case["rel"]["kind"] != "louter"  # (the pair order of a join is the device's: the layout is computed from the row ids it wrote)
    order, start, end, args = sw.window_layout(case) if own else sw.window_layout(case, sides, n)
    for frame in case["frames"]:
        out_rel, out_cols = rel.window(case["part"], order_specs(case["order"]), case["fns"], frame=frame)
        assert out_rel.rows == out_cols.rows == n
        for s, (_, ids) in enumerate(sides):  # exact row order
            assert np.array_equal(out_rel.rowids(s), order if ids is None else ids[order]), (frame, s)
        got = out_cols.to_arrow()
        for k, (fn, col) in enumerate(case["fns"]):
            vals = args[col] if col is not None else None
            want = oracle_bind.window(oracle, None if vals is None else [v or 0 for v in vals], None if vals is None else [v is not None for v in vals], start, end, fn, frame[0], frame[1])
            ty = sw.arg_type(case, col) if col is not None else None
            if fn == sw.SUM:  # the oracle accumulates in 128 bits; the result column of an int32 / int64 argument keeps the low 64
                want = [None if v is None else sw.wrap(v, sw.sum_bits_of(ty)) for v in want]
            have, have_type = column_values(got.column(k))
            assert have == want, (frame, fn, col)
            assert have_type == sw.result_type(fn, ty), (fn, col)
            if None not in want:  # a result column without NULLs carries no validity
                assert not out_cols.col_ptrs(k)[2] and got.column(k).null_count == 0, (frame, fn, col)
            else:
                assert got.column(k).null_count == want.count(None)
        out_rel.release(), out_cols.release()
    rel.release()


@pytest.mark.parametrize("name", list(WIN))
def test_window_functions_match_the_oracle(world, ctx, oracle, name):
    run_window_case(world, ctx, oracle, WIN[name])


@pytest.mark.parametrize("name", [n for n, c in WIN.items() if c["spec"]])
def test_window_over_a_pending_filter_on_specialised_kernels(world, ctx, oracle, name):
    """lazy_min_rows = 0: the filter is still pending when ldb_gpu_window gets the relation"""
    with Specialised():
        run_window_case(world, ctx, oracle, WIN[name])


def test_inverted_frames_are_empty(world, ctx, oracle):
    """from > to: SUM / MIN / MAX NULL, COUNT 0, COUNT(*) 0 wherever clamping does not bring the two ends together (the reference throws)"""
    case = WIN["inverted_frames"]
    rel, sides, n = world.rel(case["rel"])
    _, start, end, _ = sw.window_layout(case)
    for frame in ((2 ** 40, -(2 ** 40)), (1, 0)):
        _, cols = rel.window(case["part"], order_specs(case["order"]), case["fns"], frame=frame)
        got = {fn: cols.to_arrow().column(k).to_pylist() for k, (fn, _) in enumerate(case["fns"])}
        inside = [i for i in range(n) if frame[0] > 1 or i < end[i] - 1]  # (1, 0) on the last row of a partition clamps to that row
        assert len(inside) >= n - 3
        for i in inside:
            assert (got[sw.SUM][i], got[sw.MIN][i], got[sw.MAX][i], got[sw.COUNT][i], got[sw.COUNT_STAR][i]) == (None, None, None, 0, 0), (frame, i)


def test_window_columns_feed_a_filter_and_a_group_by(world, ctx):
    """rel.zip(cols), a scan_filter on a window column and a group-by that sums another, as the plan interpreter's window step chains them"""
    case = WIN["eight_functions"]
    table = case["rel"]["table"]
    order, start, end, args = sw.window_layout(case)
    rel = world.register(table).rel()
    fns = [(sw.RANK, None), (sw.SUM, (0, 2)), (sw.COUNT, (0, 2))]
    out_rel, cols = rel.window(case["part"], order_specs(case["order"]), fns, frame=(sw.P, 0))
    zipped = out_rel.zip(cols)
    side = zipped.sides - 1
    kept = zipped.scan_filter([api.pred((side, 0), capi.F_LTE, 40)])  # rank <= 40
    res = kept.groupby([(0, 0)], [api.agg(capi.AGG_SUM, api.col_expr((side, 2))), api.agg(capi.AGG_MAX, api.col_expr((side, 1))), api.agg(capi.AGG_COUNT_STAR)], est_groups=8).to_arrow()
    ref = sw.window_all(args[(0, 2)], None, start, end, [sw.RANK, sw.SUM, sw.COUNT], sw.P, 0, 64)
    p = sw.column_values(table.column(0))
    want = {}
    for i, r in enumerate(order):
        if ref[sw.RANK][i] <= 40:
            w = want.setdefault(p[int(r)], [0, None, 0])
            w[0] += ref[sw.COUNT][i]
            s = ref[sw.SUM][i]
            w[1] = w[1] if s is None else (s if w[1] is None else max(w[1], s))
            w[2] += 1
    assert {k: [a, b, c] for k, a, b, c in zip(*[c.to_pylist() for c in res.columns])} == want and len(want) == 3


@pytest.mark.parametrize("name", list(WIN_REFUSALS))
def test_window_functions_refused(world, ctx, name):
    _, table, part, order, fns, code = WIN_REFUSALS[name]
    rel = world.register(table).rel()
    refused(ctx, lambda: rel.window(part, order_specs(order), fns), getattr(capi, code))
