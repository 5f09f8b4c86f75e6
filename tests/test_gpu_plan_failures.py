"""A plan that fails leaves nothing behind: every handle a step had made when the failure came is released — the step's own fresh
relation / table / hash table (a repeated `out` is only noticed after the device work), intermediates of a filter or join applied
in chunks, the result table when a later step fails, a loop iteration's values.  Measured with ldb_gpu_mem_stats: the valid variant
of each plan runs first (it warms per-table statistics and the parked pool), then the failing variant must leave as many live
blocks and bytes as it found and no descriptor held.

Inputs are tiny — 64 and 16 rows: what can go wrong here is host bookkeeping, not a kernel, and one workgroup's worth of rows
reaches every operator.  Hash tables are built over filtered relations (a bare base table's unique build is the table's
persistent index, which stays alive by design)."""
import decimal
import gc
import json
import os

import pyarrow as pa
import pytest

from lingodb_amd import capi

pytestmark = pytest.mark.gpu

X = list(range(64))
I = [(7 * x) % 5 for x in X]
WORDS = ["", "a", "green", "Ünïcödé"]
K = X[::4]  # 16 keys, every one also in t.x


@pytest.fixture(scope="module")
def tabs(ctx):
    t = ctx.register("pf_t", pa.table({"x": pa.array(X, pa.int32()), "i": pa.array(I, pa.int32()),
                                       "d": pa.array([decimal.Decimal(x) * decimal.Decimal("1.25") for x in X], pa.decimal128(12, 2)),
                                       "s": pa.array([WORDS[x % 4] for x in X])}))
    u = ctx.register("pf_u", pa.table({"k": pa.array(K, pa.int32())}))
    yield {"t": t, "u": u}
    t.release()
    u.release()


def _live(ctx):
    gc.collect()  # (handles other tests dropped without release() go now, not in the middle of a measurement)
    s = ctx.mem_stats()
    return s["live_blocks"], s["live_bytes"]


def _fails_clean(ctx, tables, good, bad, needle):
    """the valid plan once (result released), then the failing one: same live blocks and bytes afterwards, no descriptor held"""
    ctx.run_plan(json.dumps(good), tables).release()
    want = _live(ctx)
    with pytest.raises(capi.LdbError) as e:
        ctx.run_plan(json.dumps(bad), tables)
    assert needle in str(e.value), str(e.value)
    assert _live(ctx) == want
    assert ctx.desc_cache_stats()["held"] == 0
    return str(e.value)


# ---------------------------------------------------------------- a step whose `out` repeats an earlier name
PREFIX = [{"op": "filter", "in": "t", "preds": [{"col": "x", "op": "GTE", "value": 0}], "out": "f"},
          {"op": "filter", "in": "u", "preds": [{"col": "k", "op": "GTE", "value": 0}], "out": "uf"},
          {"op": "join_build", "in": "uf", "keys": ["k"], "out": "h"}]
NINE = [{"col": "x", "op": "GTE", "value": 3}, {"col": "x", "op": "LT", "value": 60}, {"col": "x", "op": "NEQ", "value": 10}, {"col": "x", "op": "NEQ", "value": 11},
        {"col": "i", "op": "LTE", "value": 3}, {"col": "i", "op": "GTE", "value": 0}, {"col": "x", "op": "NEQ", "value": 20}, {"col": "x", "op": "GT", "value": 1},
        {"col": "x", "op": "NEQ", "value": 33}]
THREE = [{"probe": "x", "op": "LTE", "build": "k"}, {"probe": "x", "op": "GTE", "build": "k"}, {"probe": "i", "op": "NEQ", "build": "k"}]


def _mat(cols):
    return [{"op": "materialize", "in": "z", "cols": cols, "out": "result"}]


# name → (the last step, without its `out`; the steps that turn its value "z" into the result of the valid variant)
DUPLICATE_OUT = {
    "filter": ({"op": "filter", "in": "f", "preds": [{"col": "x", "op": "LT", "value": 40}]}, _mat(["x"])),
    "filter_nine_conjuncts": ({"op": "filter", "in": "f", "preds": NINE}, _mat(["x"])),
    "filter_dnf": ({"op": "filter_dnf", "in": "f", "clauses": [[{"col": "x", "op": "LT", "value": 5}], [{"col": "x", "op": "GT", "value": 60}]]}, _mat(["x"])),
    "materialize": ({"op": "materialize", "in": "f", "cols": ["x", {"col": "d", "as": "dd"}]}, _mat(["dd"])),
    "groupby": ({"op": "groupby", "in": "f", "keys": ["i"], "aggs": [{"fn": "count_star", "as": "n"}], "est_groups": 8}, _mat(["i", "n"])),
    "join_build": ({"op": "join_build", "in": "uf", "keys": ["k"]},
                   [{"op": "join_probe", "ht": "z", "in": "f", "keys": ["x"], "kind": "semi", "out": "j"}, {"op": "materialize", "in": "j", "cols": ["x"], "out": "result"}]),
    "join_probe_inner": ({"op": "join_probe", "ht": "h", "in": "f", "keys": ["x"], "kind": "inner"}, _mat(["x", "k"])),
    "join_probe_inner_three_residuals": ({"op": "join_probe", "ht": "h", "in": "f", "keys": ["x"], "kind": "inner", "residual": THREE}, _mat(["x", "k"])),
    "join_probe_mark_out": ({"op": "join_probe", "ht": "h", "in": "f", "keys": ["x"], "kind": "mark", "mark_out": "zm"}, _mat(["x"])),
    "join_probe_mark_as": ({"op": "join_probe", "ht": "h", "in": "f", "keys": ["x"], "kind": "mark", "mark_as": "m"}, _mat(["x", "m"])),
    "join_nl": ({"op": "join_nl", "in": "f", "build": "uf", "kind": "inner", "residual": [{"probe": "x", "op": "EQ", "build": "k"}]}, _mat(["x", "k"])),
    "map_expr": ({"op": "map", "in": "f", "as": "y", "expr": {"add": [1, "x"]}}, _mat(["x", "y"])),
    "map_length": ({"op": "map", "in": "f", "as": "n", "fn": "length", "col": "s"}, _mat(["s", "n"])),
    "sort": ({"op": "sort", "in": "f", "by": [{"col": "i", "desc": True}, "x"]}, _mat(["x"])),
    "topk": ({"op": "topk", "in": "f", "by": [{"col": "i", "desc": True}, "x"], "k": 5}, _mat(["x"])),
    "set_op": ({"op": "set_op", "kind": "intersect", "left": "f", "left_cols": ["x"], "right": "uf", "right_cols": ["k"]}, _mat(["x"])),
    "window_rank": ({"op": "window", "in": "f", "partition_by": ["i"], "order_by": ["x"], "fns": [{"fn": "rank", "as": "r"}]}, _mat(["x", "r"])),
}


@pytest.mark.parametrize("case", list(DUPLICATE_OUT))
def test_duplicate_out_releases_what_the_step_built(ctx, tabs, case):
    """the step has done its device work when `put` finds the name taken ("defined twice"): the fresh handle goes back"""
    last, tail = DUPLICATE_OUT[case]
    good = {"name": "pf_" + case, "steps": PREFIX + [dict(last, out="z")] + tail, "result": "result"}
    clash = dict(last, out="z", mark_out="f") if case == "join_probe_mark_out" else dict(last, out="f")  # (mark_out: the relation is in, the mark table is not)
    bad = {"name": "pf_" + case, "steps": PREFIX + [clash], "result": "result"}
    err = _fails_clean(ctx, tabs, good, bad, "value 'f' defined twice")
    assert "step '%s'" % last["op"] in err


# ---------------------------------------------------------------- other failure paths
def test_result_produced_then_a_later_step_fails(ctx, tabs):
    """the table named `result` is released too when the run fails after it was made"""
    def plan(col):
        return {"name": "pf_result_first", "steps": [PREFIX[0], {"op": "materialize", "in": "f", "cols": ["x", "i"], "out": "result"},
                                                     {"op": "filter", "in": "f", "preds": [{"col": col, "op": "LT", "value": 7}], "out": "g"}], "result": "result"}

    err = _fails_clean(ctx, tabs, plan("x"), plan("nope"), "no column 'nope'")
    assert "step 'filter' → 'g'" in err


@pytest.mark.parametrize("how", ["unknown_column", "after_three_iterations"])
def test_loop_body_failure(ctx, how):
    """plans/subop/loop_counter.json failing inside the loop: with an unknown column in the body's last step (the first iteration: its values go),
    and with max_iterations 3 where six are needed (the fourth iteration begins while the loop owns a state an earlier one produced: that goes too)"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lingo-db_amd", "plans", "subop", "loop_counter.json")) as f:
        good = json.load(f)
    bad = json.loads(json.dumps(good))
    if how == "unknown_column":
        bad["steps"][0]["body"][-1]["cols"] = ["nope"]
    else:
        bad["steps"][0]["max_iterations"] = 3
    ctr0 = ctx.register("pf_ctr0", pa.table({"ctr": pa.array([0], pa.int32())}))
    try:
        _fails_clean(ctx, {"ctr0": ctr0}, good, bad, "no column 'nope'" if how == "unknown_column" else "no fixpoint after 3 iterations")
    finally:
        ctr0.release()


def test_prepared_plan_failure_then_success(ctx, tabs):
    """an execution that fails (here: an input without the column a step names) does not spoil the prepared plan: the good inputs give
    the first run's rows again, with at most one more miss"""
    plan = ctx.prepare_plan(json.dumps({"name": "pf_prepared", "steps": [
        {"op": "filter", "in": "t", "preds": [{"col": "i", "op": "LT", "value": 3}], "out": "f"},
        {"op": "groupby", "in": "f", "keys": ["i"], "aggs": [{"fn": "sum", "expr": "x", "as": "sx"}], "out": "g"},
        {"op": "sort", "in": "g", "by": ["i"], "out": "s"},
        {"op": "materialize", "in": "s", "cols": ["i", "sx"], "out": "result"}], "result": "result"}))
    other = ctx.register("pf_other", pa.table({"x": pa.array(X, pa.int32())}))  # no column i
    try:
        def rows():
            r = plan.execute({"t": tabs["t"]})
            out = r.to_arrow().to_pylist()
            r.release()
            return out

        first = rows()
        assert first == [{"i": i, "sx": sum(x for x in X if I[x] == i)} for i in range(3)]
        assert rows() == first  # records or replays
        before = plan.stats()
        with pytest.raises(capi.LdbError) as e:
            plan.execute({"t": other})
        assert "no column 'i'" in str(e.value)
        assert rows() == first
        assert plan.stats()["misses"] <= before["misses"] + 1
        assert ctx.desc_cache_stats()["held"] == 0
    finally:
        plan.release()
        other.release()


def test_chunked_conjuncts_and_residuals_succeed_and_balance(ctx, tabs):
    """nine conjuncts (two scan_filter calls) and three residuals (two in the probe, one filter behind it): the rows plain Python
    gives over the 64 rows, and after the result is released the balance is back"""
    nine = {"name": "pf_nine", "steps": PREFIX[:1] + [{"op": "filter", "in": "f", "preds": NINE, "out": "z"}, {"op": "sort", "in": "z", "by": ["x"], "out": "zs"},
                                                      {"op": "materialize", "in": "zs", "cols": ["x"], "out": "result"}], "result": "result"}
    three = {"name": "pf_three", "steps": PREFIX + [{"op": "join_probe", "ht": "h", "in": "f", "keys": ["x"], "kind": "inner", "residual": THREE, "out": "z"},
                                                   {"op": "sort", "in": "z", "by": ["x"], "out": "zs"}, {"op": "materialize", "in": "zs", "cols": ["x", "k"], "out": "result"}], "result": "result"}
    want_nine = [{"x": x} for x in X if 3 <= x < 60 and x not in (10, 11, 20, 33) and I[x] <= 3 and x > 1]
    want_three = [{"x": x, "k": x} for x in K if I[x] != x]
    assert len(want_nine) > 8 and 0 < len(want_three) < len(K)
    for plan, want in ((nine, want_nine), (three, want_three)):
        ctx.run_plan(json.dumps(plan), tabs).release()
        live = _live(ctx)
        r = ctx.run_plan(json.dumps(plan), tabs)
        assert r.to_arrow().to_pylist() == want
        r.release()
        assert _live(ctx) == live
        assert ctx.desc_cache_stats()["held"] == 0
