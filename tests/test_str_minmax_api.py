"""MIN / MAX over utf8 columns without a device: the encoding of api.str_minmax is pinned byte for byte (the C-ABI accepts exactly this
shape: one term, one factor, the bare column, a utf8 result), and the constants it relies on; a sub-operator dump whose reduce is a
Min / Max over a string translates to a device group-by; plans/job/17a.json passes the plan checker.  (The plan interpreter resolves column
types from registered tables, so what the `groupby` step makes of a utf8 column — and what it rejects — is checked where tables exist:
tests/test_gpu_str_minmax.py::test_plan_step_and_prepared_replay.)"""
import ctypes as C

import pytest

from lingodb_amd import api, capi


def test_utf8_type_constant_matches_the_header():
    assert capi.T_UTF8 == 7 and (capi.AGG_MIN, capi.AGG_MAX) == (1, 2)


@pytest.mark.parametrize("fn", [capi.AGG_MIN, capi.AGG_MAX])
def test_str_minmax_encoding_is_pinned(fn):
    a = api.str_minmax(fn, (2, 5))
    assert (a.fn, a.wide, a.n_preds, a.avg_pow10, a.out_type, a.out_precision, a.out_scale, a.has_count_expr) == (fn, 0, 0, 0, capi.T_UTF8, 0, 0, 0)
    e = a.arg
    assert (e.n_terms, e.is_float) == (1, 0)
    t = e.t[0]
    assert (t.n_factors, t.negate, t.div_pow10) == (1, 0, 0)
    f = t.f[0]
    assert (f.has_col, f.col.side, f.col.col, f.a, f.b) == (1, 2, 5, 0, 1)
    # byte for byte: the same spec built by hand, field by field, over zeroed memory
    b = capi.AggSpec()
    b.fn = fn
    b.out_type = 7
    b.arg.n_terms = 1
    b.arg.t[0].n_factors = 1
    b.arg.t[0].f[0].has_col = 1
    b.arg.t[0].f[0].col.side = 2
    b.arg.t[0].f[0].col.col = 5
    b.arg.t[0].f[0].b = 1
    assert C.string_at(C.addressof(a), C.sizeof(a)) == C.string_at(C.addressof(b), C.sizeof(b))


def test_str_minmax_refuses_other_functions():
    for fn in (capi.AGG_SUM, capi.AGG_COUNT, capi.AGG_ANY, capi.AGG_AVG):
        with pytest.raises(ValueError):
            api.str_minmax(fn, (0, 0))


def _string_reduce_dump():
    """SELECT MIN(n_name), MAX(n_name) FROM nation as the reference's sub-operator dump (tools/subop_lower.py: a SimpleState, lookup, reduce with the
    Min / Max bodies `state > arg or state is null ? arg : state` over a string-typed member, scan of the state, materialize)"""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [p for p in (os.path.join(root, "tools"),) if p not in sys.path]
    import subop_lower as L

    cx = L.Cx("str_min")
    t = L.Table("nation")
    lo, hi = L.C("aggr0::lo", "string"), L.C("aggr0::hi", "string")
    return L.result(cx, L.Aggregate(t, [], [("min", t["n_name"], lo), ("max", t["n_name"], hi)]), [("lo", lo), ("hi", hi)], write=False)


def test_string_reduce_translates_to_a_device_groupby():
    import json

    text, report = api.translate_subop_dump(_string_reduce_dump(), "str_min")
    assert report and all(r["target"] == "gpu" for r in report), report
    steps = json.loads(text)["steps"]
    gb = [s for s in steps if s["op"] == "groupby"]
    assert len(gb) == 1 and gb[0]["keys"] == []
    assert [(a["fn"], a["expr"]) for a in gb[0]["aggs"]] == [("min", "n_name"), ("max", "n_name")]  # the bare column: what the plan step turns into out_type utf8


def test_job_17a_plan_file_passes_the_plan_checker():
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lingo-db_amd", "plans", "job", "17a.json")
    with open(path) as f:
        text = f.read()
    plan = json.loads(text)
    assert sorted(plan["inputs"]) == ["cast_info", "company_name", "keyword", "movie_companies", "movie_keyword", "name", "title"]
    last = plan["steps"][-1]
    assert last["op"] == "groupby" and last["keys"] == [] and [(a["fn"], a["expr"]) for a in last["aggs"]] == [("min", "n_name"), ("min", "n_name")]
    lib = capi.host_lib()
    arr = (C.c_char_p * len(plan["inputs"]))(*[n.encode() for n in plan["inputs"]])
    assert lib.ldb_plan_json_check(text.encode(), arr, len(plan["inputs"])) == capi.LDB_OK, lib.ldb_plan_json_last_error()
