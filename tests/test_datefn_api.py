"""Date functions without a device: the plain-Python restatement (tests/datefn_eval.py) against the reference's recorded
answers (tests/golden/ref_datefn.json, written by tests/golden/make_ref_datefn.py from DateRuntime itself) and against
datetime; the C-ABI's symbol and enums; the plan checker over the new map forms and `datediff`; the dump translator over
Extract…FromDate / DateTrunc.  The device half is tests/test_gpu_datefn.py."""
import ctypes as C
import datetime
import json
import os
import random
import subprocess
import tempfile

import pytest

from lingodb_amd import api, capi
import datefn_eval as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLD, "ref_datefn.json")) as f:
        return json.load(f)


def test_extract_and_trunc_equal_the_reference(ref):
    ts = ref["instants"]
    assert len(ts) > 400 and tuple(ref["parts"]) == E.PARTS
    for part in E.PARTS:
        assert [E.extract(part, t, False) for t in ts] == ref["extract"][part], part
        want = ref["trunc"][part]
        assert sum(w is not None for w in want) > 350
        for t, w in zip(ts, want):
            if w is not None:  # (null: before 1678-01-01, outside the reference's domain)
                assert E.trunc(part, t, False) == w, (part, t)


def test_floor_semantics_of_negative_instants(ref):
    at = {t: k for k, t in enumerate(ref["instants"])}
    for t, want in ((-1, (1969, 12, 31, 23, 59, 59)), (-86400000000001, (1969, 12, 30, 23, 59, 59)), (0, (1970, 1, 1, 0, 0, 0)), (1_500_000_000, (1970, 1, 1, 0, 0, 1))):
        assert tuple(ref["extract"][p][at[t]] for p in E.PARTS) == want
        assert tuple(E.extract(p, t, False) for p in E.PARTS) == want


def test_add_and_subtract_months_equal_the_reference(ref):
    ms, ts = ref["months"], ref["month_instants"]
    assert len(ts) == 100 and set(ms) == {0, 1, -1, 11, -11, 12, -12, 13, -13, 25, -120}
    for t, add, sub in zip(ts, ref["add_months"], ref["subtract_months"]):
        assert [E.add_months(t, m, False) for m in ms] == add, t
        assert [E.add_months(t, -m, False) for m in ms] == sub, t
        if t % E.NS_PER_DAY == 0:  # the same shift over the day number
            assert [E.add_months(t // E.NS_PER_DAY, m, True) for m in ms] == [a // E.NS_PER_DAY for a in add]


def ns(y, m, d, hh=0, mm=0, ss=0):
    return (datetime.date(y, m, d) - datetime.date(1970, 1, 1)).days * E.NS_PER_DAY + (hh * 3600 + mm * 60 + ss) * 10 ** 9


def test_months_are_not_clamped(ref):
    """the reference's month arithmetic, unlike PostgreSQL's: a day past the end of the target month runs over"""
    cases = [(ns(2023, 1, 31), 1, ns(2023, 3, 3)), (ns(2024, 1, 31), 1, ns(2024, 3, 2)), (ns(2023, 3, 31), -1, ns(2023, 3, 3)), (ns(2023, 12, 15, 1, 1, 1), 14, ns(2025, 2, 15, 1, 1, 1)),
             (ns(2023, 1, 15), -13, ns(2021, 12, 15))]
    for t, m, want in cases:
        assert E.add_months(t, m, False) == want
    i = ref["month_instants"].index(ns(2023, 1, 31))
    assert ref["add_months"][i][ref["months"].index(1)] == ns(2023, 3, 3)


def test_null_rules_of_add_months():
    assert E.add_months(None, 1, True) is None and E.add_months(0, None, True) is None
    assert E.add_months(E.DATE32_MAX, 1, True) is None and E.add_months(E.DATE32_MAX, 0, True) == E.DATE32_MAX and E.add_months(E.DATE32_MAX - 31, 1, True) == E.DATE32_MAX - 1  # 9999-11-30 → 9999-12-30
    assert E.add_months(E.DATE32_MIN, -1, True) is None and E.add_months(E.DATE32_MIN, 1, True) == E.DATE32_MIN + 31
    assert E.add_months(0, 10 ** 12, True) is None and E.add_months(0, 240001, False) is None and E.add_months(0, -240001, True) is None
    assert E.add_months(ns(2262, 3, 1), 12, False) is None and E.add_months(ns(2262, 3, 1), 1, False) == ns(2262, 4, 1)
    assert E.add_months(ns(1678, 1, 1), -12, False) is None and E.add_months(ns(1678, 1, 1), -3, False) == ns(1677, 10, 1)


def test_datediff_equals_the_reference(ref):
    pairs = ref["diff_pairs"]
    assert len(pairs) > 300 and any(e < s for e, s in pairs)
    for unit in ("day", "hour", "minute", "second"):
        assert [E.datediff(unit, e, s, False) for e, s in pairs] == ref["diff"][unit], unit
    assert E.datediff("second", 0, 1_500_000_000, False) == -1 and E.datediff("minute", 0, 90 * 10 ** 9, False) == -1
    assert E.datediff("hour", 3, 5, True) == -48 and E.datediff("day", None, 5, True) is None


def test_date32_against_datetime():
    """extract and trunc over day numbers, 0001 … 9999: 5 000 seeded days, both end days, leap days"""
    rng = random.Random(20261021)
    epoch = datetime.date(1970, 1, 1)
    days = [rng.randint(E.DATE32_MIN, E.DATE32_MAX) for _ in range(5000)] + [E.DATE32_MIN, E.DATE32_MAX, 0, -1]
    days += [(datetime.date(y, 2, 29) - epoch).days for y in (4, 1600, 1904, 2000, 2024, 2400, 9996)] + [(datetime.date(y, 3, 1) - epoch).days - 1 for y in (1, 1700, 1900, 2100, 2023)]
    for z in days:
        d = epoch + datetime.timedelta(days=z)
        assert (E.extract("year", z, True), E.extract("month", z, True), E.extract("day", z, True)) == (d.year, d.month, d.day), z
        assert E.civil_from_days(z) == (d.year, d.month, d.day) and E.days_from_civil(d.year, d.month, d.day) == z
        assert (E.extract("hour", z, True), E.extract("minute", z, True), E.extract("second", z, True)) == (0, 0, 0)
        assert E.trunc("year", z, True) == (d.replace(month=1, day=1) - epoch).days and E.trunc("month", z, True) == (d.replace(day=1) - epoch).days
        assert all(E.trunc(p, z, True) == z for p in ("day", "hour", "minute", "second"))
        assert E.extract("day", z * E.NS_PER_DAY + 86_399_999_999_999, False) == d.day


def test_symbol_and_enum_values():
    lib = capi.gpu_lib()
    assert hasattr(lib, "ldb_gpu_map_datefn") and "ldb_gpu_map_datefn" in capi.GPU_API
    prog = r'''
#include "lingodb_gpu.h"
#include <stdio.h>
#ifdef CHECK_PROTOTYPE /* (compiled only: an incompatible prototype is an error) */
int32_t (*f)(ldb_ctx*, ldb_rel*, ldb_colref, int32_t, int32_t, int64_t, const ldb_colref*, const char*, ldb_table**) = ldb_gpu_map_datefn;
#endif
int main(void){ printf("%d %d %d %d %d %d %d %d %d\n", LDB_DF_EXTRACT, LDB_DF_TRUNC, LDB_DF_ADD_MONTHS, LDB_DP_YEAR, LDB_DP_MONTH, LDB_DP_DAY, LDB_DP_HOUR, LDB_DP_MINUTE, LDB_DP_SECOND); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-Werror", "-DCHECK_PROTOTYPE", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "s.o")])
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [capi.DF_EXTRACT, capi.DF_TRUNC, capi.DF_ADD_MONTHS, capi.DP_YEAR, capi.DP_MONTH, capi.DP_DAY, capi.DP_HOUR, capi.DP_MINUTE, capi.DP_SECOND] == [0, 1, 2, 0, 1, 2, 3, 4, 5]
    assert hasattr(api.Rel, "map_datefn")


def check(plan, inputs=("t",)):
    lib = capi.host_lib()
    arr = (C.c_char_p * len(inputs))(*[n.encode() for n in inputs])
    st = lib.ldb_plan_json_check(json.dumps(plan).encode(), arr, len(inputs))
    return st, lib.ldb_plan_json_last_error().decode()


def plan_of(step):
    return {"inputs": ["t"], "steps": [{"op": "scan", "table": "t", "out": "r"}, dict(step, **{"op": "map", "in": "r", "out": "the_step"})], "result": "the_step"}


@pytest.mark.parametrize("step", [
    {"fn": "extract", "part": "month", "col": "d", "as": "v"},
    {"fn": "extract", "part": "second", "col": "ts", "as": "v"},
    {"fn": "date_trunc", "part": "day", "col": "ts", "as": "v"},
    {"fn": "date_trunc", "part": "year", "col": "d", "as": "v"},
    {"fn": "add_months", "col": "d", "months": 3, "as": "v"},
    {"fn": "add_months", "col": "d", "months": -14, "as": "v"},
    {"fn": "add_months", "col": "d", "months_col": "m", "as": "v"},
    {"expr": {"datediff": ["day", "a", "b"]}, "as": "v"},
    {"expr": {"datediff": ["second", "a", "b"]}, "as": "v"},
    {"fn": "extract_year", "col": "d", "as": "v"},
])
def test_checker_accepts_the_date_forms(step):
    st, err = check(plan_of(step))
    assert st == capi.LDB_OK, err


@pytest.mark.parametrize("step, word", [
    ({"fn": "extract", "col": "d", "as": "v"}, "part"),
    ({"fn": "date_trunc", "col": "d", "as": "v"}, "part"),
    ({"fn": "extract", "part": "week", "col": "d", "as": "v"}, "week"),
    ({"fn": "date_trunc", "part": "quarter", "col": "d", "as": "v"}, "quarter"),
    ({"fn": "extract", "part": 3, "col": "d", "as": "v"}, "part"),
    ({"fn": "add_months", "col": "d", "months": 1, "months_col": "m", "as": "v"}, "not both"),
    ({"fn": "add_months", "col": "d", "as": "v"}, "months"),
    ({"fn": "add_months", "col": "d", "months": "3", "as": "v"}, "number"),
    ({"fn": "extract", "part": "month", "as": "v"}, "col"),
    ({"fn": "add_months", "months": 1, "as": "v"}, "col"),
])
def test_checker_rejects_malformed_date_forms(step, word):
    st, err = check(plan_of(step))
    assert st == capi.LDB_ERR_INVALID and word in err, err
    if "fn" in step and "col" in step:
        assert "the_step" in err and step["fn"] in err, err  # the message names the step


def q7_dump():
    with open(os.path.join(GOLD, "subop_tpch_q7.json")) as f:
        return f.read()


def test_translator_keeps_extract_year():
    plan = json.loads(api.translate_subop_dump(q7_dump(), "tpch_q7")[0])
    maps = [s for s in plan["steps"] if s["op"] == "map" and "fn" in s]
    assert [m["fn"] for m in maps] == ["extract_year"] and "part" not in maps[0]


@pytest.mark.parametrize("call, part", [("ExtractMonthFromDate", "month"), ("ExtractDayFromDate", "day"), ("ExtractHourFromDate", "hour"), ("ExtractMinuteFromDate", "minute"),
                                        ("ExtractSecondFromDate", "second")])
def test_translator_maps_the_other_extracts(call, part):
    text = q7_dump()
    assert text.count("ExtractYearFromDate(") == 1
    plan_text, report = api.translate_subop_dump(text.replace("ExtractYearFromDate(", call + "("), "tpch_q7")
    assert all(r["target"] == "gpu" for r in report)
    plan = json.loads(plan_text)
    maps = [s for s in plan["steps"] if s["op"] == "map" and "fn" in s]
    assert len(maps) == 1 and maps[0]["fn"] == "extract" and maps[0]["part"] == part and maps[0]["col"] == "l_shipdate"
    lib = capi.host_lib()
    ins = plan["inputs"]
    arr = (C.c_char_p * len(ins))(*[n.encode() for n in ins])
    assert lib.ldb_plan_json_check(plan_text.encode(), arr, len(ins)) == capi.LDB_OK, lib.ldb_plan_json_last_error()


def with_date_trunc(part_json):
    """Q7's dump with extract(year from l_shipdate) replaced by date_trunc(<part>, l_shipdate): the part as the call's first operand"""
    doc = json.loads(q7_dump())
    hits = []

    def walk(x):
        if isinstance(x, dict):
            if x.get("type") == "expression_inner" and x.get("strings") == ["ExtractYearFromDate(", ")"]:
                hits.append(x)
            for v in x.values():
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)

    walk(doc)
    assert len(hits) == 1
    hits[0]["strings"] = ["DateTrunc(", ", ", ")"]
    hits[0]["subExpressions"] = [part_json] + hits[0]["subExpressions"]
    return json.dumps(doc)


def const_leaf(value):
    return {"type": "expression_leaf", "leaf_type": "constant", "data_type": "string", "value": value}


@pytest.mark.parametrize("part", ["year", "month", "day", "hour", "minute", "second"])
def test_translator_maps_date_trunc(part):
    plan_text, report = api.translate_subop_dump(with_date_trunc(const_leaf(part)), "tpch_q7")
    assert all(r["target"] == "gpu" for r in report)
    maps = [s for s in json.loads(plan_text)["steps"] if s["op"] == "map" and "fn" in s]
    assert len(maps) == 1 and maps[0]["fn"] == "date_trunc" and maps[0]["part"] == part and maps[0]["col"] == "l_shipdate"


def test_translator_refuses_an_unknown_date_trunc_part_and_other_date_calls():
    with pytest.raises(capi.LdbError) as ei:
        api.translate_subop_dump(with_date_trunc(const_leaf("quarter")), "tpch_q7")
    assert "quarter" in str(ei.value) + json.dumps(ei.value.report)
    with pytest.raises(capi.LdbError) as ei:  # month intervals in dumps: not settled
        api.translate_subop_dump(q7_dump().replace("ExtractYearFromDate(", "DateAdd("), "tpch_q7")
    assert "DateAdd" in str(ei.value) + json.dumps(ei.value.report)
