"""Date functions on the device (csrc/ldb_datefn.hip: ldb_gpu_map_datefn; `datediff` in expression programs): values, validity
and result type bit-exact against tests/datefn_eval.py, the plain-Python restatement that tests/test_datefn_api.py pins to the
reference's recorded answers and to datetime.  Row counts sit at the 4-row vector of the dense kernel and its tail, the
64-row ballot word of the row kernel and the 256-thread block; every count runs dense, sliced, with a validity bitmap and
behind row ids."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi
import datefn_eval as E

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART = {p: k for k, p in enumerate(E.PARTS)}
NS_1678 = -9214560000000000000  # 1678-01-01T00:00:00: an earlier instant truncates to a value outside int64 (not pinned)
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1027]


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLD, "ref_datefn.json")) as f:
        return json.load(f)


def day_arr(days):
    return pa.array(days, pa.int32()).cast(pa.date32())


def values(tab, typ):
    """the one column of `tab` as Python ints with None for NULL; its Arrow type must be `typ`"""
    arr = tab.to_arrow().column(0).combine_chunks()
    assert arr.type == typ, (arr.type, typ)
    out = (arr.cast(pa.int32()) if typ == pa.date32() else arr).to_pylist()
    tab.release()
    return out


def first_diff(got, want, what):
    if got != want:
        assert len(got) == len(want), (what, len(got), len(want))
        k = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: row %d of %d: got %r want %r" % (what, k, len(want), got[k], want[k]))


def check_column(rel, col, vals, is_date, what, trunc=True):
    """EXTRACT and TRUNC of every part over (rel, col), whose rows hold `vals`"""
    typ = pa.date32() if is_date else pa.int64()
    for part in E.PARTS:
        got = values(rel.map_datefn(col, capi.DF_EXTRACT, PART[part]), pa.int64())
        first_diff(got, [E.extract(part, v, is_date) for v in vals], "%s extract %s" % (what, part))
        if trunc:
            got = values(rel.map_datefn(col, capi.DF_TRUNC, PART[part]), typ)
            first_diff(got, [E.trunc(part, v, is_date) for v in vals], "%s trunc %s" % (what, part))


def check_add(rel, col, vals, is_date, months, what, months_col=None):
    """months: the constant, or the per-row values of months_col"""
    per_row = months if months_col is not None else [months] * len(vals)
    got = values(rel.map_datefn(col, capi.DF_ADD_MONTHS, None, 0 if months_col is not None else months, months_col), pa.date32() if is_date else pa.int64())
    want = [E.add_months(v, m, is_date) for v, m in zip(vals, per_row)]
    first_diff(got, want, what)
    return want


def sample(n, seed):
    rng = np.random.default_rng(seed)
    days = [int(x) for x in rng.integers(E.DATE32_MIN, E.DATE32_MAX, n, endpoint=True)]
    nss = [int(x) for x in rng.integers(NS_1678, E.INT64_MAX, n, endpoint=True)]
    for k, (d, t) in enumerate([(0, 0), (-1, -1), (E.DATE32_MIN, NS_1678), (E.DATE32_MAX, E.INT64_MAX), (19782, -86400000000001), (11016, 951868799999999999)][:n]):
        days[(k * 5) % n], nss[(k * 5) % n] = d, t
    return days, nss


# ---------------------------------------------------------------- every size, five ways
@pytest.mark.parametrize("n", SIZES)
def test_sizes_dense_sliced_nullable_and_filtered(ctx, n):
    days, nss = sample(n + 3, 100 + n)
    months = [(-1) ** i * (i % 27) for i in range(n + 3)]
    full = pa.table({"d": day_arr(days), "t": pa.array(nss, pa.int64()), "m": pa.array(months, pa.int32()), "k": pa.array([i % 10 for i in range(n + 3)], pa.int32())})
    for off in (0, 1, 3):  # dense, and sliced: the registered column starts inside the Arrow buffer
        t = ctx.register("datefn_off%d" % off, full.slice(off, n))
        r = t.rel()
        assert t.rows == n
        check_column(r, (0, 0), days[off:off + n], True, "date32 n=%d offset %d" % (n, off))
        check_column(r, (0, 1), nss[off:off + n], False, "int64 n=%d offset %d" % (n, off))
        check_add(r, (0, 0), days[off:off + n], True, 1, "date32 + 1 month n=%d offset %d" % (n, off))
        check_add(r, (0, 1), nss[off:off + n], False, months[off:off + n], "int64 + months column n=%d offset %d" % (n, off), months_col=(0, 2))
        r.release(), t.release()
    # a validity bitmap: NULL every 7th row
    nd = [None if i % 7 == 3 else v for i, v in enumerate(days[:n])]
    nt = [None if i % 7 == 5 else v for i, v in enumerate(nss[:n])]
    t = ctx.register("datefn_nulls", pa.table({"d": day_arr(nd), "t": pa.array(nt, pa.int64()), "m": pa.array(months[:n], pa.int32()), "k": pa.array([i % 10 for i in range(n)], pa.int32())}))
    r = t.rel()
    check_column(r, (0, 0), nd, True, "date32 with NULLs n=%d" % n)
    check_column(r, (0, 1), nt, False, "int64 with NULLs n=%d" % n)
    check_add(r, (0, 0), nd, True, months[:n], "date32 with NULLs + months column n=%d" % n, months_col=(0, 2))
    check_add(r, (0, 1), nt, False, -13, "int64 with NULLs - 13 months n=%d" % n)
    # row ids: behind a filter
    f = r.scan_filter([api.pred((0, 3), capi.F_LT, 6)])
    keep = [i for i in range(n) if i % 10 < 6]
    check_column(f, (0, 0), [nd[i] for i in keep], True, "date32 behind a filter n=%d" % n)
    check_column(f, (0, 1), [nt[i] for i in keep], False, "int64 behind a filter n=%d" % n)
    check_add(f, (0, 1), [nt[i] for i in keep], False, [months[i] for i in keep], "int64 behind a filter + months column n=%d" % n, months_col=(0, 2))
    f.release(), r.release(), t.release()


def test_dense_result_has_no_bitmap_and_keeps_the_null_count(ctx):
    t = ctx.register("datefn_nc", pa.table({"d": day_arr([1, None, 3, 4, None]), "t": pa.array([1, 2, 3, 4, 5], pa.int64())}))
    r = t.rel()
    a = r.map_datefn((0, 0), capi.DF_EXTRACT, capi.DP_DAY).to_arrow().column(0)
    b = r.map_datefn((0, 1), capi.DF_TRUNC, capi.DP_DAY).to_arrow().column(0)
    assert a.null_count == 2 and a.to_pylist() == [2, None, 4, 5, None] and b.null_count == 0 and b.to_pylist() == [0] * 5


def test_outer_join_padded_side(ctx):
    n = 300
    days, nss = sample(n, 7)
    t = ctx.register("datefn_build", pa.table({"d": day_arr(days), "t": pa.array(nss, pa.int64()), "k": pa.array(list(range(n)), pa.int64())}))
    probe = ctx.register("datefn_probe", pa.table({"k": pa.array([5, 2000, 7, 3000, 299, 0, 4000, 6] * 9, pa.int64())}))
    j = t.rel().join_build([(0, 2)], unique=True).probe(probe.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    bk = j.rowids(1).tolist()
    assert sum(1 for b in bk if b == capi.LDB_NULL_ROW) == 27 and len(bk) == 72
    sd = [None if b == capi.LDB_NULL_ROW else days[b] for b in bk]
    st = [None if b == capi.LDB_NULL_ROW else nss[b] for b in bk]
    check_column(j, (1, 0), sd, True, "outer join side, date32")
    check_column(j, (1, 1), st, False, "outer join side, int64")
    want = check_add(j, (1, 0), sd, True, 2, "outer join side + 2 months")
    assert sum(w is None for w in want) >= 27


# ---------------------------------------------------------------- the reference's recorded answers through the device
def test_fixture_instants_through_the_device(ctx, ref):
    ts = ref["instants"]
    t = ctx.register("datefn_ref", pa.table({"t": pa.array(ts, pa.int64())}))
    r = t.rel()
    for part in E.PARTS:
        assert values(r.map_datefn((0, 0), capi.DF_EXTRACT, PART[part]), pa.int64()) == ref["extract"][part], part
        got = values(r.map_datefn((0, 0), capi.DF_TRUNC, PART[part]), pa.int64())
        first_diff([g for g, w in zip(got, ref["trunc"][part]) if w is not None], [w for w in ref["trunc"][part] if w is not None], "trunc " + part)
    sub = ref["month_instants"]
    whole = [k for k, x in enumerate(sub) if x % E.NS_PER_DAY == 0]
    assert len(whole) >= 5
    tm = ctx.register("datefn_ref_m", pa.table({"t": pa.array(sub, pa.int64()), "d": day_arr([x // E.NS_PER_DAY for x in sub])}))
    rm = tm.rel()
    for j, m in enumerate(ref["months"]):
        add, subtract = [row[j] for row in ref["add_months"]], [row[j] for row in ref["subtract_months"]]
        assert values(rm.map_datefn((0, 0), capi.DF_ADD_MONTHS, months=m), pa.int64()) == add, m
        assert values(rm.map_datefn((0, 0), capi.DF_ADD_MONTHS, months=-m), pa.int64()) == subtract, m
        got = values(rm.map_datefn((0, 1), capi.DF_ADD_MONTHS, months=m), pa.date32())
        assert [got[k] for k in whole] == [add[k] // E.NS_PER_DAY for k in whole], m


def test_extreme_int32_days(ctx):
    days = [-(2 ** 31), -(2 ** 31) + 1, 2 ** 31 - 1, 2 ** 31 - 2, -1, 0, 1, -719468, -719469, -719467, 2 ** 31 - 719468 - 1, 2 ** 31 - 719468, 2 ** 31 - 719468 + 1, -(2 ** 31) + 719468, E.DATE32_MIN - 1,
            E.DATE32_MAX + 1]
    assert E.extract("year", 2 ** 31 - 1, True) == 5881580 and E.extract("year", -(2 ** 31), True) == -5877641
    for reps in (1, 5):  # the tail lanes alone, and the 4-row vector
        vals = days * reps
        t = ctx.register("datefn_extreme", pa.table({"d": day_arr(vals), "k": pa.array([0] * len(vals), pa.int32())}))
        check_column(t.rel(), (0, 0), vals, True, "extreme days, dense", trunc=False)
        check_column(t.rel().scan_filter([api.pred((0, 1), capi.F_EQ, 0)]), (0, 0), vals, True, "extreme days, row ids", trunc=False)
        want = check_add(t.rel(), (0, 0), vals, True, 0, "extreme days + 0 months")  # outside 0001 … 9999: NULL, whatever the shift
        assert [w is None for w in want[:len(days)]] == [not E.DATE32_MIN <= d <= E.DATE32_MAX for d in days]


# ---------------------------------------------------------------- ADD_MONTHS: the range rules
def ns_of(y, m, d, hh=0, mm=0, ss=0):
    return E.days_from_civil(y, m, d) * E.NS_PER_DAY + (hh * 3600 + mm * 60 + ss) * 10 ** 9


def test_add_months_null_by_range_and_by_input(ctx):
    d = E.days_from_civil
    days = [E.DATE32_MAX, E.DATE32_MAX - 31, E.DATE32_MIN, E.DATE32_MIN + 31, d(2023, 1, 31), d(2024, 1, 31), d(2023, 3, 31), d(2023, 1, 15), None, d(1999, 12, 31), d(9999, 1, 1), d(1, 12, 31)] + list(range(0, 4000, 97))
    n = len(days)
    t64 = [ns_of(2262, 3, 1), ns_of(2261, 3, 1, 5, 6, 7), ns_of(1678, 1, 1), ns_of(1679, 1, 1), ns_of(2023, 12, 15, 1, 1, 1), E.INT64_MAX, E.INT64_MIN, None] + [ns_of(1990, 1, 1) + 10 ** 15 * k + k for k in range(n - 8)]
    mcol = [1, 1, -1, -1, 1, 1, -1, -13, 5, None, 10 ** 12, -(10 ** 12)] + [(-1) ** k * (k * 7 % 50) for k in range(n - 12)]
    m32 = [None if m is None else max(-(2 ** 31), min(2 ** 31 - 1, m)) for m in mcol]
    t = ctx.register("datefn_add", pa.table({"d": day_arr(days), "t": pa.array(t64, pa.int64()), "m": pa.array(mcol, pa.int64()), "m32": pa.array(m32, pa.int32())}))
    r = t.rel()

    def by_range(vals, months, want):
        return [v is not None and m is not None and w is None for v, m, w in zip(vals, months, want)]

    # constants
    for m in (1, -1, 12, -12, 14, 240000, -240000):
        for col, vals, is_date in (((0, 0), days, True), ((0, 1), t64, False)):
            want = check_add(r, col, vals, is_date, m, "constant %d, %s" % (m, "date32" if is_date else "int64"))
            if abs(m) < 240000:
                assert 0 < sum(by_range(vals, [m] * n, want)) < n / 4
    w = check_add(r, (0, 0), days, True, 1, "date32 + 1")
    assert w[0] is None and w[1] == E.DATE32_MAX - 1 and w[4] == d(2023, 3, 3) and w[5] == d(2024, 3, 2) and w[8] is None  # 9999-12-31 + 1; no clamping
    w = check_add(r, (0, 0), days, True, -1, "date32 - 1")
    assert w[2] is None and w[3] == E.DATE32_MIN and w[6] == d(2023, 3, 3)  # 0001-01-01 - 1
    w = check_add(r, (0, 1), t64, False, 12, "int64 + 12")
    assert w[0] is None and w[1] == ns_of(2262, 3, 1, 5, 6, 7) and w[5] is None and w[6] is not None and w[7] is None  # a 2262 instant + 12
    w = check_add(r, (0, 1), t64, False, 14, "int64 + 14")
    assert w[4] == ns_of(2025, 2, 15, 1, 1, 1)
    # per row: int64 and int32 months, a NULL month, |m| = 10^12
    for mc, months in (((0, 2), mcol), ((0, 3), m32)):
        w = check_add(r, (0, 0), days, True, months, "date32 + months column %d" % mc[1], months_col=mc)
        assert w[9] is None and w[10] is None and w[11] is None and w[7] == d(2021, 12, 15) and 0 < sum(by_range(days, months, w)) < n / 4
        w = check_add(r, (0, 1), t64, False, months, "int64 + months column %d" % mc[1], months_col=mc)
        assert w[9] is None and w[10] is None and w[11] is None and 0 < sum(by_range(t64, months, w)) < n / 4
    # `months` is ignored when a column is given, `part` always
    got = values(r.map_datefn((0, 0), capi.DF_ADD_MONTHS, 77, 10 ** 12, (0, 2)), pa.date32())
    assert got == [E.add_months(v, m, True) for v, m in zip(days, mcol)]


def test_invalid_arguments_do_no_work(ctx):
    t = ctx.register("datefn_bad", pa.table({"d": day_arr([1]), "t": pa.array([1], pa.int64()), "s": pa.array(["x"], pa.string()), "i": pa.array([1], pa.int32()), "f": pa.array([1.0], pa.float64()),
                                             "i16": pa.array([1], pa.int16())}))
    r = t.rel()
    cases = [(((0, 0), 3, 0), "function"), (((0, 0), -1, 0), "function"), (((0, 0), capi.DF_EXTRACT, 6), "part"), (((0, 1), capi.DF_TRUNC, -1), "part"), (((0, 2), capi.DF_EXTRACT, 0), "date32 or int64"),
             (((0, 3), capi.DF_TRUNC, 0), "date32 or int64"), (((0, 4), capi.DF_ADD_MONTHS, 0, 1), "date32 or int64"), (((0, 0), capi.DF_ADD_MONTHS, 0, 0, (0, 2)), "months column"),
             (((0, 0), capi.DF_ADD_MONTHS, 0, 0, (0, 4)), "months column"), (((0, 1), capi.DF_ADD_MONTHS, 0, 0, (0, 5)), "months column")]
    for args, word in cases:
        before = ctx.mem_stats()["live_blocks"]
        with pytest.raises(capi.LdbError) as e:
            r.map_datefn(*args)
        assert e.value.status == capi.LDB_ERR_INVALID and word in str(e.value), str(e.value)
        assert ctx.mem_stats()["live_blocks"] == before
    lib, out = ctx.lib, C.c_void_p()
    ref = api.colref(0, 0)
    for a in ((None, r.h, ref, 0, 0, 0, None, b"x", C.byref(out)), (ctx.h, None, ref, 0, 0, 0, None, b"x", C.byref(out)), (ctx.h, r.h, ref, 0, 0, 0, None, b"x", None)):
        assert lib.ldb_gpu_map_datefn(*a) == capi.LDB_ERR_INVALID and not out.value
    # an unused argument is not looked at: a months column of any type with EXTRACT, any part with ADD_MONTHS
    assert values(r.map_datefn((0, 0), capi.DF_EXTRACT, capi.DP_DAY, 5, (0, 2)), pa.int64()) == [2]
    assert values(r.map_datefn((0, 0), capi.DF_ADD_MONTHS, 99, 1), pa.date32()) == [32]


# ---------------------------------------------------------------- the plan language
def test_plan_steps_end_to_end(ctx):
    n = 1000
    rng = np.random.default_rng(5)
    ts = [int(x) for x in rng.integers(ns_of(1969, 6, 1), ns_of(1971, 6, 1), n)]
    days = [int(x) for x in rng.integers(E.days_from_civil(2023, 11, 1), E.days_from_civil(2024, 4, 1), n)]
    t = ctx.register("datefn_plan", pa.table({"ts": pa.array(ts, pa.int64()), "d": day_arr(days), "k": pa.array(list(range(n)), pa.int64())}))

    def run(steps):
        return ctx.run_plan(json.dumps({"inputs": ["t"], "steps": steps, "result": "result"}), {"t": t}).to_arrow()

    for fn, part, key in (("extract", "month", lambda x: E.extract("month", x, False)), ("date_trunc", "day", lambda x: E.trunc("day", x, False))):
        res = run([{"op": "map", "in": "t", "fn": fn, "part": part, "col": "ts", "as": "g", "out": "r1"},
                   {"op": "groupby", "in": "r1", "keys": ["g"], "aggs": [{"fn": "count_star", "as": "c"}], "key_names": ["g"], "out": "gb"}, {"op": "materialize", "in": "gb", "cols": ["g", "c"], "out": "result"}])
        assert res.column(0).type == pa.int64() and dict(zip(res.column(0).to_pylist(), res.column(1).to_pylist())) == dict(collections.Counter(key(x) for x in ts)), fn
    res = run([{"op": "map", "in": "t", "fn": "add_months", "col": "d", "months": 1, "as": "d2", "out": "r1"}, {"op": "filter", "in": "r1", "preds": [{"col": "d2", "op": "GTE", "value": "2024-03-01"}], "out": "r2"},
               {"op": "materialize", "in": "r2", "cols": ["k", "d2"], "out": "result"}])
    want = [(k, E.add_months(x, 1, True)) for k, x in enumerate(days) if E.add_months(x, 1, True) >= E.days_from_civil(2024, 3, 1)]
    assert 0 < len(want) < n and res.column(1).type == pa.date32() and sorted(zip(res.column(0).to_pylist(), res.column(1).cast(pa.int32()).to_pylist())) == want
    res = run([{"op": "map", "in": "t", "fn": "add_months", "col": "ts", "months_col": "k", "as": "t2", "out": "r1"}, {"op": "materialize", "in": "r1", "cols": ["t2"], "out": "result"}])
    assert res.column(0).to_pylist() == [E.add_months(x, k, False) for k, x in enumerate(ts)]
    with pytest.raises(capi.LdbError) as e:
        run([{"op": "map", "in": "t", "fn": "extract", "part": "week", "col": "ts", "as": "g", "out": "result"}])
    assert "week" in str(e.value)


def test_datediff_expression(ctx):
    n = 257
    rng = np.random.default_rng(11)
    a = [None if i % 31 == 4 else int(x) for i, x in enumerate(rng.integers(ns_of(1900, 1, 1), ns_of(2100, 1, 1), n))]
    b = [None if i % 37 == 6 else int(x) for i, x in enumerate(rng.integers(ns_of(1900, 1, 1), ns_of(2100, 1, 1), n))]
    a[:6], b[:6] = [0, 1_500_000_000, 0, 90 * 10 ** 9, 5, -1], [1_500_000_000, 0, 90 * 10 ** 9, 0, 5, 86_400 * 10 ** 9]
    da = [None if x is None else x // E.NS_PER_DAY for x in a]
    db = [None if x is None else x // E.NS_PER_DAY for x in b]
    t = ctx.register("datefn_diff", pa.table({"a": pa.array(a, pa.int64()), "b": pa.array(b, pa.int64()), "da": day_arr(da), "db": day_arr(db)}))
    for unit in ("day", "hour", "minute", "second"):
        for e, s, ev, sv, is_date in (("a", "b", a, b, False), ("da", "db", da, db, True)):
            plan = {"inputs": ["t"], "steps": [{"op": "map", "in": "t", "expr": {"datediff": [unit, e, s]}, "as": "x", "out": "r1"}, {"op": "materialize", "in": "r1", "cols": ["x"], "out": "result"}], "result": "result"}
            res = ctx.run_plan(json.dumps(plan), {"t": t}).to_arrow()
            want = [E.datediff(unit, x, y, is_date) for x, y in zip(ev, sv)]
            assert res.column(0).type == pa.int64() and any(w is not None and w < 0 for w in want)
            first_diff(res.column(0).to_pylist(), want, "datediff %s %s" % (unit, "date32" if is_date else "int64"))
    for bad in (["week", "a", "b"], ["day", "a", "db"], ["day", "a"]):
        with pytest.raises(capi.LdbError):
            ctx.run_plan(json.dumps({"inputs": ["t"], "steps": [{"op": "map", "in": "t", "expr": {"datediff": bad}, "as": "x", "out": "result"}], "result": "result"}), {"t": t})
