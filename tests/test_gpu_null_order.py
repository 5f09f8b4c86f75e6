"""Nullable sort keys on the device: ldb_gpu_sort / ldb_gpu_topk / ldb_gpu_window / plan steps with LDB_NULLS_LARGEST — the reference's
comparator over nullable operands (NULL is the largest value, NULLs tie).  Every comparison is bit-exact equality of row-id vectors with the
plain-Python comparator of tests/null_order_ref.py (which tests/test_null_order.py checks without a device, against cases from the reference's
own SQL suite among others); the oracle's sort ignores validity and serves only where no key holds a NULL.  Inputs come from
null_order_ref.cases(); tables are registered once per module."""
import gc
import json
import os

import numpy as np
import pyarrow as pa
import pytest

import null_order_ref
import order_ref
from lingodb_amd import api, capi
from oracle_bind import HostTable

pytestmark = pytest.mark.gpu

CASES = {name: (table, specs) for name, table, specs in null_order_ref.cases()}
TOPK_CASES = [n for n in CASES if n.startswith("topk_")]
SORT_CASES = [n for n in CASES if not n.startswith("topk_")]
NULL_ROW = null_order_ref.NULL_ROW
N1 = capi.NULLS_LARGEST
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_null_order.json")) as f:
    FIXTURE = json.load(f)


class World:
    """device tables, each made once (keyed by the identity of the pyarrow table and the form of registration)"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.dev = {}
        self.tables = []

    def register(self, table, form="auto", narrow=False):
        """form 'plain': no dictionaries; 'dict': every utf8 column dictionary-encoded; 'auto': the library's defaults"""
        key = (id(table), form, narrow)
        if key not in self.dev:
            lib = capi.gpu_lib()
            if form == "plain":
                lib.ldb_gpu_set_option(b"dict_encode", 0)
            try:
                t = self.ctx.register("no_%d" % len(self.dev), table, narrow_decimals=narrow)
            finally:
                lib.ldb_gpu_set_option(b"dict_encode", 1)
            for c, f in enumerate(table.schema):
                if pa.types.is_string(f.type):
                    if form == "dict":
                        if table.num_rows < 4096:
                            t.dict_encode(c)
                        assert t.dict_size(c) > 0
                    elif form == "plain":
                        assert t.dict_size(c) == -1
            self.dev[key] = t
            self.tables.append(table)  # (keeps id() unique)
        return self.dev[key]

    def close(self):
        for t in self.dev.values():
            t.release()


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.close()


def forms_of(name, table):
    """the registrations a case is run under: strings plain and dictionary-encoded (a column without a single value has no dictionary),
    decimal(12,2) also narrowed to 64 bits"""
    if "utf8" in name:
        return [("plain", False)] + ([("dict", False)] if table.column(0).null_count < table.num_rows else [])
    if name.startswith("dec12_2"):
        return [("auto", False), ("auto", True)]
    return [("auto", False)]


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


# ---------------------------------------------------------------- key types x NULL patterns x row counts x directions; bytes under a NULL; several keys
@pytest.mark.parametrize("name", SORT_CASES)
def test_sort_matches_the_comparator(world, oracle, name):
    table, specs = CASES[name]
    want = null_order_ref.expected(name)
    if "_allset_" in name:  # a validity bitmap with every bit set: no flag byte, the answer is the oracle's for the column without one
        assert np.array_equal(want, oracle.sort(HostTable(table).rel(), order_ref.sort_specs(specs)))
    for form, narrow in forms_of(name, table):
        rel = world.register(table, form, narrow).rel()
        out = rel.sort(null_order_ref.sort_specs(specs))
        assert np.array_equal(out.rowids(0), want), (form, narrow)
        for k in null_order_ref.topk_ks(name):
            top = rel.topk(null_order_ref.sort_specs(specs), k)
            assert np.array_equal(top.rowids(0), want[:k]), (form, narrow, k)
            top.release()
        out.release(), rel.release()


@pytest.mark.parametrize("ty,top", [("int64", null_order_ref.I64_MAX), ("utf8", b"\xff\xff"), ("float64", float("inf"))])
@pytest.mark.parametrize("n", [41, 4100])
def test_bytes_under_a_null_are_not_read(world, ty, top, n):
    """NULL slots hold INT64_MAX / INT64_MIN, 0xFF.. bytes and a 256-byte string, +inf / -inf / NaN: the largest valid value still sorts before
    every NULL, and the NULLs tie (the tie key, then the input position, orders them)"""
    table, specs = CASES["under_null_%s_%d_asc" % (ty, n)]
    vals = null_order_ref.column_values(table.column(0))
    ties = table.column(1).to_pylist()
    n_valid = sum(v is not None for v in vals)
    got = world.register(table, "plain" if ty == "utf8" else "auto").rel().sort(null_order_ref.sort_specs(specs)).rowids(0).tolist()
    assert all(vals[r] is not None for r in got[:n_valid]) and all(vals[r] is None for r in got[n_valid:])
    assert vals[got[n_valid - 1]] == top
    tail = [(ties[r], r) for r in got[n_valid:]]
    assert tail == sorted(tail)
    if ty == "utf8":  # NULL, b"" and b"\0" are three distinct keys, in this order from the end: NULL > b"\0" > b""
        firsts = [vals[r] for r in got[:n_valid]]
        assert firsts[0] == b"" and firsts[firsts.count(b"")] == b"\0"


def test_mixed_null_orders_and_unknown_values(world, ctx):
    table, specs = CASES["two_keys_4097"]
    rel = world.register(table).rel()
    mixed = [api.sort_spec((0, 0), False, N1), api.sort_spec((0, 1), True, capi.NULLS_REFUSE)]  # key 1 holds NULLs and refuses them
    refused(ctx, lambda: rel.sort(mixed), capi.LDB_ERR_UNSUPPORTED)
    refused(ctx, lambda: rel.topk(mixed, 5), capi.LDB_ERR_UNSUPPORTED)
    refused(ctx, lambda: rel.sort([api.sort_spec((0, 0), False, 7)]), capi.LDB_ERR_INVALID)
    refused(ctx, lambda: rel.topk([api.sort_spec((0, 0), False, N1), api.sort_spec((0, 1), False, -1)], 5), capi.LDB_ERR_INVALID)
    refused(ctx, lambda: rel.window([], [api.sort_spec((0, 0), False, 7)], [(capi.WIN_RANK, None)]), capi.LDB_ERR_INVALID)


# ---------------------------------------------------------------- top-k above 4096 rows: the radix select
@pytest.mark.parametrize("name", TOPK_CASES)
def test_topk_matches_sorted_prefix(world, name):
    table, specs = CASES[name]
    want = null_order_ref.expected(name)
    rel = world.register(table).rel()
    lib = capi.gpu_lib()
    try:
        for short in (1, 0):  # option topk_short_select: stop the select passes once the candidates fit one workgroup / run all of them
            lib.ldb_gpu_set_option(b"topk_short_select", short)
            for k in null_order_ref.topk_ks(name):
                top = rel.topk(null_order_ref.sort_specs(specs), k)
                assert top.rows == min(k, table.num_rows)
                assert np.array_equal(top.rowids(0), want[:k]), (short, k)
                top.release()
    finally:
        lib.ldb_gpu_set_option(b"topk_short_select", 1)
    rel.release()


# ---------------------------------------------------------------- outer-join padding
@pytest.fixture(scope="module")
def joined(world):
    """5000 probe rows against 600 build rows with duplicate keys; some probe keys find no partner, and some build values are NULL themselves"""
    rng = np.random.default_rng(77)
    words = [b"", b"\0", b"a", b"ab", b"\xff\xff", b"Z" * 256, b"zz", "日本".encode()]
    probe = pa.table({"k": pa.array(rng.integers(0, 500, 5000), pa.int32()), "id": pa.array(np.arange(5000, dtype=np.int32))})
    build = pa.table({
        "k": pa.array(rng.integers(0, 400, 600), pa.int32()),
        "i": null_order_ref.with_validity(pa.array(rng.integers(-(2 ** 31), 2 ** 31, 600), pa.int32()), rng.random(600) >= 0.2),
        "d": null_order_ref.with_validity(order_ref.dec_array([int(v) * 2 ** 64 for v in rng.integers(-3, 4, 600)], 38, 0), rng.random(600) >= 0.2),
        "s": null_order_ref.with_validity(order_ref.str_array([words[i] for i in rng.integers(0, len(words), 600)]), rng.random(600) >= 0.2),
    })
    gp, gb = world.register(probe), world.register(build, "plain")
    out = gb.rel().join_build([(0, 0)]).probe(gp.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    p, b = out.rowids(0), out.rowids(1)  # side 0 = probe rows, side 1 = build rows; the pairs as the device wrote them are the input order
    assert (b == NULL_ROW).any() and len(p) > 4096
    return probe, build, out, p, b


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("col", [1, 2, 3], ids=["int32", "dec38_0", "utf8"])
def test_sort_and_topk_by_a_padded_side_column(joined, col, desc):
    """both sources of NULL meet in one key: padding row ids and cleared validity bits.  The utf8 column is the one whose pad-length pre-check
    used to read the offsets of the padding row id."""
    probe, build, out, p, b = joined
    specs = [api.sort_spec((1, col), desc, N1), api.sort_spec((0, 1), False, N1)]
    perm = null_order_ref.sort_rel([(probe, p), (build, b)], len(p), [(1, col, desc), (0, 1, False)])
    s = out.sort(specs)
    assert np.array_equal(s.rowids(0), p[perm]) and np.array_equal(s.rowids(1), b[perm])
    for k in (1, 100, 4097):
        t = out.topk(specs, k)
        assert np.array_equal(t.rowids(0), p[perm][:k]) and np.array_equal(t.rowids(1), b[perm][:k]), k
        t.release()
    s.release()


# ---------------------------------------------------------------- window
def test_window_over_nullable_partition_and_order_keys(world):
    n = 5000
    rng = np.random.default_rng(12)
    part = [None if v == 5 else int(v) for v in rng.integers(0, 6, n)]  # five values + NULL
    order = [None if rng.random() < 0.25 else int(v) for v in rng.integers(-40, 40, n)]
    table = pa.table({"p": pa.array(part, pa.int32()), "o": pa.array(order, pa.int64())})
    rel, cols = world.register(table).rel().window([(0, 0)], [api.sort_spec((0, 1), True, N1)], [(capi.WIN_RANK, None), (capi.WIN_COUNT_STAR, None)])
    want = null_order_ref.sort(table, [(0, False), (1, True)])  # the NULL partition last; inside a partition the NULLs first
    got = rel.rowids(0)
    assert np.array_equal(got, want)
    assert part[got[-1]] is None and order[got[0]] is None
    rank, seen = [], {}
    for r in want:
        seen[part[r]] = seen.get(part[r], 0) + 1
        rank.append(seen[part[r]])
    res = cols.to_arrow()
    assert res.column(0).to_pylist() == rank  # row-number semantics, as in the reference
    assert res.column(1).to_pylist() == rank  # default frame: partition begin .. current row
    # without the NULL order on the ORDER BY key the refusal stays
    with pytest.raises(capi.LdbError) as e:
        world.register(table).rel().window([(0, 0)], [api.sort_spec((0, 1), True)], [(capi.WIN_RANK, None)])
    assert e.value.status == capi.LDB_ERR_UNSUPPORTED


# ---------------------------------------------------------------- plan: recorded once, replayed twice
def test_plan_sorts_by_a_right_side_column_after_a_left_outer_join(world, ctx):
    rng = np.random.default_rng(3)
    n_probe, n_build = 5000, 400
    words = [b"", b"b", b"a", b"\xff", b"ab", b"a\0"]
    probe = pa.table({"pk": pa.array(rng.integers(0, 600, n_probe), pa.int32()), "pid": pa.array(np.arange(n_probe, dtype=np.int32))})
    build = pa.table({
        "bk": pa.array(rng.permutation(600)[:n_build].astype(np.int32)),  # unique keys: at most one partner, so the pair order is the probe order
        "bid": pa.array(np.arange(n_build, dtype=np.int32)),
        "bv": null_order_ref.with_validity(pa.array(rng.integers(-5, 6, n_build), pa.int64()), rng.random(n_build) >= 0.3),
        "bs": null_order_ref.with_validity(order_ref.str_array([words[i] for i in rng.integers(0, len(words), n_build)]), rng.random(n_build) >= 0.3),
    })
    k = 4500
    plan = {"steps": [{"op": "join_build", "in": "b", "keys": ["bk"], "out": "h"},
                      {"op": "join_probe", "ht": "h", "in": "p", "keys": ["pk"], "kind": "left_outer", "out": "j"},
                      {"op": "sort", "in": "j", "by": [{"col": "bv", "desc": True}, "pid"], "out": "s"},
                      {"op": "topk", "in": "s", "by": ["bs"], "k": k, "out": "top"},
                      {"op": "materialize", "in": "top", "cols": ["pid", "bid"], "out": "result"}], "result": "result"}
    # reference: the join by hand, then the two orders
    partner = {int(key): i for i, key in enumerate(build.column(0).to_pylist())}
    b = np.array([partner.get(int(key), NULL_ROW) for key in probe.column(0).to_pylist()], dtype=np.uint32)
    p = np.arange(n_probe, dtype=np.uint32)
    assert (b == NULL_ROW).any()
    first = null_order_ref.sort_rel([(probe, p), (build, b)], n_probe, [(1, 2, True), (0, 1, False)])
    p1, b1 = p[first], b[first]
    second = null_order_ref.sort_rel([(probe, p1), (build, b1)], n_probe, [(1, 3, False)])[:k]  # ties keep the first sort's order
    want_pid = p1[second].tolist()
    want_bid = [None if r == NULL_ROW else int(r) for r in b1[second]]
    assert None in want_bid and want_bid[0] is not None
    tables = {"p": world.register(probe), "b": world.register(build, "plain")}
    prepared = ctx.prepare_plan(json.dumps(plan))
    for run in range(3):  # the recording execution, then two replays of its read-backs (the per-key NULL word among them)
        res = prepared.execute(tables).to_arrow()
        assert res.column(0).to_pylist() == want_pid, run
        assert res.column(1).to_pylist() == want_bid, run
    stats = prepared.stats()
    assert stats["executions"] == 3 and stats["replays"] >= 1, stats
    prepared.release()


# ---------------------------------------------------------------- the reference's own ORDER BY cases
@pytest.mark.parametrize("case", FIXTURE, ids=[c["source"].rsplit(":", 1)[1] for c in FIXTURE])
def test_reference_suite_cases(ctx, case):
    n = len(case["expected"])
    rng = np.random.default_rng(n + 1)
    for order in (list(range(n)), list(range(n))[::-1], rng.permutation(n).tolist()):
        key = [case["expected"][i][0] for i in order]
        arr = order_ref.str_array([v.encode() if v is not None else b"" for v in key]) if case["key_type"] == "utf8" else pa.array([v or 0 for v in key], pa.int32())
        table = pa.table({"key": null_order_ref.with_validity(arr, [v is not None for v in key])})
        t = ctx.register("no_fixture", table)
        specs = [api.sort_spec((0, 0), False, N1)]
        rel = t.rel().sort(specs) if case["limit"] is None else t.rel().topk(specs, case["limit"])
        assert [order[r] for r in rel.rowids(0)] == list(range(n)), order  # distinct keys: the expected order is the only one
        rel.release(), t.release()
