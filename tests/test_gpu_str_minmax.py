"""MIN / MAX over utf8 columns in ldb_gpu_groupby (csrc/ldb_strminmax.hip; the aggregate of every Join Order Benchmark query).
Expected values are Python's own: min / max over bytes objects is std::string_view order — unsigned bytes, then length —
which is what the reference's StringRuntime::compareLt / compareGt evaluate.  Every comparison is exact equality."""
import collections
import json

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

A40 = b"0123456789abcdefghijklmnopqrstuvw" + b"A" + b"yz!+-*"  # 40 bytes; the next one differs in byte 33 only
B40 = b"0123456789abcdefghijklmnopqrstuvw" + b"B" + b"yz!+-*"
POOL = [b"", b"a", b"ab", b"ab\0", b"abc", b"exactly8", A40, B40, b"L" * 300, "é…".encode(), b"\xff", b"z", b"exactly8 and more", b"exactly"]
assert len(A40) == len(B40) == 40 and A40[:33] == B40[:33] and A40[33] != B40[33]


def str_array(vals, large=False):
    """utf8 column from bytes objects without validation (the order is bytewise: 0xff must sort above every character)"""
    return pa.array(vals, pa.large_binary() if large else pa.binary()).view(pa.large_string() if large else pa.string())


def raw(col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return col.view(pa.large_binary() if pa.types.is_large_string(col.type) else pa.binary()).to_pylist()


def pool_values(n, seed=3, null_every=9, long=True):
    """long=False: the 300-byte string shrinks to 200 bytes (the dictionary encoder sorts the distinct strings: at most 256 bytes each)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(POOL), n).tolist()
    pool = POOL if long else [p[:200] for p in POOL]
    return [None if null_every and i % null_every == 4 else pool[k] for i, k in enumerate(idx)]


def register(ctx, name, table, dict_encode):
    lib = capi.gpu_lib()
    lib.ldb_gpu_set_option(b"dict_encode", 0)
    try:
        t = ctx.register(name, table)
    finally:
        lib.ldb_gpu_set_option(b"dict_encode", 1)
    for c in dict_encode:
        assert t.dict_encode(c) > 0
    return t


def minmax(rel, col, plist=()):
    got = rel.groupby([], [api.str_minmax(capi.AGG_MIN, col), api.str_minmax(capi.AGG_MAX, col)], plist).to_arrow()
    assert got.num_rows == 1 and got.num_columns == 2
    assert pa.types.is_string(got.schema.field(0).type) and pa.types.is_string(got.schema.field(1).type)
    return raw(got.column(0))[0], raw(got.column(1))[0]


def want(vals):
    nn = [v for v in vals if v is not None]
    return (min(nn), max(nn)) if nn else (None, None)


def test_pool_order_is_the_reference_order():
    assert b"" < b"a" < b"ab" < b"ab\0" < b"abc" < b"z" < "é…".encode() < b"\xff" and min(POOL) == b"" and max(POOL) == b"\xff" and A40 < B40


@pytest.mark.parametrize("use_dict", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 70_001])
def test_keyless_min_and_max_row_counts(ctx, n, use_dict):
    vals = pool_values(n, seed=n + 1, long=not use_dict)
    t = register(ctx, "smm_n", pa.table({"s": str_array(vals)}), [0] if use_dict and any(v is not None for v in vals) else [])
    assert minmax(t.rel(), (0, 0)) == want(vals)
    t.release()


def test_keyless_targeted_inputs(ctx):
    rng = np.random.default_rng(11)
    cases = {"equal": [b"same string"] * 1000, "nulls": [None] * 1000, "one": [None] * 999 + [b"only"],
             "prefix12": [b"twelve bytes" + bytes(rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8).tolist()) for _ in range(5000)],
             "nul_tail": [b"ab\0", b"ab", b"ab\0\0", b"ab"] * 300}
    for name, vals in cases.items():
        t = register(ctx, "smm_" + name, pa.table({"s": str_array(vals)}), [])
        assert minmax(t.rel(), (0, 0)) == want(vals), name
        t.release()
    vals = pool_values(3000, seed=5)
    t = register(ctx, "smm_large", pa.table({"s": str_array(vals, large=True)}), [])
    assert minmax(t.rel(), (0, 0)) == want(vals)
    t.release()


@pytest.fixture(scope="module")
def base(ctx):
    n = 20_000
    vals = pool_values(n, seed=21, long=False)
    rng = np.random.default_rng(22)
    k = rng.integers(0, 100, n).astype(np.int32)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    tab = pa.table({"s": str_array(vals), "k": pa.array(k), "v": pa.array(v)})
    plain = register(ctx, "smm_base", tab, [])
    enc = register(ctx, "smm_base_dict", tab, [0])
    return vals, k, v, plain, enc


@pytest.mark.parametrize("which", ["plain", "dict"])
def test_keyless_relation_shapes(ctx, base, which):
    vals, k, v, plain, enc = base
    t = plain if which == "plain" else enc
    sub = [s for s, kk in zip(vals, k.tolist()) if kk < 30]
    p = lambda: [api.pred((0, 1), capi.F_LT, 30)]  # noqa: E731
    assert minmax(t.rel().scan_filter(p()), (0, 0)) == want(sub)
    assert minmax(t.rel(), (0, 0), p()) == want(sub)
    assert minmax(t.rel(), (0, 0), [api.pred((0, 1), capi.F_LT, -1)]) == (None, None)  # nothing passes: one NULL row
    lib = capi.gpu_lib()
    lib.ldb_gpu_set_option(b"lazy_filter", 1)
    lib.ldb_gpu_set_option(b"lazy_min_rows", 0)
    try:
        assert minmax(t.rel().scan_filter(p()), (0, 0)) == want(sub)
    finally:
        lib.ldb_gpu_set_option(b"lazy_min_rows", 1 << 20)


def test_keyless_over_outer_join_padding(ctx, base):
    vals, k, v, plain, enc = base
    # probe keys 0 … 149 against the build rows' k (0 … 99): LEFT OUTER keeps unmatched probe rows with LDB_NULL_ROW on the build side
    probe = ctx.register("smm_probe", pa.table({"k": pa.array(np.arange(150, dtype=np.int32))}))
    small = register(ctx, "smm_build", pa.table({"s": str_array(vals[:60]), "k": pa.array(k[:60])}), [])
    out = small.rel().join_build([(0, 1)]).probe(probe.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    assert 0xFFFFFFFF in out.rowids(1).tolist()
    assert minmax(out, (1, 0)) == want(vals[:60])
    none = small.rel().join_build([(0, 1)]).probe(ctx.register("smm_probe2", pa.table({"k": pa.array(np.arange(500, 520, dtype=np.int32))})).rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    assert none.rows == 20 and minmax(none, (1, 0)) == (None, None)  # every build-side row is padding


def test_keyless_over_a_lazy_dictionary_column(ctx, base):
    vals, k, v, plain, enc = base
    mat = enc.rel().scan_filter([api.pred((0, 1), capi.F_GTE, 10)]).materialize([(0, 0), (0, 1)])  # >= 4096 rows: codes + dictionary, no bytes
    sub = [s for s, kk in zip(vals, k.tolist()) if kk >= 10]
    assert mat.dict_size(0) > 0
    assert minmax(mat.rel(), (0, 0)) == want(sub)
    assert raw(mat.to_arrow().column(0)) == sub  # (and the column is still what it was)


def test_mixed_aggregates_keep_their_order(ctx, base):
    vals, k, v, plain, enc = base
    D = capi.T_DECIMAL128
    dec = ctx.register("smm_dec", pa.table({"s": str_array(vals), "v": pa.array(v), "m": pa.array([None if i % 5 == 0 else __import__("decimal").Decimal(int(x)).scaleb(-2) for i, x in enumerate(v)],
                                                                                                     pa.decimal128(12, 2))}))
    aggs = [api.agg(capi.AGG_COUNT_STAR), api.agg(capi.AGG_SUM, api.col_expr((0, 1))), api.str_minmax(capi.AGG_MIN, (0, 0)), api.str_minmax(capi.AGG_MAX, (0, 0)),
            api.agg(capi.AGG_MIN, api.col_expr((0, 2)), out_type=D, p=12, s=2)]
    got = dec.rel().groupby([], aggs).to_arrow()
    assert got.num_rows == 1 and got.column_names == ["agg0", "agg1", "agg2", "agg3", "agg4"]
    lo, hi = want(vals)
    assert got.column(0)[0].as_py() == len(vals) and got.column(1)[0].as_py() == int(v.sum())
    assert raw(got.column(2)) == [lo] and raw(got.column(3)) == [hi]
    assert int(got.column(4)[0].as_py().scaleb(2)) == min(int(x) for i, x in enumerate(v) if i % 5)


@pytest.mark.parametrize("keys", ["few", "sorted", "random"])
def test_grouped_min_max_over_a_dictionary(ctx, keys):
    n = 20_000
    rng = np.random.default_rng(31)
    words = [("w%02d" % i).encode() * (1 + i % 4) for i in range(35)] + [b"", b"\xff"]
    assert len(set(words)) == 37
    if keys == "few":
        k = rng.integers(0, 7, n).astype(np.int64)
    elif keys == "sorted":
        k = np.sort(rng.integers(0, 5000, n)).astype(np.int64)
    else:
        k = rng.integers(0, 1 << 40, 4000)[rng.integers(0, 4000, n)].astype(np.int64)
    null_group = int(k[0])
    s = [None if (i % 11 == 2 or int(kk) == null_group) else words[j] for i, (kk, j) in enumerate(zip(k.tolist(), rng.integers(0, 37, n).tolist()))]
    t = register(ctx, "smm_grouped", pa.table({"k": pa.array(k), "s": str_array(s)}), [1])
    got = t.rel().groupby([(0, 0)], [api.str_minmax(capi.AGG_MIN, (0, 1)), api.str_minmax(capi.AGG_MAX, (0, 1)), api.agg(capi.AGG_COUNT_STAR)], est_groups=len(set(k.tolist()))).to_arrow()
    per = collections.defaultdict(list)
    for kk, x in zip(k.tolist(), s):
        per[kk].append(x)
    have = {kk: (lo, hi, c) for kk, lo, hi, c in zip(got.column(0).to_pylist(), raw(got.column(1)), raw(got.column(2)), got.column(3).to_pylist())}
    assert have == {kk: want(xs) + (len(xs),) for kk, xs in per.items()}
    assert have[null_group][:2] == (None, None)
    t.release()


def held(ctx):
    st = ctx.desc_cache_stats()
    return st["held"], st["underflows"]


def test_refusals(ctx, base):
    vals, k, v, plain, enc = base
    f = api.factor

    def status(rel, keys, aggs):
        with pytest.raises(capi.LdbError) as e:
            rel.groupby(keys, aggs)
        assert held(ctx) == (0, 0)
        return e.value.status, str(e.value)

    st, msg = status(plain.rel(), [(0, 1)], [api.str_minmax(capi.AGG_MIN, (0, 0))])
    assert st == capi.LDB_ERR_UNSUPPORTED and "grouped MIN / MAX over a string column without a dictionary" in msg
    assert status(plain.rel(), [], [api.agg(capi.AGG_MIN, api.col_expr((0, 0)), out_type=capi.T_INT64)])[0] == capi.LDB_ERR_INVALID
    assert status(plain.rel(), [], [api.agg(capi.AGG_MIN, api.col_expr((0, 2)), out_type=capi.T_UTF8)])[0] == capi.LDB_ERR_INVALID
    two = api.expr([{"factors": [f(0, 1, (0, 0)), f(0, 1, (0, 2))]}])
    assert status(plain.rel(), [], [api.agg(capi.AGG_MIN, two, out_type=capi.T_UTF8)])[0] == capi.LDB_ERR_UNSUPPORTED
    assert status(plain.rel(), [], [api.agg(capi.AGG_SUM, api.col_expr((0, 0)), out_type=capi.T_UTF8)])[0] == capi.LDB_ERR_UNSUPPORTED
    cond = api.agg(capi.AGG_MAX, api.col_expr((0, 0)), out_type=capi.T_UTF8, preds=[api.pred((0, 1), capi.F_LT, 5)])
    assert status(plain.rel(), [], [cond])[0] == capi.LDB_ERR_UNSUPPORTED
    assert status(enc.rel(), [(0, 1)], [cond])[0] == capi.LDB_ERR_UNSUPPORTED


def test_plan_step_and_prepared_replay(ctx, base):
    vals, k, v, plain, enc = base
    sub = [s for s, kk in zip(vals, k.tolist()) if kk >= 50]
    plan = json.dumps({"name": "str_minmax", "inputs": ["t"], "steps": [
        {"op": "groupby", "in": "t", "keys": [], "preds": [{"col": "k", "op": "GTE", "value": 50}],
         "aggs": [{"fn": "min", "expr": "s", "as": "lo"}, {"fn": "max", "expr": "s", "as": "hi"}, {"fn": "count_star", "as": "n"}], "est_groups": 1, "out": "r"}], "result": "r"})
    for t in (plain, enc):
        prepared = ctx.prepare_plan(plan)
        for _ in range(3):
            got = prepared.execute({"t": t}).to_arrow()
            assert got.column_names == ["lo", "hi", "n"]
            assert (raw(got.column(0))[0], raw(got.column(1))[0]) == want(sub) and got.column(2)[0].as_py() == len(sub)
        st = prepared.stats()
        assert st["replays"] >= 1 and st["misses"] == 0, st
        prepared.release()
    bad = json.dumps({"name": "bad", "inputs": ["t"], "steps": [{"op": "groupby", "in": "t", "keys": [], "aggs": [{"fn": "min", "expr": {"mul": ["s", "v"]}}], "out": "r"}], "result": "r"})
    with pytest.raises(capi.LdbError, match="string column"):
        ctx.run_plan(bad, {"t": plain})


def test_two_level_min_equals_one_level(ctx, base):
    """per-slice MIN / MAX, the partial rows concatenated, MIN / MAX again: what the sharded plan does after its allgather"""
    vals, k, v, plain, enc = base
    parts = []
    for lo in (0, 40, 80):
        r = plain.rel().groupby([], [api.str_minmax(capi.AGG_MIN, (0, 0)), api.str_minmax(capi.AGG_MAX, (0, 0))], [api.pred((0, 1), capi.F_GTE, lo), api.pred((0, 1), capi.F_LT, lo + 40)])
        parts.append(r.to_arrow())
    parts.append(plain.rel().groupby([], [api.str_minmax(capi.AGG_MIN, (0, 0)), api.str_minmax(capi.AGG_MAX, (0, 0))], [api.pred((0, 1), capi.F_LT, -5)]).to_arrow())  # an empty slice: NULLs
    both = ctx.register("smm_partials", pa.concat_tables(parts))
    got = both.rel().groupby([], [api.str_minmax(capi.AGG_MIN, (0, 0)), api.str_minmax(capi.AGG_MAX, (0, 1))]).to_arrow()
    assert (raw(got.column(0))[0], raw(got.column(1))[0]) == want(vals)


def test_job_17a_plan_file_prepared(ctx):
    """plans/job/17a.json over a seven-table toy schema; the expected row is the SQL read in Python: MIN(n.name) over the cast rows of people whose
    name starts with B, in movies that exist in title, carry the keyword 'character-name-in-title' and have a company with country code '[us]'"""
    rng = np.random.default_rng(17)
    i32 = lambda a: pa.array(np.asarray(a, dtype=np.int32))  # noqa: E731
    kw = ["kw%02d" % i for i in range(50)]
    kw[7] = "character-name-in-title"
    cc = ["[us]" if i % 3 == 0 else "[de]" for i in range(100)]
    t_id = [i for i in range(400) if i % 10 != 3]
    n_name = ["%s%s %05d" % ("ABCb"[int(a)], "aeiou"[int(b)], int(c)) for a, b, c in zip(rng.integers(0, 4, 1000), rng.integers(0, 5, 1000), rng.integers(0, 100000, 1000))]
    mk_m, mk_k = rng.integers(0, 400, 3000), rng.integers(0, 50, 3000)
    mc_m, mc_c = rng.integers(0, 400, 2000), rng.integers(0, 100, 2000)
    ci_p, ci_m = rng.integers(0, 1000, 5000), rng.integers(0, 400, 5000)
    tabs = {"keyword": pa.table({"k_id": i32(range(50)), "k_keyword": pa.array(kw)}),
            "company_name": pa.table({"cn_id": i32(range(100)), "cn_country_code": pa.array(cc)}),
            "title": pa.table({"t_id": i32(t_id)}),
            "name": pa.table({"n_id": i32(range(1000)), "n_name": pa.array(n_name)}),
            "movie_keyword": pa.table({"mk_movie_id": i32(mk_m), "mk_keyword_id": i32(mk_k)}),
            "movie_companies": pa.table({"mc_movie_id": i32(mc_m), "mc_company_id": i32(mc_c)}),
            "cast_info": pa.table({"ci_person_id": i32(ci_p), "ci_movie_id": i32(ci_m)})}
    movies = {int(m) for m, k in zip(mk_m, mk_k) if k == 7} & set(t_id) & {int(m) for m, c in zip(mc_m, mc_c) if cc[int(c)] == "[us]"}
    names = [n_name[int(p)].encode() for p, m in zip(ci_p, ci_m) if int(m) in movies and n_name[int(p)].startswith("B")]
    assert len(names) > 20 and len(movies) > 5
    regs = {n: ctx.register("job_" + n, t) for n, t in tabs.items()}
    prepared = ctx.prepare_plan("job/17a.json")
    for _ in range(3):
        got = prepared.execute(regs).to_arrow()
        assert got.num_rows == 1 and got.column_names == ["member_in_charnamed_american_movie", "a1"]
        assert raw(got.column(0)) == [min(names)] and raw(got.column(1)) == [min(names)]
    st = prepared.stats()
    assert st["replays"] >= 1 and st["misses"] == 0, st
    prepared.release()
    for t in regs.values():
        t.release()


def test_string_reduce_dump_runs_on_the_device(ctx):
    """SELECT MIN(n_name), MAX(n_name) FROM nation from the reference's sub-operator dump: translator → plan interpreter → the string reduction"""
    import test_str_minmax_api as cpu_half

    names = [b"PERU", b"ALGERIA", None, b"VIETNAM", b"ALGERIA ", b"ZAMBIA\xc3\xa9", b"", b"Z"] * 5
    t = ctx.register("nation_smm", pa.table({"n_nationkey": pa.array(np.arange(len(names), dtype=np.int32)), "n_name": str_array(names)}))
    got = ctx.run_subop_dump(cpu_half._string_reduce_dump(), {"nation": t}).to_arrow()
    assert got.num_rows == 1 and (raw(got.column(0))[0], raw(got.column(1))[0]) == want(names)
    t.release()
