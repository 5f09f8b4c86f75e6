"""String IN lists and string constants of any size in scans (csrc/ldb_strset.hip behind ldb_gpu_scan_filter / _count / the `preds` of
ldb_gpu_groupby, the plan language, the sub-operator translator, the dictionary path).  Expected rows are Python's own: set membership of
bytes objects, and comparison of bytes objects — unsigned bytes, then length, the reference's std::string_view order.  Every comparison is
exact equality of ascending row-id lists.  One fixture (tests/golden/ref_long_in.json) holds what the reference's own Restrictions answered."""
import gc
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

LDS_MAX = 5376  # constants a workgroup stages in LDS (tests/test_strset_api.py pins it against the library)
P12 = b"twelve bytes"
SHARED = [P12 + b"%02d" % i + b"x" * (i % 5) for i in range(40)]  # 40 constants sharing a 12-byte prefix
NEAR = [P12, P12 + b"00x", P12 + b"0", P12 + b"99xxxx", P12 + b"07xx!", P12 + b"\xff"]  # rows that match the prefix and no constant
LENGTHS = [b"", b"1", b"seven77", b"exactly8", b"nine char", b"sixteen bytes 16", b"seventeen bytes 7", b"L" * 200]
assert [len(c) for c in LENGTHS] == [0, 1, 7, 8, 9, 16, 17, 200] and not set(NEAR) & set(SHARED)
PREFIXES = [b"a", b"ab", b"ab\0", b"ab\0\0", b"abc", b"abcdefgh", b"abcdefghi", b"abcdefghij"]
HIGH = ["é…".encode(), b"\xff", b"\xff\xfe", b"\x80abc", "日本語のタイトル".encode()]
OTHERS = [b"b", b"abd", b"abcdefgh\0", b"abcdefghik", b"exactly9", b"nine chars", b"sixteen bytes 61", b"L" * 199, b"L" * 201, b"\xfe", b"z" * 30]


def str_array(vals):
    """utf8 column from bytes objects without validation (bytes >= 0x80 that are no UTF-8 must stay as they are)"""
    return pa.array(vals, pa.binary()).view(pa.string())


def register(ctx, name, table, dict_encode=()):
    lib = capi.gpu_lib()
    lib.ldb_gpu_set_option(b"dict_encode", 0)
    try:
        t = ctx.register(name, table)
    finally:
        lib.ldb_gpu_set_option(b"dict_encode", 1)
    for c in dict_encode:
        assert t.dict_encode(c) > 0
    return t


def in_pred(col, consts):
    d, keep = api.pred(col, capi.F_IN, values=list(consts))
    d.rhs_kind = capi.RHS_STRING  # (an empty list carries no type of its own)
    return d, keep


def rows_of(rel, side=0):
    return rel.rowids(side).tolist()


def want_in(vals, consts):
    s = set(consts)
    return [i for i, v in enumerate(vals) if v is not None and v in s]


def column_values(n, consts, seed, null_every=0):
    """members and near misses in equal parts"""
    rng = np.random.default_rng(seed)
    pool = list(consts) + OTHERS + NEAR + PREFIXES
    idx = rng.integers(0, len(pool), n).tolist()
    return [None if null_every and i % null_every == 3 else pool[k] for i, k in enumerate(idx)]


class option:
    def __init__(self, name, value, restore):
        self.name, self.value, self.restore = name, value, restore

    def __enter__(self):
        capi.gpu_lib().ldb_gpu_set_option(self.name, self.value)

    def __exit__(self, *exc):
        capi.gpu_lib().ldb_gpu_set_option(self.name, self.restore)


NINE = [b"ALGERIA", b"BRAZIL", b"CANADA", b"", b"UNITED KINGDOM", b"UNITED STATES", b"a", b"ab\0", b"exactly8"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 16_383, 16_384, 16_385, 70_001])
def test_row_counts(ctx, n):
    vals = column_values(n, NINE, seed=n + 7, null_every=11)
    t = register(ctx, "ss_n", pa.table({"s": str_array(vals)}))
    want = want_in(vals, NINE)
    assert rows_of(t.rel().scan_filter([in_pred((0, 0), NINE)])) == want
    assert t.rel().scan_count([in_pred((0, 0), NINE)]) == len(want)
    with option(b"scan_split", 0, 1):  # one workgroup per 16 384 rows instead of the split of a short input
        assert rows_of(t.rel().scan_filter([in_pred((0, 0), NINE)])) == want
    t.release()


def many(k, width=5):
    return [b"c%0*d" % (width, 7 * i) for i in range(k)]


CONSTANT_CASES = {
    "nine": NINE,
    "sixty_four": many(64),
    "thousand": many(1000) + LENGTHS,
    "lds_full": many(LDS_MAX),
    "lds_plus_one": many(LDS_MAX + 1),  # the search over global memory
    "lengths": LENGTHS + [b"pad"],
    "shared_prefix": SHARED,
    "prefixes": PREFIXES + [b"pad"],
    "duplicates": NINE + NINE[:4] + [b"BRAZIL"] * 5,
    "high_bytes": HIGH + [b"a", b"b", b"c", b"d"],
    "few_but_long": [b"A" * 60, b"A" * 61, b"B" * 40],  # 3 constants, 161 bytes: over the inline blob
}


@pytest.mark.parametrize("case", list(CONSTANT_CASES))
def test_constants(ctx, case):
    consts = CONSTANT_CASES[case]
    n = 20_000
    vals = column_values(n, consts, seed=len(consts), null_every=13)
    if case in ("lds_full", "lds_plus_one"):  # every constant appears: the last one and the first one too
        vals[:len(consts)] = consts
        vals[7] = None
    t = register(ctx, "ss_c", pa.table({"s": str_array(vals)}))
    want = want_in(vals, consts)
    assert 0 < len(want) < n
    ctx.prof_enable(True)
    ctx.prof_reset()
    got = rows_of(t.rel().scan_filter([in_pred((0, 0), consts)]))
    prof = ctx.prof_all()
    ctx.prof_enable(False)
    assert got == want
    kernel = "k_strset_bitmap_glb" if len(set(consts)) > LDS_MAX else "k_strset_bitmap_lds"
    assert prof.get(kernel, (0, 0.0))[0] == 1 and "k_scan_bitmap" not in prof, prof
    t.release()


def test_empty_list_passes_nothing(ctx):
    vals = column_values(1000, NINE, seed=1)
    t = register(ctx, "ss_empty", pa.table({"s": str_array(vals)}))
    assert rows_of(t.rel().scan_filter([in_pred((0, 0), [])])) == []
    with option(b"scan_strset_min_in", 0, 9):
        assert rows_of(t.rel().scan_filter([in_pred((0, 0), [])])) == []
        assert t.rel().scan_count([in_pred((0, 0), [])]) == 0
    t.release()


@pytest.fixture(scope="module")
def base(ctx):
    n = 20_000
    consts = many(12) + [b"", b"ab\0"]
    vals = column_values(n, consts, seed=77, null_every=9)
    assert sum(v is None for v in vals) > 1000 and len(consts) == 14  # a nullable column with NULLs under every test that uses this fixture
    rng = np.random.default_rng(78)
    k = rng.integers(0, 100, n).astype(np.int32)
    words = [b"forest green", b"dark green lace", b"red", b"blue lace", b"green"]
    w = [words[j] for j in rng.integers(0, len(words), n)]
    cols = {"s": str_array(vals), "k": pa.array(k), "w": str_array(w)}
    cols.update({"c%d" % i: pa.array(rng.integers(0, 100, n).astype(np.int32)) for i in range(9)})
    cols["i"] = pa.array(np.arange(n, dtype=np.int64))
    tab = pa.table(cols)
    plain = register(ctx, "ss_base", tab)
    enc = register(ctx, "ss_base_dict", tab, [0])
    return {"vals": vals, "k": k, "w": w, "consts": consts, "tab": tab, "plain": plain, "enc": enc, "words": words}


def test_through_row_ids_after_a_filter_and_a_join(ctx, base):
    vals, k, consts, plain = base["vals"], base["k"], base["consts"], base["plain"]
    f = plain.rel().scan_filter([api.pred((0, 1), capi.F_LT, 40)])
    got = rows_of(f.scan_filter([in_pred((0, 0), consts)]))
    assert got == [i for i in want_in(vals, consts) if k[i] < 40] and len(got) > 100
    probe = ctx.register("ss_probe", pa.table({"k": pa.array(np.arange(150, dtype=np.int32))}))
    small = register(ctx, "ss_build", pa.table({"s": str_array(vals[:300]), "k": pa.array(k[:300])}))
    out = small.rel().join_build([(0, 1)]).probe(probe.rel(), [(0, 0)], capi.JOIN_INNER)
    pr, br = out.rowids(0).tolist(), out.rowids(1).tolist()
    hit = out.scan_filter([in_pred((1, 0), consts)])
    member = set(consts)
    keep = [j for j, b in enumerate(br) if vals[b] is not None and vals[b] in member]
    assert 0 < len(keep) < len(br)
    assert hit.rowids(0).tolist() == [pr[j] for j in keep] and hit.rowids(1).tolist() == [br[j] for j in keep]


def test_over_outer_join_padding(ctx, base):
    vals, k, consts = base["vals"], base["k"], base["consts"]
    probe = ctx.register("ss_probe_o", pa.table({"k": pa.array(np.arange(150, dtype=np.int32))}))
    small = register(ctx, "ss_build_o", pa.table({"s": str_array(vals[:60]), "k": pa.array(k[:60])}))
    out = small.rel().join_build([(0, 1)]).probe(probe.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    pr, br = out.rowids(0).tolist(), out.rowids(1).tolist()
    assert 0xFFFFFFFF in br
    member = set(consts)
    keep = [j for j, b in enumerate(br) if b != 0xFFFFFFFF and vals[b] is not None and vals[b] in member]
    hit = out.scan_filter([in_pred((1, 0), consts)])
    assert len(keep) > 0 and hit.rowids(1).tolist() == [br[j] for j in keep] and hit.rowids(0).tolist() == [pr[j] for j in keep]
    long_c = b"c00007" + b"!" * 60  # a comparison: padding fails NEQ too
    neq = out.scan_filter([api.pred((1, 0), capi.F_NEQ, long_c)])
    assert neq.rowids(1).tolist() == [b for b in br if b != 0xFFFFFFFF and vals[b] is not None]


def test_dictionary_column_and_lazy_dictionary_column(ctx, base):
    vals, k, enc = base["vals"], base["k"], base["enc"]
    twelve = many(12)
    assert enc.dict_size(0) > 0
    assert rows_of(enc.rel().scan_filter([in_pred((0, 0), twelve)])) == want_in(vals, twelve)
    other = many(12)[:11] + [b"ab\0"]  # a second long list over the same dictionary: not the first one's cached code set
    assert rows_of(enc.rel().scan_filter([in_pred((0, 0), other)])) == want_in(vals, other) != want_in(vals, twelve)
    long_c = b"c00035" + b"z" * 50
    assert rows_of(enc.rel().scan_filter([api.pred((0, 0), capi.F_LT, long_c)])) == [i for i, v in enumerate(vals) if v is not None and v < long_c]
    mat = enc.rel().scan_filter([api.pred((0, 1), capi.F_GTE, 10)]).materialize([(0, 0), (0, 1)])  # >= 4096 rows: codes + dictionary, no bytes
    sub = [s for s, kk in zip(vals, k.tolist()) if kk >= 10]
    assert mat.dict_size(0) > 0
    assert rows_of(mat.rel().scan_filter([in_pred((0, 0), twelve)])) == want_in(sub, twelve)


def test_conjunctions_counts_and_groupby(ctx, base):
    vals, k, w, consts, plain = base["vals"], base["k"], base["w"], base["consts"], base["plain"]
    colors = [x for x in base["words"] if b"green" in x] + [b"no such %d" % i for i in range(9)]
    plist = lambda: [api.pred((0, 1), capi.F_GTE, 20), in_pred((0, 0), consts), api.pred((0, 2), capi.F_LIKE, b"%green%"), api.pred((0, 1), capi.F_LT, 90)]  # noqa: E731
    want = [i for i in want_in(vals, consts) if 20 <= k[i] < 90 and b"green" in w[i]]
    assert len(want) > 50
    assert rows_of(plain.rel().scan_filter(plist())) == want
    assert plain.rel().scan_count(plist()) == len(want)
    two = lambda: [in_pred((0, 0), consts), in_pred((0, 2), colors)]  # noqa: E731
    want2 = [i for i in want_in(vals, consts) if w[i] in set(colors)]
    assert rows_of(plain.rel().scan_filter(two())) == want2 and len(want2) > 50
    assert plain.rel().scan_count(two()) == len(want2)
    aggs = lambda: [api.agg(capi.AGG_COUNT_STAR), api.agg(capi.AGG_SUM, api.col_expr((0, 1)))]  # noqa: E731
    for keys in ([(0, 1)], []):
        a = plain.rel().groupby(keys, aggs(), plist(), est_groups=100).to_arrow()
        b = plain.rel().scan_filter(plist()).groupby(keys, aggs(), est_groups=100).to_arrow()
        assert sorted(map(tuple, (r.values() for r in a.to_pylist()))) == sorted(map(tuple, (r.values() for r in b.to_pylist())))
        assert sum(a.column(len(keys)).to_pylist()) == len(want) and sum(a.column(len(keys) + 1).to_pylist()) == int(sum(int(k[i]) for i in want))


@pytest.mark.parametrize("consts", [[b"c00007"], [b"c00014", b"", b"ab\0", b"nothing"], NINE[:8]], ids=["one", "four", "eight"])
def test_inline_and_string_set_kernel_agree(ctx, base, consts):
    vals, plain = base["vals"], base["plain"]
    inline = plain.rel().scan_filter([in_pred((0, 0), consts), api.pred((0, 1), capi.F_LT, 70)])
    ctx.prof_enable(True)
    ctx.prof_reset()
    with option(b"scan_strset_min_in", 1, 9):
        forced = plain.rel().scan_filter([in_pred((0, 0), consts), api.pred((0, 1), capi.F_LT, 70)])
        forced_count = plain.rel().scan_count([in_pred((0, 0), consts), api.pred((0, 1), capi.F_LT, 70)])
    prof = ctx.prof_all()
    ctx.prof_enable(False)
    assert prof.get("k_strset_bitmap_lds", (0, 0.0))[0] == 2
    want = [i for i in want_in(vals, consts) if base["k"][i] < 70]
    assert rows_of(inline) == rows_of(forced) == want and forced_count == len(want) and inline.sides == forced.sides == 1


def test_lazy_mode_forces(ctx, base):
    vals, k, consts, plain = base["vals"], base["k"], base["consts"], base["plain"]
    want = [i for i in want_in(vals, consts) if k[i] < 50]
    with option(b"lazy_min_rows", 0, 1 << 20):
        assert rows_of(plain.rel().scan_filter([in_pred((0, 0), consts), api.pred((0, 1), capi.F_LT, 50)])) == want
        lazy = plain.rel().scan_filter([api.pred((0, 1), capi.F_LT, 50)])  # stays pending
        assert rows_of(lazy.scan_filter([in_pred((0, 0), consts)])) == want
        lazy2 = plain.rel().scan_filter([api.pred((0, 1), capi.F_LT, 50)])
        assert lazy2.scan_count([in_pred((0, 0), consts)]) == len(want)


OPS = {"EQ": (capi.F_EQ, lambda a, b: a == b), "NEQ": (capi.F_NEQ, lambda a, b: a != b), "LT": (capi.F_LT, lambda a, b: a < b),
       "LTE": (capi.F_LTE, lambda a, b: a <= b), "GT": (capi.F_GT, lambda a, b: a > b), "GTE": (capi.F_GTE, lambda a, b: a >= b)}


@pytest.fixture(scope="module")
def long_rows(ctx):
    rows = [None, b"", b"\xff"]
    for size in (49, 100):
        c = bytes((65 + j % 26) for j in range(size))
        rows += [c, c, c[:48], c[:48] + b"!" * (size - 48), c[:48] + b"\xff" * (size - 48), c[:-1], c + b"\0", c + b"z", c[:8], c[:7] + b"\0", c[:20] + b"@" + c[21:]]
    rng = np.random.default_rng(5)
    rows = [rows[j] for j in rng.integers(0, len(rows), 3000)] + rows
    return rows, register(ctx, "ss_long", pa.table({"s": str_array(rows)}))


@pytest.mark.parametrize("size", [49, 100])
@pytest.mark.parametrize("op", list(OPS))
def test_long_constants(ctx, long_rows, op, size):
    rows, t = long_rows
    c = bytes((65 + j % 26) for j in range(size))
    assert c in rows and c[:48] in rows and c[:-1] in rows
    code, fn = OPS[op]
    want = [i for i, v in enumerate(rows) if v is not None and fn(v, c)]
    assert 0 < len(want) < len(rows)
    assert rows_of(t.rel().scan_filter([api.pred((0, 0), code, c)])) == want
    assert t.rel().scan_count([api.pred((0, 0), code, c)]) == len(want)


TEN = [b"c00000", b"c00007", b"c00014", b"c00021", b"", b"ab", b"not there", b"abcdefghij", b"twelve bytes07xx", b"x" * 70]


def plan_text():
    preds = [{"col": "s", "op": "IN", "values": [c.decode() for c in TEN]}] + [{"col": "c%d" % i, "op": "GTE" if i % 2 else "LTE", "value": 3 if i % 2 else 97} for i in range(9)]
    return json.dumps({"name": "strset", "inputs": ["t"], "steps": [{"op": "filter", "in": "t", "out": "f", "preds": preds}, {"op": "materialize", "in": "f", "cols": ["i"], "out": "r"}],
                       "result": "r"})


def plan_want(base):
    tab = base["tab"]
    keep = np.ones(tab.num_rows, dtype=bool)
    for i in range(9):
        c = tab.column("c%d" % i).to_numpy()
        keep &= (c >= 3) if i % 2 else (c <= 97)
    return [i for i in want_in(base["vals"], TEN) if keep[i]]


def test_plan_filter_step_and_prepared_replay(ctx, base):
    want = plan_want(base)
    assert len(want) > 100
    for t in (base["plain"], base["enc"]):
        assert ctx.run_plan(plan_text(), {"t": t}).to_arrow().column(0).to_pylist() == want
        prepared = ctx.prepare_plan(plan_text())
        for _ in range(3):
            assert prepared.execute({"t": t}).to_arrow().column(0).to_pylist() == want
        st = prepared.stats()
        assert st["replays"] >= 1 and st["misses"] == 0, st
        prepared.release()
    long_value = json.dumps({"name": "strset_cmp", "inputs": ["t"], "steps": [
        {"op": "filter", "in": "t", "out": "f", "preds": [{"col": "s", "op": "GTE", "value": "c00035" + "z" * 50}]}, {"op": "materialize", "in": "f", "cols": ["i"], "out": "r"}], "result": "r"})
    c = b"c00035" + b"z" * 50
    assert ctx.run_plan(long_value, {"t": base["plain"]}).to_arrow().column(0).to_pylist() == [i for i, v in enumerate(base["vals"]) if v is not None and v >= c]


def test_translated_sub_operator_document(ctx):
    import test_strset_api as cpu_half

    names = [b"PERU", b"ALGERIA", None, b"UNITED KINGDOM, THE ISLE OF MAN AND THE CHANNEL ISLANDS OF", b"ALGERIA ", b"GERMANY", b"", b"INDIA", b"UNITED KINGDOM"] * 5
    t = ctx.register("nation_ss", pa.table({"n_nationkey": pa.array(np.arange(len(names), dtype=np.int32)), "n_name": str_array(names)}))
    got = ctx.run_subop_dump(cpu_half.string_in_dump(), {"nation": t}).to_arrow()
    member = {c.encode() for c in cpu_half.COUNTRIES}
    assert got.column(0).to_pylist() == [i for i, v in enumerate(names) if v in member] and got.num_rows == 20
    t.release()


def _live(ctx):
    gc.collect()
    s = ctx.mem_stats()
    return s["live_blocks"], s["live_bytes"]


def held(ctx):
    st = ctx.desc_cache_stats()
    return st["held"], st["underflows"]


def test_dnf_refuses_and_resources_balance(ctx, base):
    plain, consts = base["plain"], base["consts"]
    big = many(LDS_MAX + 1)

    def run():
        r = plain.rel()
        outs = [r.scan_filter([in_pred((0, 0), consts), api.pred((0, 1), capi.F_LT, 50)]), r.scan_filter([in_pred((0, 0), big)]),
                r.scan_filter([api.pred((0, 0), capi.F_GT, b"c" * 90)])]
        r.scan_count([in_pred((0, 0), consts)])
        g = r.groupby([], [api.agg(capi.AGG_COUNT_STAR)], [in_pred((0, 0), consts)])
        with pytest.raises(capi.LdbError) as e:
            r.scan_filter_dnf([[api.pred((0, 1), capi.F_LT, 5)], [in_pred((0, 0), consts), api.pred((0, 1), capi.F_GT, 90)]])
        assert e.value.status == capi.LDB_ERR_UNSUPPORTED and "clause 1 holds a string-set conjunct" in str(e.value)
        for o in outs + [g, r]:
            o.release()

    run()
    run()
    want = _live(ctx)
    run()
    assert _live(ctx) == want
    assert held(ctx) == (0, 0)


def test_reference_restrictions_fixture(ctx):
    """tests/golden/ref_long_in.json (make_ref_long_in.py): the reference's own Restrictions over a seeded table, lists of 10 and 300 strings"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_long_in.json")) as f:
        fx = json.load(f)
    rows = [None if v is None else v.encode() for v in fx["rows"]]
    assert len(rows) >= 2000 and sorted(len(c["values"]) for c in fx["cases"]) == [10, 300]
    t = register(ctx, "ss_ref", pa.table({"s": str_array(rows), "k": pa.array(np.asarray(fx["k"], dtype=np.int32))}))
    for case in fx["cases"]:
        consts = [v.encode() for v in case["values"]]
        plist = [in_pred((0, 0), consts)] + ([api.pred((0, 1), capi.F_LT, case["k_lt"])] if "k_lt" in case else [])
        got = rows_of(t.rel().scan_filter(plist))
        assert got == case["passing"] and len(got) > 0
    t.release()
