"""String expressions as computed columns on the device (csrc/ldb_strfn.hip: ldb_gpu_map_strcat / ldb_gpu_map_strlen): every case
bit-exact — offsets, bytes and validity — against tests/strfn_eval.py, the Python restatement of the reference's string
runtime that tests/test_strfn_api.py pins to the recorded outputs of the reference; the fixture's own cases are compared
with those recorded outputs directly.  Shapes are the smallest at which the byte-parallel fill can go wrong: T = the tile
(bytes of output per workgroup step), W = 16 = the bytes one lane stores, R = the offsets staged in LDS at a time."""
import collections
import ctypes as C
import gc
import json

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi
import strfn_eval as E

pytestmark = pytest.mark.gpu
W = 16


@pytest.fixture(scope="module")
def geom():
    lib = capi.gpu_lib()
    return int(lib.ldb_strcat_tile_bytes()), int(lib.ldb_strcat_lds_rows())


@pytest.fixture(scope="module")
def fx():
    return E.load_fixture()


def tobytes(v):
    return None if v is None else v.encode() if isinstance(v, str) else v


def assert_utf8(tab, want, what=""):
    """the one column of `tab` = want (bytes or None per row): offsets, value bytes, validity"""
    want = [tobytes(v) for v in want]
    assert tab.rows == len(want), what
    arr = tab.to_arrow().column(0).combine_chunks()
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.chunk(0) if arr.num_chunks else pa.array([], arr.type)
    n = len(want)
    assert len(arr) == n, what
    if n == 0:
        return
    assert arr.type in (pa.large_string(), pa.string(), pa.large_binary(), pa.binary()), arr.type
    bufs = arr.buffers()
    odt = np.int64 if arr.type in (pa.large_string(), pa.large_binary()) else np.int32
    offs = np.frombuffer(bufs[1], dtype=odt)[arr.offset: arr.offset + n + 1].astype(np.int64)
    exp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([0 if v is None else len(v) for v in want], out=exp[1:])
    assert np.array_equal(offs - offs[0], exp), what
    data = bufs[2].to_pybytes()[int(offs[0]): int(offs[-1])] if bufs[2] is not None else b""
    blob = b"".join(v for v in want if v is not None)
    if data != blob:
        k = next(i for i in range(min(len(data), len(blob))) if data[i] != blob[i]) if len(data) == len(blob) else -1
        raise AssertionError("%s: value bytes differ (first at byte %d of %d): got %r want %r" % (what, k, len(blob), data[max(0, k - 8): k + 24], blob[max(0, k - 8): k + 24]))
    valid = [arr[i].is_valid for i in range(n)] if n <= 4096 else np.asarray(arr.is_valid()).tolist()
    assert valid == [v is not None for v in want], what


def reg(ctx, cols, name="strfn_t", dict_encode=True):
    """dict_encode = False: registered without dictionaries (building one sorts the distinct strings, which takes keys of at most 256 bytes)"""
    lib = capi.gpu_lib()
    if not dict_encode:
        lib.ldb_gpu_set_option(b"dict_encode", 0)
    try:
        return ctx.register(name, pa.table(cols))
    finally:
        lib.ldb_gpu_set_option(b"dict_encode", 1)


def sarr(vals):
    return pa.array([None if v is None else (v.decode() if isinstance(v, bytes) else v) for v in vals], pa.string())


def run_forms(ctx, strings, what, dict_encode=True):
    """copy, upper, lower, a || a, const || a over one column of strings"""
    t = reg(ctx, {"s": sarr(strings)}, dict_encode=dict_encode)
    r = t.rel()
    s = [tobytes(v) for v in strings]
    n = len(s)
    assert_utf8(r.map_strcat([{"col": (0, 0)}]), s, what + " copy")
    assert_utf8(r.map_upper((0, 0)), E.strcat([{"col": s, "case": "upper"}], n), what + " upper")
    assert_utf8(r.map_lower((0, 0)), E.strcat([{"col": s, "case": "lower"}], n), what + " lower")
    assert_utf8(r.map_strcat([{"col": (0, 0)}, {"col": (0, 0), "case": "upper"}]), E.strcat([{"col": s}, {"col": s, "case": "upper"}], n), what + " a||A")
    assert_utf8(r.map_strcat(["<>", {"col": (0, 0)}]), E.strcat([b"<>", {"col": s}], n), what + " const||a")
    ln = r.map_strlen((0, 0)).to_arrow().column(0).to_pylist()
    assert ln == [None if v is None else E.length(v) for v in s], what + " length"
    r.release(), t.release()


# ---------------------------------------------------------------- row counts, totals, NULL / empty extremes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_row_counts(ctx, fx, n):
    pool = [b.decode() for b in fx["strings"]]
    strings = [None if i % 29 == 7 else pool[(i * 7) % len(pool)] for i in range(n)]
    run_forms(ctx, strings, "n=%d" % n)
    if n:
        run_forms(ctx, [pool[(i * 5) % len(pool)] for i in range(n)], "n=%d not null" % n)


def test_totals_around_the_lane_word(ctx):
    for k in (W - 1, W, W + 1, 2 * W, 3 * W - 1):
        run_forms(ctx, ["ab"] * (k // 2) + (["c"] if k % 2 else []), "total %d" % k)
    run_forms(ctx, [None] * 130, "all NULL")
    run_forms(ctx, [""] * 130, "all empty")
    run_forms(ctx, ["", None] * 70 + ["x"], "one byte at the end")


# ---------------------------------------------------------------- tile and LDS boundaries
def test_tile_and_lds_boundaries(ctx, geom):
    T, R = geom
    cases = {
        "row straddles a tile boundary": ["a" * (T - 6), "Bc" * 10, "d" * 3, "e" * (T + 1)],
        "3T+5 among 1-byte rows": ["x"] * 700 + ["Ab" * ((3 * T + 5) // 2) + "z"] + ["y"] * 700,
        "more empty / 1-byte rows in a tile than the LDS holds": ["q"] * 10 + [""] * (2 * R + 300) + ["r"] * (R + 500) + [""] * (R + 77) + ["s" * (T + 9)] + [""] * (3 * R) + ["t"],
        "last row ends on a tile boundary": ["a" * (T - 96), "b" * 96, "c" * T],
        "exactly one tile": ["m" * T],
        "tile + 1": ["m" * T, "n"],
        "more than one workgroup's run of tiles": ["Row %d " % i * 40 for i in range(700)],
    }
    for what, rows in cases.items():
        run_forms(ctx, rows, what, dict_encode=False)


# ---------------------------------------------------------------- part shapes
def test_part_counts_constants_and_windows(ctx, fx):
    pool = [b.decode() for b in fx["strings"]]
    n = 300
    a = [pool[(3 * i) % len(pool)] for i in range(n)]
    b = [None if i % 41 == 0 else pool[(11 * i + 5) % len(pool)] for i in range(n)]
    k = [int(v) for v in (fx["ints"] * 4)[:n]]
    t = reg(ctx, {"a": sarr(a), "b": sarr(b), "k": pa.array(k, pa.int64())})
    r = t.rel()
    ab, bb = [tobytes(v) for v in a], [tobytes(v) for v in b]
    big = ("0123456789" * 30).encode()
    shapes = {
        "1 part": ([{"col": (0, 0)}], [{"col": ab}]),
        "2 parts": ([{"col": (0, 0)}, {"col": (0, 1)}], [{"col": ab}, {"col": bb}]),
        "8 parts": (["[", {"col": (0, 0), "case": "lower"}, "|", {"int": (0, 2)}, "|", {"col": (0, 1), "case": "upper"}, "]", {"col": (0, 0)}],
                    [b"[", {"col": ab, "case": "lower"}, b"|", {"int": k}, b"|", {"col": bb, "case": "upper"}, b"]", {"col": ab}]),
        "same column twice": ([{"col": (0, 1)}, {"col": (0, 1)}], [{"col": bb}, {"col": bb}]),
        "empty constant": (["", {"col": (0, 0)}, ""], [b"", {"col": ab}, b""]),
        "only constants": (["abc", ""], [b"abc", b""]),
        "300-byte constant": ([big, {"col": (0, 0)}, big], [big, {"col": ab}, big]),
    }
    for what, (parts, ev) in shapes.items():
        assert_utf8(r.map_strcat(parts), E.strcat(ev, n), what)
    # windows in CHARACTERS on strings with multi-byte characters: inside, before and past the string, with the case mapping applied afterwards
    for frm, ln in ((1, 3), (2, 2), (0, 2), (-2, 5), (3, 0), (4, -1), (1, 1 << 30), (30, 4), (6, 7), (2, capi.STR_WHOLE), (1, capi.STR_WHOLE)):
        parts = [{"col": (0, 0), "case": "upper", "from": frm, "for": ln}, "-", {"col": (0, 1), "from": frm, "for": ln}]
        ev = [{"col": ab, "case": "upper", "from": frm, "for": ln}, b"-", {"col": bb, "from": frm, "for": ln}]
        assert_utf8(r.map_strcat(parts), E.strcat(ev, n), "window (%d, %d)" % (frm, ln))
    r.release(), t.release()


def test_integer_parts(ctx, fx):
    ints = [int(v) for v in fx["ints"]]
    k64 = ints + [None, 0, None]
    i32 = [v for v in ints if -(2 ** 31) <= v < 2 ** 31]
    k32 = (i32 * (len(k64) // len(i32) + 1))[: len(k64) - 1] + [None]
    t = reg(ctx, {"k64": pa.array(k64, pa.int64()), "k32": pa.array(k32, pa.int32())})
    r = t.rel()
    n = len(k64)
    got = r.map_strcat([{"int": (0, 0)}])
    assert_utf8(got, [None if v is None else E.from_int(v) for v in k64], "int64")
    assert got.to_arrow().column(0).to_pylist()[: len(ints)] == [s.decode() for s in fx["from_int"]]  # the reference's recorded fromInt
    assert_utf8(r.map_strcat([{"int": (0, 1)}]), [None if v is None else E.from_int(v) for v in k32], "int32")
    assert_utf8(r.map_strcat(["k=", {"int": (0, 0)}, "/", {"int": (0, 1)}]), E.strcat([b"k=", {"int": k64}, b"/", {"int": k32}], n), "const || int64 || const || int32")
    r.release(), t.release()


# ---------------------------------------------------------------- relation shapes
def test_filtered_relation_and_outer_join_side(ctx, fx):
    pool = [b.decode() for b in fx["strings"]]
    n = 1000
    s = [None if i % 13 == 2 else pool[(7 * i) % len(pool)] for i in range(n)]
    v = [i % 10 for i in range(n)]
    t = reg(ctx, {"s": sarr(s), "v": pa.array(v, pa.int32()), "k": pa.array(list(range(n)), pa.int64())})
    f = t.rel().scan_filter([api.pred((0, 1), capi.F_LT, 4)])  # row-id indirection
    keep = [i for i in range(n) if v[i] < 4]
    sb = [tobytes(x) for x in s]
    assert_utf8(f.map_strcat([{"col": (0, 0), "case": "upper"}, "#", {"int": (0, 2)}]), [None if sb[i] is None else E.upper(sb[i]) + b"#" + E.from_int(i) for i in keep], "behind a filter")
    assert f.map_strlen((0, 0)).to_arrow().column(0).to_pylist() == [None if sb[i] is None else E.length(sb[i]) for i in keep]
    # the nullable side of a left outer join: NULL row ids
    probe = reg(ctx, {"k": pa.array([5, 2000, 7, 3000, 999, 0, 4000], pa.int64())}, "strfn_probe")
    ht = t.rel().join_build([(0, 2)], unique=True)
    j = ht.probe(probe.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    pk, bk = j.rowids(0).tolist(), j.rowids(1).tolist()
    want = []
    for b in bk:
        want.append(None if b == capi.LDB_NULL_ROW or sb[b] is None else b"<" + E.lower(sb[b]) + b">")
    assert sum(1 for b in bk if b == capi.LDB_NULL_ROW) == 3 and len(pk) == 7
    assert_utf8(j.map_strcat(["<", {"col": (1, 0), "case": "lower"}, ">"]), want, "outer join side")
    assert j.map_strlen((1, 0)).to_arrow().column(0).to_pylist() == [None if b == capi.LDB_NULL_ROW or sb[b] is None else E.length(sb[b]) for b in bk]


def test_nulls_at_bitmap_word_boundaries(ctx):
    n = 200
    s = [None if i in (63, 64, 127) else "Row%d" % i for i in range(n)]
    k = [None if i in (0, 128, 199) else i for i in range(n)]
    t = reg(ctx, {"s": sarr(s), "k": pa.array(k, pa.int32())})
    r = t.rel()
    assert_utf8(r.map_upper((0, 0)), [None if v is None else v.upper() for v in s], "nulls at 63 / 64 / 127")
    assert_utf8(r.map_strcat([{"col": (0, 0)}, {"int": (0, 1)}]), [None if a is None or b is None else "%s%d" % (a, b) for a, b in zip(s, k)], "nulls of two parts")


# ---------------------------------------------------------------- the reference's recorded outputs
def test_reference_fixture(ctx, fx):
    s = fx["strings"]
    t = reg(ctx, {"a": sarr(s[:-1]), "b": sarr(s[1:])}, "strfn_fixture")
    r = t.rel()
    assert_utf8(r.map_upper((0, 0)), fx["upper"][:-1], "upper")
    assert_utf8(r.map_upper((0, 1)), fx["upper"][1:], "upper b")
    assert_utf8(r.map_lower((0, 0)), fx["lower"][:-1], "lower")
    assert_utf8(r.map_lower((0, 1)), fx["lower"][1:], "lower b")
    assert r.map_strlen((0, 0)).to_arrow().column(0).to_pylist() + r.map_strlen((0, 1)).to_arrow().column(0).to_pylist()[-1:] == fx["length"]
    assert_utf8(r.map_strcat([{"col": (0, 0)}, {"col": (0, 1)}]), fx["concat_next"], "a || b")
    by_args = collections.defaultdict(list)
    for c in fx["substr"]:
        by_args[(c["from"], c["for"])].append(c)
    for (frm, ln), cs in by_args.items():
        tt = reg(ctx, {"s": sarr([s[c["i"]] for c in cs])}, "strfn_sub")
        assert_utf8(tt.rel().map_strcat([{"col": (0, 0), "from": frm, "for": ln}]), [c["out"] for c in cs], "substr (%d, %d)" % (frm, ln))
        tt.release()


# ---------------------------------------------------------------- lazy dictionary columns
def test_lazily_gathered_dictionary_column(ctx):
    words = ["", "AIR", "Reg Air", "Zürich", "straße", "中文 mixed Ab", "a considerably longer string value, Past The Short Boundary"]
    n = 12_000
    rng = np.random.default_rng(7)
    s = [None if i % 19 == 4 else words[int(j)] for i, j in enumerate(rng.integers(0, len(words), n))]
    v = rng.integers(0, 3, n).astype(np.int32)
    t = reg(ctx, {"s": sarr(s), "v": pa.array(v)}, "strfn_dict")
    assert t.dict_size(0) == len(words)
    keep = [i for i in range(n) if v[i] < 2]
    assert len(keep) >= 4096
    sb = [tobytes(x) for x in s]
    want_u = [None if sb[i] is None else E.upper(sb[i]) + b"!" for i in keep]
    want_l = [None if sb[i] is None else E.length(sb[i]) for i in keep]
    lib = capi.gpu_lib()
    got = {}
    try:
        for lazy in (1, 0):
            lib.ldb_gpu_set_option(b"lazy_strings", lazy)
            m = t.rel().scan_filter([api.pred((0, 1), capi.F_LT, 2)]).materialize([(0, 0)])  # lazy when on: codes + the shared dictionary only
            u = m.rel().map_strcat([{"col": (0, 0), "case": "upper"}, "!"])
            assert_utf8(u, want_u, "lazy_strings=%d" % lazy)
            m2 = t.rel().scan_filter([api.pred((0, 1), capi.F_LT, 2)]).materialize([(0, 0)])
            assert m2.rel().map_strlen((0, 0)).to_arrow().column(0).to_pylist() == want_l
            got[lazy] = u.to_arrow().column(0).to_pylist()
    finally:
        lib.ldb_gpu_set_option(b"lazy_strings", 1)
    assert got[1] == got[0]


# ---------------------------------------------------------------- composition: the result is an ordinary utf8 column
def test_group_by_upper_and_join_on_a_concatenation(ctx):
    import pandas as pd

    rng = np.random.default_rng(11)
    n = 3000
    names = ["alpha", "Alpha", "ALPHA", "beta", "Beta", "gamma", "straße", "STRAßE", "é", "É"]
    df = pd.DataFrame({"s": [names[int(j)] for j in rng.integers(0, len(names), n)], "v": rng.integers(0, 100, n).astype(np.int64), "a": ["k%d" % int(j) for j in rng.integers(0, 30, n)],
                       "b": rng.integers(0, 20, n).astype(np.int64)})
    t = reg(ctx, {c: pa.array(df[c]) for c in df.columns}, "strfn_comp")
    r = t.rel()
    z = r.zip(r.map_upper((0, 0), name="u"))
    g = z.groupby([(1, 0)], [api.agg(capi.AGG_SUM, api.col_expr((0, 1))), api.agg(capi.AGG_COUNT_STAR)], est_groups=16).to_arrow()
    got = {k: (int(a), int(b)) for k, a, b in zip(g.column(0).to_pylist(), g.column(1).to_pylist(), g.column(2).to_pylist())}
    key = df["s"].map(lambda x: E.upper(x.encode()).decode())
    want = {k: (int(d["v"].sum()), len(d)) for k, d in df.groupby(key)}
    # six groups: alpha / Alpha / ALPHA, beta / Beta, gamma, straße / STRAßE (ß passes through), and é and É apart (no mapping of bytes >= 0x80 in the C locale)
    assert got == want and set(want) == {"ALPHA", "BETA", "GAMMA", "STRAßE", "é", "É"}
    # join on a || '-' || cast(b as varchar)
    other = pd.DataFrame({"key": ["k%d-%d" % (i, j) for i in range(0, 30, 2) for j in range(0, 20, 3)]})
    other["id"] = np.arange(len(other), dtype=np.int64)
    o = reg(ctx, {c: pa.array(other[c]) for c in other.columns}, "strfn_other")
    z2 = r.zip(r.map_strcat([{"col": (0, 2)}, "-", {"int": (0, 3)}], name="k"))
    j = o.rel().join_build([(0, 0)], unique=True).probe(z2, [(1, 0)], capi.JOIN_INNER)
    pairs = sorted(zip(j.rowids(0).tolist(), j.rowids(j.sides - 1).tolist()))
    df["k"] = df["a"] + "-" + df["b"].astype(str)
    m = df.reset_index().merge(other, left_on="k", right_on="key")
    assert pairs == sorted(zip(m["index"].tolist(), m["id"].tolist())) and len(pairs) > 100


# ---------------------------------------------------------------- the plan language
def test_plan_steps(ctx, fx):
    pool = [b.decode() for b in fx["strings"]]
    n = 1000
    s = [None if i % 23 == 1 else pool[(5 * i) % len(pool)] for i in range(n)]
    k = [(-1) ** i * i * 977 for i in range(n)]
    t = reg(ctx, {"c_name": sarr(s), "s_key": pa.array(k, pa.int64())}, "strfn_plan")
    sb = [tobytes(x) for x in s]
    steps = [
        {"op": "map", "in": "t", "fn": "upper", "col": "c_name", "as": "u", "out": "r1"},
        {"op": "map", "in": "r1", "fn": "lower", "col": "c_name", "as": "l", "out": "r2"},
        {"op": "map", "in": "r2", "fn": "length", "col": "c_name", "as": "n", "out": "r3"},
        {"op": "map", "in": "r3", "fn": "concat", "as": "k", "out": "r4", "parts": [{"const": "store"}, {"col": "c_name", "case": "upper", "from": 1, "for": 4}, {"int": "s_key"}, {"col": "u"}]},
        {"op": "materialize", "in": "r4", "cols": ["u", "l", "n", "k"], "out": "result"},
    ]
    plan = json.dumps({"inputs": ["t"], "steps": steps, "result": "result"})
    res = ctx.run_plan(plan, {"t": t}).to_arrow()
    dec = lambda v: None if v is None else v.decode()  # noqa: E731
    assert res.column(0).to_pylist() == [dec(None if b is None else E.upper(b)) for b in sb]
    assert res.column(1).to_pylist() == [dec(None if b is None else E.lower(b)) for b in sb]
    assert res.column(2).to_pylist() == [None if b is None else E.length(b) for b in sb]
    up = [None if b is None else E.upper(b) for b in sb]
    assert res.column(3).to_pylist() == [dec(v) for v in E.strcat([b"store", {"col": sb, "case": "upper", "from": 1, "for": 4}, {"int": k}, {"col": up}], n)]


# ---------------------------------------------------------------- errors and device-memory balance
def _live(ctx):
    gc.collect()
    m = ctx.mem_stats()
    return m["live_blocks"], m["live_bytes"]


def test_errors_name_the_part_and_leave_nothing_behind(ctx):
    t = reg(ctx, {"s": sarr(["a", "b", None]), "k": pa.array([1, 2, 3], pa.int64()), "d": pa.array([1.0, 2.0, 3.0], pa.float64())}, "strfn_err")
    r = t.rel()
    cases = [
        ([], capi.LDB_ERR_UNSUPPORTED, "LDB_MAX_STRPARTS = 8"),
        (["x"] * 9, capi.LDB_ERR_UNSUPPORTED, "LDB_MAX_STRPARTS = 8"),
        (["x", {"col": (0, 1)}], capi.LDB_ERR_INVALID, "part 1"),
        (["x", "y", {"int": (0, 0)}], capi.LDB_ERR_INVALID, "part 2"),
        ([{"int": (0, 2)}], capi.LDB_ERR_INVALID, "part 0"),
    ]
    bad_case = api.str_parts(["x", "y"])[0]
    bad_case[1].strcase = capi.SC_UPPER
    cases.append(([bad_case[0], bad_case[1]], capi.LDB_ERR_INVALID, "part 1"))
    bad_win = api.str_parts([{"col": (0, 0)}, {"int": (0, 1)}])[0]
    bad_win[1].from_, bad_win[1].for_len = 2, 3
    cases.append(([bad_win[0], bad_win[1]], capi.LDB_ERR_INVALID, "part 1"))
    r.map_upper((0, 0)).release()  # (warms whatever the first call caches)
    for parts, status, word in cases:
        before = _live(ctx)
        with pytest.raises(capi.LdbError) as e:
            r.map_strcat(parts)
        assert e.value.status == status and word in str(e.value), str(e.value)
        assert _live(ctx) == before, word
    before = _live(ctx)
    with pytest.raises(capi.LdbError) as e:
        r.map_strlen((0, 1))
    assert e.value.status == capi.LDB_ERR_INVALID and _live(ctx) == before


def test_successful_calls_balance(ctx, fx):
    pool = [b.decode() for b in fx["strings"]]
    t = reg(ctx, {"s": sarr([None if i % 9 == 0 else pool[i % len(pool)] for i in range(5000)]), "k": pa.array(list(range(5000)), pa.int32())}, "strfn_bal")
    r = t.rel()

    def run():
        r.map_strcat(["store", {"col": (0, 0), "case": "upper", "from": 2, "for": 5}, {"int": (0, 1)}, {"col": (0, 0)}]).release()
        r.map_upper((0, 0)).release()
        r.map_strlen((0, 0)).release()

    run()
    run()
    want = _live(ctx)
    run()
    assert _live(ctx) == want
