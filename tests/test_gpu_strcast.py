"""Casts between text and int / decimal / date on the device (csrc/ldb_strcast.hip: ldb_gpu_map_strparse; csrc/ldb_strfn.hip:
the DECIMAL / DATE parts of ldb_gpu_map_strcat): every case bit-exact — values, validity, offsets and bytes — against
tests/strcast_eval.py, the plain-Python restatement that tests/test_strcast_api.py pins to pyarrow.  Shapes are the smallest
at which the kernels can go wrong: the 64-row ballot word and the 256-thread block for the parse, the last bytes of the
value buffer for its eight-byte loads, the 16-byte lane word, the tile T and the staged offsets R for the fill."""
import decimal
import json

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi
import strcast_eval as E

pytestmark = pytest.mark.gpu
CTX80 = decimal.Context(prec=80)
KINDS = {"int": capi.PARSE_INT64, "decimal": capi.PARSE_DECIMAL, "date": capi.PARSE_DATE}


@pytest.fixture(scope="module")
def geom():
    lib = capi.gpu_lib()
    return int(lib.ldb_strcat_tile_bytes()), int(lib.ldb_strcat_lds_rows())


def tobytes(v):
    return None if v is None else v.encode() if isinstance(v, str) else v


def sarr(vals):
    return pa.array([None if v is None else (v.decode() if isinstance(v, bytes) else v) for v in vals], pa.string())


def darr(unscaled, p, s):
    return pa.array([None if v is None else decimal.Decimal(v).scaleb(-s, context=CTX80) for v in unscaled], pa.decimal128(p, s))


def reg(ctx, cols, name="strcast_t", dict_encode=True, narrow=0):
    lib = capi.gpu_lib()
    if not dict_encode:
        lib.ldb_gpu_set_option(b"dict_encode", 0)
    try:
        return ctx.register(name, pa.table(cols), narrow_decimals=narrow)
    finally:
        lib.ldb_gpu_set_option(b"dict_encode", 1)


def one_chunk(tab):
    arr = tab.to_arrow().column(0).combine_chunks()
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.chunk(0) if arr.num_chunks else pa.array([], arr.type)
    return arr


def parsed_values(tab, kind, precision=0, scale=0):
    """the one column of a parse result as Python ints (unscaled for decimals, days for dates) with None for NULL"""
    arr = one_chunk(tab)
    if kind == "int":
        assert arr.type == pa.int64()
        return arr.to_pylist()
    if kind == "date":
        assert arr.type == pa.date32()
        return arr.cast(pa.int32()).to_pylist()
    assert arr.type == pa.decimal128(precision, scale), arr.type
    return [None if v is None else int(v.scaleb(scale, context=CTX80)) for v in arr.to_pylist()]


def assert_parse(rel, col, kind, strings, precision=0, scale=0, what=""):
    """strings: what the rows of (rel, col) hold, in order.  Values, validity and both ways of asking for the bad count"""
    want, bad = E.parse_column(kind, [tobytes(s) for s in strings], precision, scale)
    tab, n_bad = rel.map_strparse(col, KINDS[kind], precision, scale)
    assert tab.rows == len(strings), what
    got = parsed_values(tab, kind, precision, scale)
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s %s: row %d %r: got %r want %r" % (what, kind, k, strings[k], got[k], want[k]))
    assert n_bad == bad, (what, kind, n_bad, bad)
    quiet, none = rel.map_strparse(col, KINDS[kind], precision, scale, count_bad=False)  # n_bad = NULL: the same column
    assert none is None and parsed_values(quiet, kind, precision, scale) == want, what
    tab.release(), quiet.release()
    return want


def assert_utf8(tab, want, what=""):
    """the one column of `tab` = want (bytes or None per row): offsets, value bytes, validity"""
    want = [tobytes(v) for v in want]
    assert tab.rows == len(want), what
    arr = one_chunk(tab)
    n = len(want)
    assert len(arr) == n, what
    if n == 0:
        return
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


# ---------------------------------------------------------------- the cases of the issue
INT_CASES = ["9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "+0", "-0", "0" * 30 + "12", "\t\n 12", "12 ", "1 2", "0x10", "+", "", "7", "-15", " +5"]
DEC_CASES_12_2 = ["+1.5", "-.5", "1.", "1e2", "00012.30", "-0", " 1.5", "1.5 ", ".", "", "1_0", "1.23E-1", "1.230", "1.234", "1e2000000000", "9999999999.99", "10000000000", "-9999999999.99", "-10000000000.00",
                  "1e+-2", "1e-+2", "0e39"]
DATE_CASES = ["0001-01-01", "9999-12-31", "1970-01-01", "1900-02-29", "2000-02-29", "2004-02-29", "2100-02-29", "1998-04-31", "1998-06-31", "1998-09-31", "1998-11-31", "1998-04-30", "1998-02-30",
              "1998-13-01", "1998-00-10", "1998-01-00", "1998-01-0", "1998-01-011", "1998-1-011", "1998 01-01", "0000-01-01", "199a-01-01", "2024-12-31"]
DEC_VALUES = sorted({0} | {s * v for k in (1, 18, 19, 20, 37) for v in (1, 10 ** k - 1, 10 ** k) for s in (1, -1)})
POOL = {"int": INT_CASES, "decimal": DEC_CASES_12_2, "date": DATE_CASES}
PS = {"int": (0, 0), "decimal": (12, 2), "date": (0, 0)}


# ---------------------------------------------------------------- row counts at the ballot word and the block, NULLs
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts_and_validity(ctx, n):
    for kind, pool in POOL.items():
        p, s = PS[kind]
        for nulls in (True, False):
            strings = [None if nulls and i % 29 == 7 else pool[(i * 5) % len(pool)] for i in range(n)]
            t = reg(ctx, {"s": sarr(strings)})
            r = t.rel()
            assert_parse(r, (0, 0), kind, strings, p, s, "n=%d nulls=%s" % (n, nulls))
            r.release(), t.release()


def test_filtered_relation_and_outer_join_side(ctx):
    n = 1000
    pool = DEC_CASES_12_2 + ["%d.%02d" % (i, i % 100) for i in range(40)]
    s = [None if i % 13 == 2 else pool[(7 * i) % len(pool)] for i in range(n)]
    v = [i % 10 for i in range(n)]
    t = reg(ctx, {"s": sarr(s), "v": pa.array(v, pa.int32()), "k": pa.array(list(range(n)), pa.int64())})
    f = t.rel().scan_filter([api.pred((0, 1), capi.F_LT, 4)])  # row-id indirection
    keep = [i for i in range(n) if v[i] < 4]
    assert_parse(f, (0, 0), "decimal", [s[i] for i in keep], 12, 2, "behind a filter")
    # the nullable side of a left outer join: NULL row ids are NULL, and not bad
    probe = reg(ctx, {"k": pa.array([5, 2000, 7, 3000, 999, 0, 4000, 6], pa.int64())}, "strcast_probe")
    j = t.rel().join_build([(0, 2)], unique=True).probe(probe.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    bk = j.rowids(1).tolist()
    assert sum(1 for b in bk if b == capi.LDB_NULL_ROW) == 3 and len(bk) == 8
    side = [None if b == capi.LDB_NULL_ROW else s[b] for b in bk]
    want = assert_parse(j, (1, 0), "decimal", side, 12, 2, "outer join side")
    assert sum(1 for b, w in zip(bk, want) if b == capi.LDB_NULL_ROW and w is None) == 3


@pytest.mark.parametrize("dict_encode", [True, False])
def test_last_string_ends_at_the_end_of_the_value_buffer(ctx, dict_encode):
    """the unaligned eight-byte loads stop at value_bytes: the last string of the buffer, at every length around two loads"""
    for ln in range(1, 18):
        digits = ("123456789" * 2)[:ln]
        date = "2024-02-29" if ln == 10 else digits
        for kind, last, p, s in (("int", digits, 0, 0), ("decimal", digits, 38, 0), ("decimal", digits[:-1] + "." if ln > 1 else digits, 38, 2), ("date", date, 0, 0)):
            strings = ["1", "22", last] if dict_encode else ["1", "22", "333", last]
            t = reg(ctx, {"s": sarr(strings)}, dict_encode=dict_encode)
            r = t.rel()
            want = assert_parse(r, (0, 0), kind, strings, p, s, "last string of %d bytes" % ln)
            assert (want[-1] is not None) == (kind != "date" or ln == 10)
            r.release(), t.release()


def test_to_int_cases(ctx):
    strings = INT_CASES + [" " * 4096 + "7", "\v\f\r-77", "99999999999999999999999", "-" + "0" * 40 + "9223372036854775808"]
    t = reg(ctx, {"s": sarr(strings)}, dict_encode=False)
    want = assert_parse(t.rel(), (0, 0), "int", strings, what="to_int")
    assert want[:13] == [2 ** 63 - 1, None, -(2 ** 63), None, 0, 0, 12, 12, None, None, None, None, None] and want[16] == 7


def test_to_decimal_cases(ctx):
    t = reg(ctx, {"s": sarr(DEC_CASES_12_2)})
    want = assert_parse(t.rel(), (0, 0), "decimal", DEC_CASES_12_2, 12, 2, "(12,2)")
    assert want[:12] == [150, -50, 100, 10000, 1230, 0, None, None, None, None, None, None]  # the table of the header
    assert want[12:19] == [123, None, None, 10 ** 12 - 1, None, -(10 ** 12 - 1), None]  # a dropped zero / non-zero digit, the exponent, 10^p - 1 and 10^p
    wide = ["9" * 38, "9" * 39, "-" + "9" * 38, "1e37", "1e38", "1E-38", "0." + "9" * 38, "0." + "0" * 37 + "1", "0" * 50 + "1", "1" + "0" * 38, "12345678901234567890.123456789012345678", "1e2000000000", "0e2000000000"]
    tw = reg(ctx, {"s": sarr(wide)}, "strcast_wide")
    w0 = assert_parse(tw.rel(), (0, 0), "decimal", wide, 38, 0, "(38,0)")
    assert w0[:5] == [10 ** 38 - 1, None, -(10 ** 38 - 1), 10 ** 37, None] and w0[8] == 1
    w38 = assert_parse(tw.rel(), (0, 0), "decimal", wide, 38, 38, "(38,38)")
    assert w38[3] is None and w38[4] is None and w38[5] == 1 and w38[6] == 10 ** 38 - 1 and w38[7] == 1
    assert_parse(tw.rel(), (0, 0), "decimal", wide, 38, 18, "(38,18)")
    for p, s in ((1, 0), (1, 1), (20, 8)):
        assert_parse(t.rel(), (0, 0), "decimal", DEC_CASES_12_2, p, s, "(%d,%d)" % (p, s))


def test_to_date_cases(ctx):
    strings = DATE_CASES + ["%04d-%02d-%02d" % (y, m, d) for y in (1, 1600, 1999, 2000) for m in (1, 2, 3, 12) for d in (1, 28, 29, 30, 31)]
    t = reg(ctx, {"s": sarr(strings)})
    want = assert_parse(t.rel(), (0, 0), "date", strings, what="to_date")
    assert want[:7] == [E.DATE_MIN, E.DATE_MAX, 0, None, 11016, 12477, None] and want[7:11] == [None] * 4 and want[11] is not None and want[16:22] == [None] * 6


def test_invalid_arguments_do_no_work(ctx):
    t = reg(ctx, {"s": sarr(["1"]), "k": pa.array([1], pa.int64())})
    r = t.rel()
    for args, word in ((((0, 1), capi.PARSE_INT64), "utf8"), (((0, 0), 3), "kind"), (((0, 0), capi.PARSE_DECIMAL, 0, 0), "precision"), (((0, 0), capi.PARSE_DECIMAL, 39, 0), "precision"),
                       (((0, 0), capi.PARSE_DECIMAL, 5, 6), "scale"), (((0, 0), capi.PARSE_DECIMAL, 5, -1), "scale")):
        before = ctx.mem_stats()["live_blocks"]
        with pytest.raises(capi.LdbError) as e:
            r.map_strparse(*args)
        assert e.value.status == capi.LDB_ERR_INVALID and word in str(e.value), str(e.value)
        assert ctx.mem_stats()["live_blocks"] == before
    for parts, word in (([{"dec": (0, 1)}], "part 0"), (["x", {"date": (0, 1)}], "part 1"), (["x", "y", {"dec": (0, 0)}], "part 2")):
        with pytest.raises(capi.LdbError) as e:
            r.map_strcat(parts)
        assert e.value.status == capi.LDB_ERR_INVALID and word in str(e.value), str(e.value)
    for key in ("dec", "date"):
        bad = api.str_parts(["x", {key: (0, 1)}])[0]
        bad[1].strcase = capi.SC_UPPER
        with pytest.raises(capi.LdbError) as e:
            r.map_strcat([bad[0], bad[1]])
        assert e.value.status == capi.LDB_ERR_INVALID and "part 1" in str(e.value)
        bad[1].strcase, bad[1].from_, bad[1].for_len = capi.SC_NONE, 2, 3
        with pytest.raises(capi.LdbError) as e:
            r.map_strcat([bad[0], bad[1]])
        assert e.value.status == capi.LDB_ERR_INVALID and "part 1" in str(e.value)


# ---------------------------------------------------------------- numbers and dates as text
@pytest.mark.parametrize("scale", [0, 2, 6, 7, 8, 38])
def test_decimal_parts_and_round_trip(ctx, scale):
    vals = DEC_VALUES + [None, 5, -5, 12, 99, 100, -(10 ** 38 - 1), 10 ** 38 - 1]
    t = reg(ctx, {"d": darr(vals, 38, scale)})
    r = t.rel()
    text = r.map_strcat([{"dec": (0, 0)}], name="txt")
    want = [None if v is None else E.from_decimal(v, scale) for v in vals]
    assert_utf8(text, want, "scale %d" % scale)
    assert_utf8(r.map_strcat(["<", {"dec": (0, 0)}, "|", {"dec": (0, 0)}, ">"]), E.strcat([b"<", {"dec": vals, "scale": scale}, b"|", {"dec": vals, "scale": scale}, b">"], len(vals)), "scale %d twice" % scale)
    # to_decimal(to_varchar(x), p, s) == x: arrow parses its own scientific form
    back, bad = r.zip(text).map_strparse((1, 0), capi.PARSE_DECIMAL, 38, scale)
    assert parsed_values(back, "decimal", 38, scale) == vals and bad == 0


@pytest.mark.parametrize("narrow", [0, 1, 2])
def test_decimal_parts_at_every_stored_width(ctx, narrow):
    vals = [0, 1, -1, 5, -5, 99, -100, 127, -128, 128, 32767, -32768, 32768, 2 ** 31 - 1, -(2 ** 31), 2 ** 31, 10 ** 12 - 1, -(10 ** 12 - 1), None, 10 ** 11]
    small = [0, 1, -1, 5, -5, 99, -100, 127, -128, None]
    t = reg(ctx, {"d": darr(vals, 12, 2), "e": darr(small * 2, 3, 1), "w": darr([v if v is None else v * 10 ** 20 for v in vals], 38, 8)}, narrow=narrow)
    r = t.rel()
    assert_utf8(r.map_strcat([{"dec": (0, 0)}]), [None if v is None else E.from_decimal(v, 2) for v in vals], "narrow %d (12,2)" % narrow)
    assert_utf8(r.map_strcat([{"dec": (0, 1)}]), [None if v is None else E.from_decimal(v, 1) for v in small * 2], "narrow %d (3,1)" % narrow)
    assert_utf8(r.map_strcat([{"dec": (0, 2)}]), [None if v is None else E.from_decimal(v * 10 ** 20, 8) for v in vals], "narrow %d (38,8)" % narrow)


def test_date_parts_and_round_trip(ctx):
    days = [E.DATE_MIN, E.DATE_MAX, E.DATE_MIN - 1, E.DATE_MAX + 1, 0, None, -25509, 11016, 12477, 47540, -1, 59, 60, -(2 ** 31), 2 ** 31 - 1] + [E.to_date(s) for s in ("1900-02-28", "1900-03-01", "2000-02-29", "2004-02-29", "2100-03-01")]
    t = reg(ctx, {"d": pa.array(days, pa.int32()).cast(pa.date32())})
    r = t.rel()
    text = r.map_strcat([{"date": (0, 0)}])
    want = [None if d is None else E.from_date(d) for d in days]
    assert want[:5] == [b"0001-01-01", b"9999-12-31", None, None, b"1970-01-01"]
    assert_utf8(text, want, "dates")
    back, bad = r.zip(text).map_strparse((1, 0), capi.PARSE_DATE)
    assert parsed_values(back, "date") == [None if w is None else d for d, w in zip(days, want)] and bad == 0
    # a DATE part makes the result nullable even over a column without NULLs
    t2 = reg(ctx, {"d": pa.array([0, E.DATE_MAX + 1, 1], pa.int32()).cast(pa.date32())}, "strcast_d2")
    assert_utf8(t2.rel().map_strcat(["[", {"date": (0, 0)}, "]"]), [b"[1970-01-01]", None, b"[1970-01-02]"], "nullable by range")


def test_int_round_trip(ctx):
    vals = [0, 1, -1, 2 ** 63 - 1, -(2 ** 63), None, 10 ** 18, -(10 ** 18), 99999999, 100000000, 9999999999999999, 10 ** 16]
    t = reg(ctx, {"k": pa.array(vals, pa.int64())})
    r = t.rel()
    text = r.map_strcat([{"int": (0, 0)}])
    assert_utf8(text, [None if v is None else E.from_int(v) for v in vals], "ints")
    back, bad = r.zip(text).map_strparse((1, 0), capi.PARSE_INT64)
    assert parsed_values(back, "int") == vals and bad == 0


def test_number_parts_across_words_tiles_and_staged_offsets(ctx, geom):
    T, R = geom
    # a constant of T - 5 bytes in front: the decimal and the date behind it straddle a 16-byte word and the tile boundary
    dec = [-123456789012345678901234567890123456, 1, None, 10 ** 37, -5, 99]
    day = [0, E.DATE_MAX, 11016, None, E.DATE_MIN, E.DATE_MAX + 1]
    t = reg(ctx, {"d": darr(dec, 38, 8), "e": pa.array(day, pa.int32()).cast(pa.date32()), "k": pa.array([7, -8, 9, 10, None, 12], pa.int64())})
    r = t.rel()
    for front in (T - 5, T - 21, 2 * T - 1, 11):
        c = b"c" * front
        assert_utf8(r.map_strcat([c, {"dec": (0, 0)}, {"date": (0, 1)}, {"int": (0, 2)}]), E.strcat([c, {"dec": dec, "scale": 8}, {"date": day}, {"int": [7, -8, 9, 10, None, 12]}], len(dec)), "front %d" % front)
    # 2 R + 300 one-byte rows (a decimal of one digit) before a long one, and date rows (ten bytes) behind it
    n1 = 2 * R + 300
    dv = [i % 10 for i in range(n1)] + [-(10 ** 37)] + [3] * 40
    sv = [""] * n1 + ["L" * (T + 9)] + ["xy"] * 40
    ev = [None] * n1 + [0] + [11016 + i for i in range(40)]
    t2 = reg(ctx, {"d": darr(dv, 38, 0), "s": sarr(sv), "e": pa.array([0 if v is None else v for v in ev], pa.int32()).cast(pa.date32())}, "strcast_runs", dict_encode=False)
    r2 = t2.rel()
    assert_utf8(r2.map_strcat([{"dec": (0, 0)}, {"col": (0, 1)}]), E.strcat([{"dec": dv, "scale": 0}, {"col": [tobytes(x) for x in sv]}], len(dv)), "runs of one-byte rows")
    days2 = [0 if v is None else v for v in ev]
    assert_utf8(r2.map_strcat([{"date": (0, 2)}, {"dec": (0, 0)}]), E.strcat([{"date": days2}, {"dec": dv, "scale": 0}], len(dv)), "date || dec")


def test_mixed_parts_with_nulls_in_each(ctx):
    n = 300
    dec = [None if i % 31 == 3 else (-1) ** i * (i * 7919 + 10 ** (i % 20)) for i in range(n)]
    col = [None if i % 37 == 5 else "s%d" % (i * i) for i in range(n)]
    day = [None if i % 41 == 7 else -719000 + i * 12300 for i in range(n)]  # (the last ones are past 9999-12-31: NULL by range)
    k = [None if i % 43 == 9 else (-1) ** i * 3 ** (i % 39) for i in range(n)]
    assert any(d is not None and d > E.DATE_MAX for d in day)
    t = reg(ctx, {"d": darr(dec, 30, 6), "s": sarr(col), "e": pa.array(day, pa.int32()).cast(pa.date32()), "k": pa.array(k, pa.int64())})
    got = t.rel().map_strcat(["id=", {"dec": (0, 0)}, {"col": (0, 1)}, {"date": (0, 2)}, {"int": (0, 3)}])
    assert_utf8(got, E.strcat([b"id=", {"dec": dec, "scale": 6}, {"col": [tobytes(x) for x in col]}, {"date": day}, {"int": k}], n), "const || dec || col || date || int")


# ---------------------------------------------------------------- the plan language
def test_plan_steps(ctx):
    n = 200
    dec = [None if i % 17 == 1 else (-1) ** i * i * 977 for i in range(n)]
    day = [None if i % 19 == 2 else 10000 + i for i in range(n)]
    k = [(-1) ** i * i * 31 for i in range(n)]
    txt = ["%d.%02d" % (i, i % 100) for i in range(n)]
    txt[5], txt[50], txt[51] = "1.234", "x", None
    t = reg(ctx, {"p": darr(dec, 12, 2), "d": pa.array(day, pa.int32()).cast(pa.date32()), "k": pa.array(k, pa.int64()), "k32": pa.array(k, pa.int32()), "s": sarr(txt)}, "strcast_plan")

    def run(steps, cols):
        plan = json.dumps({"inputs": ["t"], "steps": steps + [{"op": "materialize", "in": steps[-1]["out"], "cols": cols, "out": "result"}], "result": "result"})
        return ctx.run_plan(plan, {"t": t}).to_arrow()

    res = run([{"op": "map", "in": "t", "fn": "to_varchar", "col": "p", "as": "tp", "out": "r1"}, {"op": "map", "in": "r1", "fn": "to_varchar", "col": "d", "as": "td", "out": "r2"},
               {"op": "map", "in": "r2", "fn": "to_varchar", "col": "k", "as": "tk", "out": "r3"}, {"op": "map", "in": "r3", "fn": "to_varchar", "col": "k32", "as": "tk32", "out": "r4"},
               {"op": "map", "in": "r4", "fn": "concat", "as": "c", "out": "r5", "parts": [{"dec": "p"}, {"const": "@"}, {"date": "d"}]}],
              ["tp", "td", "tk", "tk32", "c"])  # (a relation has at most six sides: the table and five computed columns)
    dec_s = lambda v: None if v is None else v.decode()  # noqa: E731
    assert res.column(0).to_pylist() == [None if v is None else E.from_decimal(v, 2).decode() for v in dec]
    assert res.column(1).to_pylist() == [None if v is None else E.from_date(v).decode() for v in day]
    assert res.column(2).to_pylist() == [str(v) for v in k] and res.column(3).to_pylist() == [str(v) for v in k]
    assert res.column(4).to_pylist() == [dec_s(v) for v in E.strcat([{"dec": dec, "scale": 2}, b"@", {"date": day}], n)]
    res = run([{"op": "map", "in": "t", "fn": "to_varchar", "col": "d", "as": "td", "out": "r1"}, {"op": "map", "in": "r1", "fn": "to_varchar", "col": "k", "as": "tk", "out": "r2"},
               {"op": "map", "in": "r2", "fn": "to_decimal", "col": "s", "precision": 12, "scale": 2, "on_error": "null", "as": "v", "out": "r3"},
               {"op": "map", "in": "r3", "fn": "to_date", "col": "td", "as": "d2", "out": "r4"}, {"op": "map", "in": "r4", "fn": "to_int", "col": "tk", "as": "k2", "out": "r5"}],
              ["v", "d2", "k2"])
    want, bad = E.parse_column("decimal", [tobytes(s) for s in txt], 12, 2)
    assert bad == 2 and [None if v is None else int(v.scaleb(2)) for v in res.column(0).to_pylist()] == want
    assert res.column(1).cast(pa.int32()).to_pylist() == day and res.column(2).to_pylist() == k
    # on_error "fail" (the default): the step fails as the reference's throw would, and says how many rows
    for extra in ({}, {"on_error": "fail"}):
        with pytest.raises(capi.LdbError) as e:
            run([dict({"op": "map", "in": "t", "fn": "to_decimal", "col": "s", "precision": 12, "scale": 2, "as": "v", "out": "r1"}, **extra)], ["v"])
        assert e.value.status == capi.LDB_ERR_INVALID and "2 bad rows" in str(e.value), str(e.value)
    with pytest.raises(capi.LdbError) as e:
        run([{"op": "map", "in": "t", "fn": "to_varchar", "col": "s", "as": "v", "out": "r1"}], ["v"])
    assert "to_varchar" in str(e.value) and "type %d" % capi.T_UTF8 in str(e.value)
