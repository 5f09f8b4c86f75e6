"""The inputs of tests/test_gpu_setwin_edges.py, before any device sees them: the generators of setwin_ref hold the sizes and special values they
claim, the oracle's ora_window / ora_setop_multiplicity (oracle/ldb_oracle.c, the checker of the GPU suite) give exactly what setwin_ref's plain
slices and counters give for every case, and setwin_ref.window reproduces the answers of the reference's real SegmentTreeView
(tests/golden/ref_segtree.npz).  No GPU."""
import collections
import os

import numpy as np
import pyarrow as pa
import pytest

import golden_io
import oracle_bind
import setwin_ref as sw

SET = {c["name"]: c for c in sw.set_cases()}
WIN = {c["name"]: c for c in sw.window_cases()}
P, F = sw.P, sw.F


def set_rows(case):
    (ls, _), (rs, _) = sw.rel_sides(case["left"]), sw.rel_sides(case["right"])
    return sw.rel_rows(ls, case["lcols"]), sw.rel_rows(rs, case["rcols"])


def col0(case, side):
    return [r[0] for r in set_rows(case)[0 if side == "left" else 1]]


# ---------------------------------------------------------------- the generators
def test_the_set_generator_holds_what_it_claims():
    assert len(SET) == sum(1 for _ in sw.set_cases()) and not set(SET) & set(WIN)
    for case in SET.values():
        for rel in (case["left"], case["right"]):
            assert all(t.num_rows <= sw.MAX_ROWS for t in sw.rel_tables(rel))
        assert tuple(case["ops"]) == sw.ALL_OPS
    # ---- types
    for ty in ("int32", "int64", "date32", "dec12_2", "dec38_0", "utf8", "float64", "dec12_2_narrow"):
        l, r = set_rows(SET["type_" + ty])
        assert set(l) & set(r) and set(l) - set(r) and set(r) - set(l), ty  # rows on both sides and on one side only
    assert min(col0(SET["type_date32"], "left")) < 0
    d38 = set(col0(SET["type_dec38_0"], "left")) | set(col0(SET["type_dec38_0"], "right"))
    assert {2 ** 64, -(2 ** 64), 2 ** 64 + 1, -(2 ** 64) - 1, 2 ** 64 - 1, 1 - 2 ** 64} <= d38
    assert {2 ** 64 + 5, 2 * 2 ** 64 + 5} <= d38 and {7 * 2 ** 64 + 1, 7 * 2 ** 64 + 2} <= d38  # differ in the high word only / in the low word only
    s = set(col0(SET["type_utf8"], "left")) | set(col0(SET["type_utf8"], "right"))
    assert {b"", b"a", b"a\0", b"ab", b"\x80", b"\xff\xfe"} <= s and {13, 300} <= {len(v) for v in s}
    long = [v for v in s if len(v) in (53, 300)]
    assert len(long) == 3 and all(v[:40] == sw.PREFIX40 for v in long)
    f = col0(SET["type_float64"], "left") + col0(SET["type_float64"], "right")
    assert all(v == v for v in f) and 0.0 in f and not any(v == 0.0 and np.signbit(v) for v in f)  # no NaN, one sign of zero
    assert [f.type for f in SET["three_columns"]["left"]["table"].schema] == [pa.int32(), pa.string(), pa.decimal128(12, 2)]
    # ---- NULLs
    for na in (7, 8, 9):
        for which, (lnull, rnull) in (("left", (True, False)), ("right", (False, True)), ("both", (True, True))):
            case = SET["null_%s_na%d" % (which, na)]
            lt, rt = case["left"]["table"], case["right"]["table"]
            assert lt.num_rows == na and (lt.column(0).null_count > 0) == lnull and (rt.column(0).null_count > 0) == rnull
            assert (lt.column(0).chunk(0).buffers()[0] is not None) == lnull and (rt.column(0).chunk(0).buffers()[0] is not None) == rnull
    assert set(col0(SET["null_all_left"], "left")) == {None} and set(col0(SET["null_all_right"], "right")) == {None}
    l, r = map(collections.Counter, set_rows(SET["null_pairs"]))
    assert set(l) == set(r) == {(1, None), (None, 1), (None, None), (1, 1)} and all(l[k] != r[k] for k in l)
    assert {None, b""} <= set(col0(SET["null_vs_empty"], "left")) and {None, 0} <= set(col0(SET["null_vs_zero"], "left"))
    # ---- sizes
    size = lambda name: tuple(len(x) for x in set_rows(SET[name]))
    assert size("empty_both") == (0, 0) and size("empty_left")[0] == 0 < size("empty_left")[1] and size("empty_right")[1] == 0 < size("empty_right")[0]
    assert size("one_one_same") == size("one_one_other") == (1, 1)
    assert sum(size("lds_1000")) == 1000 and sum(size("lds_overflow_5000")) == 5000
    l, r = set_rows(SET["lds_overflow_5000"])
    assert 3500 < len(set(l) | set(r)) < 4500
    for name in ("direct_12000", "sorted_12000_seam_mid", "sorted_12000_seam_chunk", "outlier_12000", "hashed_12000", "pairs_12000", "mult_zero_runs"):
        assert sum(size(name)) == 12000, name
    k = col0(SET["direct_12000"], "left") + col0(SET["direct_12000"], "right")
    assert max(k) - min(k) < 6000 and None not in k and k != sorted(k) and SET["direct_12000"]["path"] == "k_groupby_direct"
    for seam, nl in (("mid", 6390), ("chunk", 6400)):
        case = SET["sorted_12000_seam_" + seam]
        l, r = col0(case, "left"), col0(case, "right")
        assert len(l) == nl and l == sorted(l) and r == sorted(r) and r[0] == l[-1] and None not in l + r and case["path"] == "k_gb_sorted_heads"
        k = l + r
        heads = {i for i in range(1, 12000) if k[i] != k[i - 1]}
        assert {64, 128, 256, 320, 384, 448, 640, 704} <= heads and nl not in heads  # runs that begin and end on chunk boundaries; one group spans the seam
    k = col0(SET["outlier_12000"], "left")
    assert max(k) == 2 ** 31 - 5 and sorted(k)[-2] < 50000
    k = col0(SET["hashed_12000"], "left")
    assert max(k) - min(k) >= 2 ** 32
    assert len(SET["pairs_12000"]["lcols"]) == 2
    # ---- multiplicities
    l, r = map(collections.Counter, set_rows(SET["mult_3000_1"]))
    assert (l[(11,)], r[(11,)]) == (3000, 1) and (l[(22,)], r[(22,)]) == (1, 3000) and l[(33,)] == r[(33,)] == 5 and (44,) not in r and (55,) not in l
    l, r = set_rows(SET["mult_zero_runs"])
    for op in (sw.EXCEPT_ALL, sw.INTERSECT_ALL):
        res = sw.set_op(l, r, op)
        assert set(res) == {(0,), (500,), (1002,)} and all(500 <= m <= 3000 for m in res.values())
    assert len(set(l) | set(r)) == 1003 and min(set(l) | set(r)) == (0,) and max(set(l) | set(r)) == (1002,)
    l, r = set_rows(SET["empty_left"])
    assert all(not sw.set_op(l, r, op) for op in (sw.INTERSECT, sw.INTERSECT_ALL, sw.EXCEPT, sw.EXCEPT_ALL)) and sw.set_op(l, r, sw.UNION)
    # ---- relations
    assert SET["rel_filter_left"]["left"]["kind"] == "filter" and 0 < len(set_rows(SET["rel_filter_left"])[0]) < 900
    case = SET["rel_louter_right"]
    sides, n = sw.rel_sides(case["right"])
    assert case["right"]["kind"] == "louter" and (sides[1][1] == sw.NULL_ROW).any() and all(s == 1 for s, _ in case["rcols"])
    l, r = set_rows(case)
    assert (None, None) in l and (None, None) in r and any(a is None and b is not None for a, b in r)  # padding and a NULL of the build table itself
    assert SET["cols_other_positions"]["lcols"] != SET["cols_other_positions"]["rcols"] and SET["cols_reordered_pair"]["rcols"] == SET["cols_reordered_pair"]["lcols"][::-1]
    assert SET["same_table"]["left"]["table"] is SET["same_table"]["right"]["table"]
    assert SET["dict_left"]["dict"] == "left" and SET["dict_right"]["dict"] == "right"
    assert len(SET["eight_columns"]["lcols"]) == 8
    assert {c["name"] for c in SET.values() if c["spec"]} == {"lds_1000", "lds_overflow_5000", "direct_12000", "sorted_12000_seam_mid", "outlier_12000", "hashed_12000", "pairs_12000"}
    assert [(name, len(lc), op, code) for name, _, lc, _, _, op, code in sw.set_refusals()] == [
        ("nine_columns", 9, sw.UNION, "LDB_ERR_INVALID"), ("int32_against_int64", 1, sw.INTERSECT, "LDB_ERR_INVALID"), ("dec12_2_against_dec12_3", 1, sw.UNION_ALL, "LDB_ERR_INVALID"),
        ("operation_6", 1, 6, "LDB_ERR_INVALID")]


def test_the_window_generator_holds_what_it_claims():
    assert len(WIN) == sum(1 for _ in sw.window_cases())
    for case in WIN.values():
        assert all(t.num_rows <= sw.MAX_ROWS for t in sw.rel_tables(case["rel"])) and len(case["fns"]) <= 8
        assert all(abs(o) < 2 ** 62 for fr in case["frames"] for o in fr if o not in (P, F))
    for n in sw.SINGLE_SIZES:
        case = WIN["single_%d" % n]
        assert case["rel"]["table"].num_rows == n and not case["part"] and [fn for fn, _ in case["fns"]] == list(sw.FNS6)
        assert case["frames"] == [(P, 0), (P, F), (0, F), (0, 0), (-1, 1), (-3, -1), (1, 3), (-n, n), (-(2 ** 40), 2 ** 40), (5, F), (P, -5)]
        assert case["rel"]["table"].column(1).null_count == len(range(1, n, 6)) and case["rel"]["table"].schema.field(1).type == pa.int64()
    assert sw.SINGLE_SIZES == (1, 2, 3, 63, 64, 65, 255, 256, 257, 4096, 4097, 8193)
    _, start, end, _ = sw.window_layout(WIN["part_sizes"])
    bounds = sorted(set(start))
    assert sorted(np.diff(bounds + [len(start)]).tolist()) == sorted([1, 1, 2, 63, 64, 65, 1, 700, 1, 256, 255, 257, 1])
    assert {256, 512} <= set(bounds) and {576, 640, 1408} <= set(bounds)  # multiples of 256 and of 64 of the sorted position
    _, start, end, _ = sw.window_layout(WIN["part_5000_of_one_row"])
    assert start == list(range(5000)) and end == list(range(1, 5001))
    t = WIN["part_key_i32_utf8"]["rel"]["table"]
    assert [f.type for f in t.schema][:2] == [pa.int32(), pa.string()] and t.column(0).null_count and t.column(1).null_count
    for ty, want in (("utf8", pa.string()), ("dec38_0", pa.decimal128(38, 0)), ("date32", pa.date32())):
        t = WIN["part_key_" + ty]["rel"]["table"]
        assert t.schema.field(0).type == want and t.column(0).null_count and WIN["part_key_" + ty]["part"] == [(0, 0)]
    arg = lambda name: sw.column_values(WIN["arg_" + name]["rel"]["table"].column(2))
    assert {2 ** 31 - 1, -(2 ** 31)} <= set(arg("int32_extremes")) and WIN["arg_int32_extremes"]["rel"]["table"].schema.field(2).type == pa.int32()
    assert {2 ** 62, -(2 ** 62)} <= set(arg("int64_wraps"))
    _, start, end, args = sw.window_layout(WIN["arg_int64_wraps"])
    assert any(not -(2 ** 63) <= sum(v for v in args[(0, 2)][s:e] if v is not None) < 2 ** 63 for s, e in set(zip(start, end)))  # the true sum leaves 64 bits
    assert min(v for v in arg("date32") if v is not None) < 0 and sw.SUM not in [fn for fn, _ in WIN["arg_date32"]["fns"]]
    assert WIN["arg_dec12_2"]["rel"]["table"].schema.field(2).type == pa.decimal128(12, 2) and WIN["arg_dec12_2_narrow"]["narrow"]
    _, start, end, args = sw.window_layout(WIN["arg_dec38_0"])
    v = args[(0, 2)]
    sums = [s for frm, to in ((P, 0), (-3, 3)) for s in sw.window(v, None, start, end, sw.SUM, frm, to) if s is not None]
    assert any(s > 2 ** 64 for s in sums) and any(0 < s < 2 ** 64 for s in sums) and any(-(2 ** 64) < s < 0 for s in sums) and any(s < -(2 ** 64) for s in sums)  # on either side of +2^64 and of -2^64
    assert {5 * 2 ** 64 + 9, 6 * 2 ** 64 + 9, 5 * 2 ** 64 + 8} <= set(v)  # ties in the low word / in the high word
    assert set(arg("all_null")) == {None} and None not in arg("no_nulls") and WIN["arg_no_nulls"]["rel"]["table"].column(2).null_count == 0
    _, start, end, args = sw.window_layout(WIN["arg_null_partition"])
    assert None not in args[(0, 2)][:200] and set(args[(0, 2)][200:]) == {None} and end[0] == 200
    o = sw.column_values(WIN["order_ties"]["rel"]["table"].column(0))
    assert len(set(o)) == 5
    assert [(d, nl) for _, _, d, nl in WIN["order_two_keys_second_desc"]["order"]] == [(False, 0), (True, 0)]
    for way, desc in (("asc", False), ("desc", True)):
        case = WIN["order_nullable_" + way]
        assert case["order"] == [(0, 1, desc, sw.NULLS_LARGEST)] and case["rel"]["table"].column(1).null_count
    for name, lo, hi in (("rel_filter", 4097, 7000), ("rel_filter_small", 1, 4096)):
        assert WIN[name]["rel"]["kind"] == "filter" and lo <= sw.rel_sides(WIN[name]["rel"])[1] < hi and WIN[name]["spec"]
    assert {c["name"] for c in WIN.values() if c["spec"]} == {"rel_filter", "rel_filter_small"}
    for name, ref in (("rel_louter_arg", WIN["rel_louter_arg"]["fns"][0][1]), ("rel_louter_part_key", WIN["rel_louter_part_key"]["part"][0])):
        sides, n = sw.rel_sides(WIN[name]["rel"])
        assert ref[0] == 1 and (sides[1][1] == sw.NULL_ROW).any()
    fns = WIN["eight_functions"]["fns"]
    assert len(fns) == 8 and collections.Counter(c for _, c in fns)[(0, 2)] == 4
    assert all(a > b for a, b in WIN["inverted_frames"]["frames"])
    assert [(name, code) for name, _, _, _, _, code in sw.window_refusals()] == [
        ("order_nulls_refused", "LDB_ERR_UNSUPPORTED"), ("nine_functions", "LDB_ERR_INVALID"), ("sum_over_date32", "LDB_ERR_INVALID"), ("float64_argument", "LDB_ERR_UNSUPPORTED"),
        ("function_6", "LDB_ERR_INVALID"), ("nine_partition_keys", "LDB_ERR_INVALID")]
    r = {name: (part, fns) for name, _, part, _, fns, _ in sw.window_refusals()}
    assert len(r["nine_functions"][1]) == 9 and len(r["nine_partition_keys"][0]) == 9 and r["function_6"][1][0][0] == 6


# ---------------------------------------------------------------- the oracle against the plain statements
@pytest.mark.parametrize("name", list(WIN))
def test_oracle_window_equals_the_plain_slices(oracle, name):
    case = WIN[name]
    order, start, end, args = sw.window_layout(case)
    for frm, to in case["frames"]:
        for col in list(args) + [None]:
            fns = [fn for fn, c in case["fns"] if c == col]
            if not fns:
                continue
            bits = sw.sum_bits_of(sw.arg_type(case, col)) if col is not None else 64
            vals = args[col] if col is not None else None
            want = sw.window_all(vals, None, start, end, fns, frm, to, bits)
            for fn in fns:
                got = oracle_bind.window(oracle, None if vals is None else [v or 0 for v in vals], None if vals is None else [v is not None for v in vals], start, end, fn, frm, to)
                if fn == sw.SUM:  # the oracle accumulates in 128 bits; the result column of an int32 / int64 argument keeps the low 64
                    got = [None if v is None else sw.wrap(v, bits) for v in got]
                assert got == want[fn], (frm, to, fn, col)


@pytest.mark.parametrize("name", list(SET))
def test_oracle_set_multiplicities_equal_the_plain_counters(oracle, name):
    l, r = set_rows(SET[name])
    cl, cr = collections.Counter(l), collections.Counter(r)
    for op in SET[name]["ops"]:
        got = collections.Counter()
        for row in set(cl) | set(cr):
            m = oracle.lib.ora_setop_multiplicity(op, cl.get(row, 0), cr.get(row, 0))
            if m:
                got[row] = m
        assert got == sw.set_op(l, r, op), op


def test_plain_window_reproduces_the_reference_segment_tree():
    """tests/golden/ref_segtree.npz: ten frames over one partition, answered by the reference's real SegmentTreeView"""
    z = np.load(os.path.join(golden_io.GOLDEN, "ref_segtree.npz"))
    vals, valid = [int(v) for v in z["vals"]], z["valid"].tolist()
    n = len(vals)
    frames = z["frames"].tolist()
    assert len(frames) == 10
    for fi, (frm, to) in enumerate(frames):
        for fn in (sw.SUM, sw.MIN, sw.MAX, sw.COUNT):
            want = [int(v) if (ok or fn == sw.COUNT) else None for v, ok in zip(z["f%d_fn%d_val" % (fi, fn)].tolist(), z["f%d_fn%d_ok" % (fi, fn)].tolist())]
            assert sw.window(vals, valid, [0] * n, [n] * n, fn, frm, to, 64) == want, (fi, fn)


# ---------------------------------------------------------------- answers written out
def test_hand_made_rows():
    l = [(1, b"a"), (1, b"a"), (1, b"a"), (None, None), (None, None), (2, b""), (2, None), (7, b"x")]
    r = [(1, b"a"), (None, None), (None, None), (None, None), (2, None), (2, None), (5, b"e")]
    C = collections.Counter
    assert sw.set_op(l, r, sw.UNION_ALL) == C(l + r)
    assert sw.set_op(l, r, sw.UNION) == C({(1, b"a"): 1, (None, None): 1, (2, b""): 1, (2, None): 1, (7, b"x"): 1, (5, b"e"): 1})
    assert sw.set_op(l, r, sw.INTERSECT) == C({(1, b"a"): 1, (None, None): 1, (2, None): 1})
    assert sw.set_op(l, r, sw.INTERSECT_ALL) == C({(1, b"a"): 1, (None, None): 2, (2, None): 1})
    assert sw.set_op(l, r, sw.EXCEPT) == C({(2, b""): 1, (7, b"x"): 1})
    assert sw.set_op(l, r, sw.EXCEPT_ALL) == C({(1, b"a"): 2, (2, b""): 1, (7, b"x"): 1})
    assert sw.set_op([], r, sw.EXCEPT_ALL) == C() and sw.set_op(l, [], sw.INTERSECT) == C()
    # window order: partition key ascending with NULL last, then o descending with NULL first (NULL is the largest value), then the position
    t = pa.table({"p": pa.array([1, None, 0, 1, None, 0, 1], pa.int32()), "o": pa.array([5, 1, None, 5, 2, 3, None], pa.int64())})
    assert sw.window_order(t, [0], [(1, True, sw.NULLS_LARGEST)]).tolist() == [2, 5, 6, 0, 3, 4, 1]
    assert sw.window_order(t, [0], [(1, False, sw.NULLS_LARGEST)]).tolist() == [5, 2, 0, 3, 6, 1, 4]
    with pytest.raises(ValueError):
        sw.window_order(t, [0], [(1, False, sw.NULLS_REFUSE)])
    # two partitions [0, 3) and [3, 5): 4, NULL, -1 | NULL, NULL
    v, ok = [4, 99, -1, 99, 99], [1, 0, 1, 0, 0]
    ps, pe = [0, 0, 0, 3, 3], [3, 3, 3, 5, 5]
    w = lambda fn, frm, to, bits=64: sw.window(v, ok, ps, pe, fn, frm, to, bits)
    assert w(sw.SUM, P, 0) == [4, 4, 3, None, None] and w(sw.SUM, P, F) == [3, 3, 3, None, None]
    assert w(sw.MIN, -1, 1) == [4, -1, -1, None, None] and w(sw.MAX, 0, F) == [4, -1, -1, None, None]
    assert w(sw.COUNT, P, F) == [2, 2, 2, 0, 0] and w(sw.COUNT_STAR, -1, 0) == [1, 2, 2, 1, 2] and w(sw.RANK, P, 0) == [1, 2, 3, 1, 2]
    assert w(sw.SUM, 5, F) == [-1, -1, -1, None, None] and w(sw.COUNT_STAR, 5, F) == [1, 1, 1, 1, 1]  # both ends clamp to the last row
    assert w(sw.SUM, P, -5) == [4, 4, 4, None, None] and w(sw.RANK, -1, 1) == [1, 2, 2, 1, 2]
    # an inverted frame is empty unless clamping brings the ends together
    assert w(sw.COUNT_STAR, 1, 0) == [0, 0, 1, 0, 1] and w(sw.SUM, 1, 0) == [None, None, -1, None, None] and w(sw.COUNT, 1, 0) == [0, 0, 1, 0, 0]
    assert w(sw.MIN, 2, 1)[0] is None and w(sw.MAX, 2, 1)[0] is None and w(sw.RANK, 1, 0) == [0, 0, 1, 0, 1]
    # SUM wraps to the width of the result column
    big, one = [2 ** 63 - 1, 1, 1], [1, 1, 1]
    assert sw.window(big, one, [0] * 3, [3] * 3, sw.SUM, P, 0, 64) == [2 ** 63 - 1, -(2 ** 63), -(2 ** 63) + 1]
    assert sw.window(big, one, [0] * 3, [3] * 3, sw.SUM, P, 0, 128) == [2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1]
    assert sw.window([2 ** 127 - 1, 1], [1, 1], [0, 0], [2, 2], sw.SUM, P, 0, 128) == [2 ** 127 - 1, -(2 ** 127)]
