"""Plain-Python statement of the set operations and the window functions (csrc/ldb_setops.hip) — TEST INFRASTRUCTURE, no device, no oracle.

  * set_op: the multiplicities of the header comment of ldb_gpu_set_op (include/lingodb_gpu.h), on collections.Counter; rows are tuples of Python
    values (ints, unscaled decimal ints, bytes, None for NULL), so NULL = NULL is tuple equality;
  * window_order: (PARTITION BY keys ascending, NULL the largest value) then the ORDER BY keys with their own `nulls`, then the input position —
    the comparator is null_order_ref's, nothing is restated here;
  * window: every frame is a Python slice of its partition; sum / min / max / count of what is not None.  No tree, no prefix sums.
A relation is described by a small dict (`table_rel`, `filter_rel`, `louter_rel`) that the device test turns into api.Rel objects and `rel_sides`
into [(pyarrow table, row ids or None)]: a row id of 0xFFFFFFFF is outer-join padding, every column of that side is NULL there.
`set_cases()` / `window_cases()` / `set_refusals()` / `window_refusals()` own the seeded inputs of tests/test_setwin_edges.py (no device) and
tests/test_gpu_setwin_edges.py (device): both see the same tables.  Seeds are fixed; nothing here reads a clock or the environment."""
import collections

import numpy as np
import pyarrow as pa

import null_order_ref
import order_ref

NULL_ROW = null_order_ref.NULL_ROW
I64_MIN, I64_MAX = order_ref.I64_MIN, order_ref.I64_MAX
P, F = I64_MIN, I64_MAX  # unbounded preceding / following
UNION_ALL, UNION, INTERSECT, INTERSECT_ALL, EXCEPT, EXCEPT_ALL = range(6)  # ldb_set_op
ALL_OPS = (UNION_ALL, UNION, INTERSECT, INTERSECT_ALL, EXCEPT, EXCEPT_ALL)
RANK, SUM, MIN, MAX, COUNT, COUNT_STAR = range(6)  # ldb_window_fn_kind
NULLS_REFUSE, NULLS_LARGEST = 0, 1  # ldb_null_order
MAX_ROWS = 20000
PREFIX40 = order_ref.PREFIX40
with_validity, str_array, dec_array, column_values = null_order_ref.with_validity, order_ref.str_array, order_ref.dec_array, null_order_ref.column_values


# ------------------------------------------------------------------ relations
def table_rel(table):
    return {"kind": "table", "table": table}


def filter_rel(table, col, op, value):
    """rows of `table` whose column `col` is not NULL and `op` ("GTE", "LT", "EQ", "NEQ") `value`, in input order"""
    return {"kind": "filter", "table": table, "col": col, "op": op, "value": value}


def louter_rel(probe, build, pkey, bkey):
    """probe LEFT OUTER JOIN build ON probe.pkey = build.bkey: side 0 = probe rows, side 1 = build rows or padding"""
    return {"kind": "louter", "probe": probe, "build": build, "pkey": pkey, "bkey": bkey}


_CMP = {"GTE": lambda a, b: a >= b, "LT": lambda a, b: a < b, "EQ": lambda a, b: a == b, "NEQ": lambda a, b: a != b}


def rel_tables(spec):
    return [spec["probe"], spec["build"]] if spec["kind"] == "louter" else [spec["table"]]


def rel_sides(spec):
    """→ ([(table, row ids or None)], number of rows).  The pair order of a join is probe order, then build order: the device may produce
    another one, so the device test passes the row ids it read back to `sides_from` instead."""
    if spec["kind"] == "table":
        return [(spec["table"], None)], spec["table"].num_rows
    if spec["kind"] == "filter":
        vals = column_values(spec["table"].column(spec["col"]))
        ids = np.array([i for i, v in enumerate(vals) if v is not None and _CMP[spec["op"]](v, spec["value"])], dtype=np.uint32)
        return [(spec["table"], ids)], len(ids)
    pk, bk = column_values(spec["probe"].column(spec["pkey"])), column_values(spec["build"].column(spec["bkey"]))
    where = collections.defaultdict(list)
    for j, v in enumerate(bk):
        if v is not None:
            where[v].append(j)
    p, b = [], []
    for i, v in enumerate(pk):
        for j in (where.get(v) if v is not None and v in where else [NULL_ROW]):
            p.append(i), b.append(j)
    return sides_from(spec, [np.array(p, dtype=np.uint32), np.array(b, dtype=np.uint32)])


def sides_from(spec, rowids):
    return [(t, r) for t, r in zip(rel_tables(spec), rowids)], len(rowids[0])


def rel_column(sides, ref):
    side, col = ref
    return null_order_ref.side_values(sides[side][0], col, sides[side][1])


def rel_rows(sides, cols):
    """the listed columns of a relation as row tuples"""
    return list(zip(*[rel_column(sides, c) for c in cols])) if cols else []


def table_rows(table):
    return list(zip(*[column_values(c) for c in table.columns])) if table.num_rows else []


# ------------------------------------------------------------------ set operations
def set_op(left_rows, right_rows, op):
    """result rows of `left OP right` with their multiplicities (ldb_gpu_set_op: per distinct row l = copies on the left, r = copies on the right)"""
    cl, cr = collections.Counter(left_rows), collections.Counter(right_rows)
    out = collections.Counter()
    for row in set(cl) | set(cr):
        l, r = cl.get(row, 0), cr.get(row, 0)
        if op == UNION_ALL:
            k = l + r  # every row of both inputs
        elif op == UNION:
            k = 1
        elif op == INTERSECT:
            k = 1 if l > 0 and r > 0 else 0
        elif op == EXCEPT:
            k = 1 if l > 0 and r == 0 else 0
        elif op == INTERSECT_ALL:
            k = min(l, r)
        elif op == EXCEPT_ALL:
            k = max(l - r, 0)
        else:
            raise ValueError(op)
        if k:
            out[row] = k
    return out


# ------------------------------------------------------------------ window functions
def window_order_values(part_vals, order_keys, n):
    """positions 0..n-1 in window order; part_vals = [values], order_keys = [(values, descending, nulls)]"""
    for vals, _, nulls in order_keys:
        if nulls == NULLS_REFUSE and any(v is None for v in vals):
            raise ValueError("a NULL in an ORDER BY key that refuses them")
    return null_order_ref.sort_values([(v, False) for v in part_vals] + [(v, desc) for v, desc, _ in order_keys], n)


def window_order(table, part_keys, order_specs):
    """row numbers of `table` in window order; part_keys = [column], order_specs = [(column, descending, nulls)]"""
    return window_order_values([column_values(table.column(c)) for c in part_keys], [(column_values(table.column(c)), d, nl) for c, d, nl in order_specs], table.num_rows)


def partitions(part_vals, order, n):
    """(part_start, part_end) per row of the ordered input: rows with equal partition keys (NULL = NULL) are one partition; end is exclusive"""
    keys = [tuple(v[int(r)] for v in part_vals) for r in order]
    start, end = [0] * n, [n] * n
    for i in range(1, n):
        start[i] = start[i - 1] if keys[i] == keys[i - 1] else i
    for i in range(n - 2, -1, -1):
        end[i] = end[i + 1] if keys[i] == keys[i + 1] else i + 1
    return start, end


def wrap(v, bits):
    """two's complement at `bits` bits"""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def window_all(values, valid, part_start, part_end, fns, frm, to, sum_bits=128):
    """{fn: [value or None per row]} — the frame of row i is the slice [lo, hi] of its partition [part_start[i], part_end[i]): an end is the
    partition's begin / end when unbounded, else current row + offset clamped into the partition.  lo > hi (an inverted frame) is the empty slice."""
    n = len(part_start)
    vals = [v if (valid is None or valid[i]) else None for i, v in enumerate(values)] if values is not None else [None] * n
    out = {fn: [] for fn in fns}
    for i in range(n):
        st, last = part_start[i], part_end[i] - 1
        lo = st if frm == I64_MIN else min(max(i + frm, st), last)
        hi = last if to == I64_MAX else min(max(i + to, st), last)
        frame = vals[lo : hi + 1]
        there = [v for v in frame if v is not None]
        for fn in fns:
            if fn == RANK:
                r = i - lo + 1
            elif fn == COUNT_STAR:
                r = len(frame)
            elif fn == COUNT:
                r = len(there)
            elif not there:
                r = None
            elif fn == SUM:
                r = wrap(sum(there), sum_bits)
            else:
                r = min(there) if fn == MIN else max(there)
            out[fn].append(r)
    return out


def window(values_in_window_order, valid, part_start, part_end, fn, frm, to, sum_bits=128):
    """one function over every row's frame → [value or None]; SUM wraps to `sum_bits` (64 for int32 / int64 arguments, 128 for decimals)"""
    return window_all(values_in_window_order, valid, part_start, part_end, [fn], frm, to, sum_bits)[fn]


def sum_bits_of(arrow_type):
    return 128 if pa.types.is_decimal(arrow_type) else 64


def result_type(fn, arrow_type):
    """the result column type ldb_gpu_window states for `fn` over an argument of `arrow_type`"""
    if fn in (RANK, COUNT, COUNT_STAR):
        return pa.int64()
    if fn == SUM and pa.types.is_int32(arrow_type):
        return pa.int64()
    return arrow_type


# ------------------------------------------------------------------ inputs: helpers
def _i64(vals):
    return pa.array([int(v) for v in vals], pa.int64())


def _i32(vals):
    return pa.array([int(v) for v in vals], pa.int32())


def _date(vals):
    return _i32(vals).cast(pa.date32())


def _nullable(arr, valid):
    return with_validity(arr, np.asarray(valid, dtype=bool))


def _opt(make, vals, fill):
    """column from Python values with None for NULL; the slot under a NULL holds `fill`"""
    return _nullable(make([fill if v is None else v for v in vals]), [v is not None for v in vals])


def _draw(rng, pool, n):
    """n values from `pool`, every one at least once when n allows"""
    idx = np.concatenate([rng.permutation(len(pool))[:n], rng.integers(0, len(pool), max(n - len(pool), 0))])
    return [pool[int(i)] for i in rng.permutation(idx)]


def _sides_of(rng, pool, nl, nr):
    """two draws whose pools overlap but for two values at either end: some rows are on one side only"""
    return _draw(rng, pool[:-2], nl), _draw(rng, pool[2:], nr)


STR_POOL = [b"", b"a", b"a\0", b"ab", b"thirteen byte", PREFIX40 + b"thirteen more", PREFIX40 + b"x" * 260, PREFIX40 + b"x" * 259 + b"y", b"\x80", b"\xff\xfe", "é".encode(), b"b"]
assert [len(s) for s in STR_POOL[4:8]] == [13, 53, 300, 300]
DEC38_POOL = [1 * 2 ** 64 + 5, 2 * 2 ** 64 + 5, 3 * 2 ** 64 + 5, 7 * 2 ** 64 + 1, 7 * 2 ** 64 + 2, 7 * 2 ** 64 + 3, 2 ** 64, -(2 ** 64), 2 ** 64 + 1, -(2 ** 64 + 1), 2 ** 64 - 1, -(2 ** 64 - 1), 0, 5, -1,
              10 ** 38 - 1]
I32_POOL = [-(2 ** 31), 2 ** 31 - 1, -1, 0, 1, 7, 255, 256, -256, 65536, 2 ** 31 - 2, 12]
I64_POOL = [I64_MIN, I64_MAX, -1, 0, 1, 2 ** 32, -(2 ** 32), 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 31, 7, -7]
DATE_POOL = [-25567, -1, 0, 1, -365, 365, 19000, -719162, 2932896, 10957]
DEC12_POOL = [0, -1, 1, 10 ** 12 - 1, -(10 ** 12) + 1, 100, -100, 2 ** 32, -(2 ** 32), 12345]
# float64 keys: hashing is by bits while equality is by value, so +0.0 and -0.0 together would be one key with two hashes — deliberately out of scope
# (the frontend never produces both from one expression); only +0.0 appears, and no NaN
F64_POOL = [0.0, 1.5, -1.5, 5e-324, -5e-324, float("inf"), float("-inf"), 1e308, 0.1, 2.0 ** 53, 3.0, -3.0]

_SET, _SET_REFUSE, _WIN, _WIN_REFUSE = None, None, None, None


def _set_case(out, name, left, right, lcols=None, rcols=None, **kw):
    """left / right: a pyarrow table or a relation dict; lcols / rcols default to every column of a table, side 0"""
    left = table_rel(left) if isinstance(left, pa.Table) else left
    right = table_rel(right) if isinstance(right, pa.Table) else right
    lcols = lcols if lcols is not None else [(0, c) for c in range(left["table"].num_columns)]
    rcols = rcols if rcols is not None else [(0, c) for c in range(right["table"].num_columns)]
    case = {"name": name, "left": left, "right": right, "lcols": lcols, "rcols": rcols, "ops": ALL_OPS, "path": None, "spec": False, "dict": None, "narrow": False}
    assert not set(kw) - set(case), kw
    case.update(kw)
    out.append(case)


def _build_set_cases():
    rng = np.random.default_rng(20261022)
    out, refuse = [], []
    # ---- one column of every key type d_hash_part / d_key_part_equal distinguish
    for ty, pool, make in (("int32", I32_POOL, _i32), ("int64", I64_POOL, _i64), ("date32", DATE_POOL, _date), ("dec12_2", DEC12_POOL, lambda v: dec_array(v, 12, 2)),
                           ("dec38_0", DEC38_POOL, lambda v: dec_array(v, 38, 0)), ("utf8", STR_POOL, str_array), ("float64", F64_POOL, lambda v: pa.array(np.array(v, dtype=np.float64)))):
        l, r = _sides_of(rng, pool, 40, 33)
        _set_case(out, "type_" + ty, pa.table({"k": make(l)}), pa.table({"k": make(r)}))
        if ty == "dec12_2":  # both sides narrowed to 64 bits at registration: the concatenation keeps the source width
            _set_case(out, "type_dec12_2_narrow", pa.table({"k": make(l)}), pa.table({"k": make(r)}), narrow=True)
    # ---- three columns
    def three(n):
        return pa.table({"i": _i32(rng.integers(-1, 2, n)), "s": str_array([STR_POOL[int(i)] for i in rng.integers(0, 4, n)]), "d": dec_array([int(v) for v in rng.integers(-1, 2, n)], 12, 2)})

    _set_case(out, "three_columns", three(150), three(110))
    # ---- NULLs: which side carries a bitmap x where the right bitmap lands (bit offset na % 8 = 7, 0, 1)
    for na in (7, 8, 9):
        for which in ("left", "right", "both"):
            lv, rv = [int(v) for v in rng.integers(0, 4, na)], [int(v) for v in rng.integers(0, 4, 21)]
            lok, rok = rng.random(na) >= 0.4, rng.random(21) >= 0.4
            lok[0], rok[0], rok[20] = False, False, False  # a NULL at the seam and in the last bit
            left = pa.table({"k": _nullable(_i64(lv), lok) if which != "right" else _i64(lv)})
            right = pa.table({"k": _nullable(_i64(rv), rok) if which != "left" else _i64(rv)})
            _set_case(out, "null_%s_na%d" % (which, na), left, right)
    _set_case(out, "null_all_left", pa.table({"k": _nullable(_i64(range(13)), np.zeros(13, bool))}), pa.table({"k": _opt(_i64, [None, 1, 2, None, 12, 1], 3)}))
    _set_case(out, "null_all_right", pa.table({"k": _opt(_i64, [4, None, 4, 0], 0)}), pa.table({"k": _nullable(_i64(range(9)), np.zeros(9, bool))}))
    pair = lambda rows: pa.table({"a": _opt(_i32, [a for a, _ in rows], 1), "b": _opt(_i64, [b for _, b in rows], 1)})  # (the slot under a NULL holds 1 as well)
    _set_case(out, "null_pairs", pair([(1, None)] * 3 + [(None, 1)] * 2 + [(None, None)] * 4 + [(1, 1)]), pair([(1, 1)] * 3 + [(None, None)] * 2 + [(1, None)] + [(None, 1)] * 5))
    _set_case(out, "null_vs_empty", pa.table({"s": _opt(str_array, [None, b"", b"", None, b"a", None], b"")}), pa.table({"s": _opt(str_array, [b"", None, b"a", b"a"], b"")}))
    _set_case(out, "null_vs_zero", pa.table({"k": _opt(_i32, [None, 0, 0, None, 5, None], 0)}), pa.table({"k": _opt(_i32, [0, None, 5, 5], 0)}))
    # ---- sizes and group-by layouts (one int key unless noted)
    none = pa.table({"k": pa.array([], pa.int64())})
    some = pa.table({"k": _i64([3, 1, 3, 2, 3])})
    _set_case(out, "empty_both", none, none)
    _set_case(out, "empty_left", none, some)  # INTERSECT [ALL] and EXCEPT [ALL] are empty: nothing on the left
    _set_case(out, "empty_right", some, none)
    _set_case(out, "one_one_same", pa.table({"k": _i64([7])}), pa.table({"k": _i64([7])}))
    _set_case(out, "one_one_other", pa.table({"k": _i64([7])}), pa.table({"k": _i64([8])}))
    _set_case(out, "lds_1000", pa.table({"k": _i64(rng.integers(0, 300, 600))}), pa.table({"k": _i64(rng.integers(100, 400, 400))}), spec=True)
    _set_case(out, "lds_overflow_5000", pa.table({"k": _i64(rng.integers(0, 10000, 3000))}), pa.table({"k": _i64(rng.integers(0, 10000, 2000))}), spec=True)
    _set_case(out, "direct_12000", pa.table({"k": _i32(rng.integers(-3000, 3000, 7000))}), pa.table({"k": _i32(rng.integers(-3000, 3000, 5000))}), path="k_groupby_direct", spec=True)
    # dense sorted path: both sides ascending, the right side starts with the left side's largest value; runs begin and end on multiples of 64 rows
    runs_l = [64, 64, 128, 1, 63, 64, 5, 59, 192, 1, 1, 62]  # 704 rows = 11 chunks; boundaries at 64, 128, 256, 320, 384, 448, 640, 704
    for seam, tail in (("mid", 6390 - 704), ("chunk", 6400 - 704)):
        lens = runs_l + [int(v) for v in rng.integers(1, 9, 2000)]
        cut = np.searchsorted(np.cumsum(lens), 704 + tail - 30)
        lens = lens[:cut] + [704 + tail - int(np.sum(lens[:cut]))]  # the last run (>= 30 rows) ends the side exactly
        lk = np.repeat(np.arange(len(lens)) * 3 - 500, lens)
        rl = [40] + [int(v) for v in rng.integers(1, 9, 2000)]
        cut = np.searchsorted(np.cumsum(rl), 12000 - len(lk) - 70)
        rl = rl[:cut] + [12000 - len(lk) - int(np.sum(rl[:cut]))]
        rk = np.repeat(lk[-1] + np.arange(len(rl)) * 2, rl)
        assert len(lk) + len(rk) == 12000 and rk[0] == lk[-1]
        _set_case(out, "sorted_12000_seam_" + seam, pa.table({"k": _i64(lk)}), pa.table({"k": _i64(rk)}), path="k_gb_sorted_heads", spec=seam == "mid")
    lo = rng.integers(0, 50000, 7000)
    lo[3456] = 2 ** 31 - 5  # one far key: the ordered slots squeeze every other key into a few slots and give up
    _set_case(out, "outlier_12000", pa.table({"k": _i32(lo)}), pa.table({"k": _i32(rng.integers(0, 50000, 5000))}), spec=True)
    pool64 = rng.integers(I64_MIN, I64_MAX, 5000, endpoint=True)
    _set_case(out, "hashed_12000", pa.table({"k": _i64(pool64[rng.integers(0, 4000, 7000)])}), pa.table({"k": _i64(pool64[rng.integers(1000, 5000, 5000)])}), spec=True)
    pairs = lambda n: pa.table({"a": _i32(rng.integers(0, 90, n)), "b": _i64(rng.integers(0, 70, n) << 33)})
    _set_case(out, "pairs_12000", pairs(7000), pairs(5000), spec=True)
    # ---- multiplicities
    l = [11] * 3000 + [22] + [33] * 5 + [44] * 2
    r = [11] + [22] * 3000 + [33] * 5 + [55] * 3
    _set_case(out, "mult_3000_1", pa.table({"k": _i64(rng.permutation(l))}), pa.table({"k": _i64(rng.permutation(r))}))
    # EXCEPT ALL / INTERSECT ALL: 1000 keys of multiplicity 0 (on the right only) around three large groups, first, in the middle and last by key
    l = [0] * 3000 + [500] * 1500 + [1002] * 4000
    r = [0] * 500 + [500] * 1000 + [1002] * 1000 + [k for k in range(1, 1002) if k != 500]
    _set_case(out, "mult_zero_runs", pa.table({"k": _i32(rng.permutation(l))}), pa.table({"k": _i32(rng.permutation(r))}))
    # ---- relations
    base = pa.table({"id": _i32(range(900)), "v": _i64(rng.integers(-20, 20, 900)), "s": str_array([STR_POOL[int(i)] for i in rng.integers(0, 6, 900)])})
    other = pa.table({"v": _i64(rng.integers(-5, 30, 500)), "s": str_array([STR_POOL[int(i)] for i in rng.integers(2, 8, 500)])})
    _set_case(out, "rel_filter_left", filter_rel(base, 1, "GTE", 0), other, lcols=[(0, 1), (0, 2)])
    probe = pa.table({"k": _i32(rng.integers(0, 60, 700))})
    build = pa.table({"k": _i32(rng.integers(0, 40, 90)), "v": _opt(_i64, [None if i % 9 == 0 else int(v) for i, v in enumerate(rng.integers(0, 4, 90))], -1),
                      "s": str_array([STR_POOL[int(i)] for i in rng.integers(0, 3, 90)])})
    nulls = pa.table({"v": _opt(_i64, [None, 0, 1, None, 2, 3, 1, None], 0), "s": _opt(str_array, [None, b"", b"a", b"a", b"a\0", b"", b"a", None], b"zz")})
    _set_case(out, "rel_louter_right", nulls, louter_rel(probe, build, 0, 0), rcols=[(1, 1), (1, 2)])  # padding = (NULL, NULL) = the left side's (NULL, NULL)
    a = pa.table({"x": _i64(rng.integers(0, 5, 300)), "pad": _i32(range(300)), "y": _i32(rng.integers(0, 3, 300))})
    b = pa.table({"pad": str_array([b"p"] * 200), "y": _i32(rng.integers(0, 4, 200)), "x": _i64(rng.integers(1, 6, 200))})
    _set_case(out, "cols_other_positions", a, b, lcols=[(0, 0), (0, 2)], rcols=[(0, 2), (0, 1)])
    sq = pa.table({"p": _i32(rng.integers(0, 3, 200)), "q": _i32(rng.integers(0, 3, 200))})
    _set_case(out, "cols_reordered_pair", sq, sq, lcols=[(0, 0), (0, 1)], rcols=[(0, 1), (0, 0)])
    _set_case(out, "same_table", base, base, lcols=[(0, 1), (0, 2)], rcols=[(0, 1), (0, 2)])
    short = [v for v in STR_POOL if len(v) <= 256]  # (a dictionary is ordered by the string sort, whose keys hold at most 256 bytes)
    sl = pa.table({"s": str_array(_draw(rng, short[:-2], 300))})
    sr = pa.table({"s": str_array(_draw(rng, short[2:], 260))})
    _set_case(out, "dict_left", sl, sr, dict="left")
    _set_case(out, "dict_right", sl, sr, dict="right")

    def wide(n, extra):
        cols = {"a": _i32(rng.integers(0, 2, n)), "b": _i64(rng.integers(0, 2, n) << 40), "c": _date(rng.integers(-1, 1, n)), "d": dec_array([int(v) for v in rng.integers(-1, 1, n)], 12, 2),
                "e": str_array([[b"", b"a"][int(i)] for i in rng.integers(0, 2, n)]), "f": dec_array([int(v) * 2 ** 64 for v in rng.integers(0, 2, n)], 38, 0),
                "g": _opt(_i32, [None if v else 1 for v in rng.integers(0, 2, n)], 1), "h": pa.array(rng.integers(0, 2, n).astype(np.float64))}
        if extra:
            cols["i"] = _i32(rng.integers(0, 2, n))
        return pa.table(cols)

    _set_case(out, "eight_columns", wide(700, False), wide(500, False))
    # ---- refusals: (name, left table, left columns, right table, right columns, op, status name)
    nine = wide(50, True)
    refuse.append(("nine_columns", nine, list(range(9)), nine, list(range(9)), UNION, "LDB_ERR_INVALID"))
    refuse.append(("int32_against_int64", pa.table({"k": _i32([1, 2])}), [0], pa.table({"k": _i64([1, 2])}), [0], INTERSECT, "LDB_ERR_INVALID"))
    refuse.append(("dec12_2_against_dec12_3", pa.table({"k": dec_array([1, 2], 12, 2)}), [0], pa.table({"k": dec_array([1, 2], 12, 3)}), [0], UNION_ALL, "LDB_ERR_INVALID"))
    refuse.append(("operation_6", some, [0], some, [0], 6, "LDB_ERR_INVALID"))
    return out, refuse


def set_cases():
    """yields dicts: name, left / right (relation dicts), lcols / rcols ([(side, column)]), ops, path (a profiler name that must have run, or None),
    spec (also run with specialised kernels), dict ('left' / 'right': that side's strings dictionary-encoded), narrow.  Tables are shared and must
    not be changed."""
    global _SET, _SET_REFUSE
    if _SET is None:
        _SET, _SET_REFUSE = _build_set_cases()
    return iter(_SET)


def set_refusals():
    set_cases()
    return iter(_SET_REFUSE)


FNS6 = (SUM, MIN, MAX, COUNT, RANK, COUNT_STAR)
SINGLE_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4096, 4097, 8193)
PART_SIZES = (256, 255, 1, 63, 1, 64, 65, 2, 700, 1, 257, 1, 1)  # in key order: boundaries at 256, 512 (multiples of 256), 576, 640, 1408 (of 64)


def single_frames(n):
    return [(P, 0), (P, F), (0, F), (0, 0), (-1, 1), (-3, -1), (1, 3), (-n, n), (-(2 ** 40), 2 ** 40), (5, F), (P, -5)]


def _win_case(out, name, rel, part, order, fns, frames, **kw):
    """part = [(side, col)], order = [(side, col, descending, nulls)], fns = [(fn, (side, col) or None)]"""
    rel = table_rel(rel) if isinstance(rel, pa.Table) else rel
    case = {"name": name, "rel": rel, "part": part, "order": order, "fns": fns, "frames": frames, "spec": False, "narrow": False}
    assert not set(kw) - set(case), kw
    case.update(kw)
    assert 1 <= len(fns) <= 8
    out.append(case)


def _six(col):
    return [(fn, None if fn in (RANK, COUNT_STAR) else col) for fn in FNS6]


def _build_window_cases():
    rng = np.random.default_rng(20261023)
    out, refuse = [], []
    N1 = NULLS_LARGEST
    # ---- one partition at the sizes where the tree's shape and the sort change; int64 argument, one NULL in six
    for n in SINGLE_SIZES:
        t = pa.table({"o": _i32(rng.permutation(n)), "v": _nullable(_i64(rng.integers(-(10 ** 6), 10 ** 6, n)), np.arange(n) % 6 != 1)})
        _win_case(out, "single_%d" % n, t, [], [(0, 0, False, 0)], _six((0, 1)), single_frames(n))
    # ---- partitions
    some_frames = [(P, 0), (P, F), (-2, 1), (0, 3), (-5, -1), (-1, 1)]
    n = sum(PART_SIZES)
    p = np.concatenate([np.full(s, 10 * k - 30) for k, s in enumerate(PART_SIZES)])
    o = np.concatenate([rng.permutation(s) for s in PART_SIZES])
    sh = rng.permutation(n)
    t = pa.table({"p": _i32(p[sh]), "o": _i32(o[sh]), "v": _nullable(_i64(rng.integers(-1000, 1000, n)), rng.integers(0, 6, n) > 0)})
    _win_case(out, "part_sizes", t, [(0, 0)], [(0, 1, True, 0)], _six((0, 2)), some_frames)
    t = pa.table({"p": _i32(rng.permutation(5000) - 2500), "v": _nullable(_i64(rng.integers(-9, 9, 5000)), rng.integers(0, 4, 5000) > 0)})
    _win_case(out, "part_5000_of_one_row", t, [(0, 0)], [], _six((0, 1)), [(P, 0), (-1, 1), (P, F), (1, 3)])
    n = 600
    keys = {"i32_utf8": None, "utf8": str_array, "dec38_0": lambda v: dec_array(v, 38, 0), "date32": _date}
    pools = {"utf8": [s for s in STR_POOL if len(s) <= 256] + [b"Z" * 256], "dec38_0": DEC38_POOL, "date32": DATE_POOL}  # (a string sort key holds at most 256 bytes)
    for name, make in keys.items():
        o = _i32(rng.permutation(n))
        v = _nullable(_i64(rng.integers(-1000, 1000, n)), rng.integers(0, 5, n) > 0)
        if make is None:  # (int32, utf8), a NULL in either
            a = _opt(_i32, [None if x == 3 else int(x) for x in rng.integers(0, 4, n)], 0)
            b = _opt(str_array, [None if x == 3 else [b"", b"a", b"a\0"][int(x)] for x in rng.integers(0, 4, n)], b"")
            _win_case(out, "part_key_" + name, pa.table({"a": a, "b": b, "o": o, "v": v}), [(0, 0), (0, 1)], [(0, 2, False, 0)], _six((0, 3)), some_frames[:3])
        else:
            pool = pools[name]
            k = _opt(make, [None if x == len(pool) else pool[int(x)] for x in rng.integers(0, len(pool) + 1, n)], pool[0])
            _win_case(out, "part_key_" + name, pa.table({"k": k, "o": o, "v": v}), [(0, 0)], [(0, 1, False, 0)], _six((0, 2)), some_frames[:3])
    # ---- argument types: two partitions (200 and 100 rows), unique order key
    n = 300
    p, o = _i32([0] * 200 + [1] * 100), _i32(rng.permutation(n))
    arg_frames = [(P, 0), (P, F), (-3, 3), (0, 0)]

    def arg_case(name, col, fns=None, **kw):
        _win_case(out, "arg_" + name, pa.table({"p": p, "o": o, "v": col}), [(0, 0)], [(0, 1, False, 0)], fns or _six((0, 2)), arg_frames, **kw)

    near = [2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 2, -(2 ** 31) + 1]
    arg_case("int32_extremes", _nullable(_i32(_draw(rng, near, n)), rng.integers(0, 7, n) > 0))  # SUM leaves 32 bits after two rows and must not wrap there
    arg_case("int64_wraps", _nullable(_i64(_draw(rng, [2 ** 62, 2 ** 62 + 1, -(2 ** 62), 2 ** 62 - 1, I64_MAX], n)), rng.integers(0, 7, n) > 0))  # SUM wraps at 64 bits
    arg_case("date32", _nullable(_date(_draw(rng, DATE_POOL, n)), rng.integers(0, 5, n) > 0), [(MIN, (0, 2)), (MAX, (0, 2)), (COUNT, (0, 2)), (RANK, None), (COUNT_STAR, None)])
    dec12 = _nullable(dec_array(_draw(rng, DEC12_POOL, n), 12, 2), rng.integers(0, 5, n) > 0)
    arg_case("dec12_2", dec12)
    arg_case("dec12_2_narrow", dec12, narrow=True)
    cross = [2 ** 63, 2 ** 63, -(2 ** 64), 2 ** 64 - 1, 1, -(2 ** 63) - 1, 5 * 2 ** 64 + 9, 6 * 2 ** 64 + 9, 5 * 2 ** 64 + 8, -(5 * 2 ** 64) - 9, -(6 * 2 ** 64) - 9, -(2 ** 63)]  # partial sums cross ±2^64; values that tie in one word
    arg_case("dec38_0", _nullable(dec_array(_draw(rng, cross, n), 38, 0), rng.integers(0, 6, n) > 0))
    arg_case("all_null", _nullable(_i64(rng.integers(-9, 9, n)), np.zeros(n, bool)))
    arg_case("null_partition", _nullable(_i64(rng.integers(-9, 9, n)), np.arange(n) < 200))  # partition 1 is NULL throughout, partition 0 has no NULL
    arg_case("no_nulls", _i64(rng.integers(-(10 ** 9), 10 ** 9, n)))
    # ---- order
    t = pa.table({"o": _i32(rng.integers(0, 5, 500)), "v": _nullable(_i64(rng.integers(-50, 50, 500)), rng.integers(0, 5, 500) > 0)})
    _win_case(out, "order_ties", t, [], [(0, 0, False, 0)], _six((0, 1)), arg_frames)  # ties keep the input order
    t = pa.table({"a": _i32(rng.integers(0, 7, 500)), "b": _i64(rng.integers(0, 9, 500)), "v": _i64(rng.integers(-50, 50, 500))})
    _win_case(out, "order_two_keys_second_desc", t, [], [(0, 0, False, 0), (0, 1, True, 0)], _six((0, 2)), arg_frames)
    t = pa.table({"p": _i32(rng.integers(0, 3, 500)), "o": _opt(_i64, [None if x == 9 else int(x) for x in rng.integers(0, 10, 500)], 4), "v": _i64(rng.integers(-50, 50, 500))})
    _win_case(out, "order_nullable_asc", t, [(0, 0)], [(0, 1, False, N1)], _six((0, 2)), arg_frames)
    _win_case(out, "order_nullable_desc", t, [(0, 0)], [(0, 1, True, N1)], _six((0, 2)), arg_frames)
    refuse.append(("order_nulls_refused", t, [(0, 0)], [(0, 1, False, NULLS_REFUSE)], [(RANK, None)], "LDB_ERR_UNSUPPORTED"))
    # ---- relations
    n = 7000
    base = pa.table({"p": _i32(rng.integers(0, 4, n)), "o": _i32(rng.permutation(n)), "v": _nullable(_i64(rng.integers(-100, 100, n)), rng.integers(0, 6, n) > 0), "w": _i32(rng.integers(0, 10, n))})
    _win_case(out, "rel_filter", filter_rel(base, 3, "LT", 7), [(0, 0)], [(0, 1, False, 0)], _six((0, 2)), some_frames[:4], spec=True)  # about 4900 rows: the radix sort over row ids
    _win_case(out, "rel_filter_small", filter_rel(base, 3, "EQ", 2), [(0, 0)], [(0, 1, True, 0)], _six((0, 2)), some_frames[:4], spec=True)  # about 700 rows
    probe = pa.table({"k": _i32(rng.integers(0, 60, 800)), "id": _i32(rng.permutation(800))})
    build = pa.table({"k": _i32(rng.integers(0, 40, 90)), "g": _i32(rng.integers(0, 3, 90)), "v": _opt(_i64, [None if i % 9 == 0 else int(v) for i, v in enumerate(rng.integers(-40, 40, 90))], 7),
                      "id": _i32(rng.permutation(90))})
    j = louter_rel(probe, build, 0, 0)
    jorder = [(0, 1, False, 0), (1, 3, False, N1)]  # (probe id, build id): a total order of the pairs, whatever order the join wrote them in
    _win_case(out, "rel_louter_arg", j, [(0, 0)], jorder, _six((1, 2)), some_frames[:3])
    _win_case(out, "rel_louter_part_key", j, [(1, 1)], jorder, _six((1, 2)), some_frames[:3])
    # ---- limits
    t = pa.table({"p": _i32(rng.integers(0, 3, 400)), "o": _i32(rng.permutation(400)), "v": _nullable(_i64(rng.integers(-50, 50, 400)), rng.integers(0, 5, 400) > 0), "w": _i32(rng.integers(-5, 5, 400))})
    eight = [(SUM, (0, 2)), (MIN, (0, 2)), (MAX, (0, 2)), (COUNT, (0, 2)), (SUM, (0, 3)), (MAX, (0, 3)), (RANK, None), (COUNT_STAR, None)]
    _win_case(out, "eight_functions", t, [(0, 0)], [(0, 1, False, 0)], eight, arg_frames)
    # ---- inverted frames (from > to): the empty state, where the reference throws
    _win_case(out, "inverted_frames", t, [(0, 0)], [(0, 1, False, 0)], _six((0, 2)), [(3, 1), (2, -2), (1, 0), (0, -1), (2 ** 40, -(2 ** 40))])
    # ---- refusals: (name, table, part, order, fns, status name)
    d = pa.table({"p": _i32([0, 0, 1]), "dt": _date([1, -2, 3]), "f": pa.array([1.0, 2.0, 3.0]), "v": _i64([1, 2, 3])})
    refuse.append(("nine_functions", d, [(0, 0)], [], [(SUM, (0, 3))] * 9, "LDB_ERR_INVALID"))
    refuse.append(("sum_over_date32", d, [(0, 0)], [], [(SUM, (0, 1))], "LDB_ERR_INVALID"))
    refuse.append(("float64_argument", d, [(0, 0)], [], [(SUM, (0, 2))], "LDB_ERR_UNSUPPORTED"))
    refuse.append(("function_6", d, [(0, 0)], [], [(6, (0, 3))], "LDB_ERR_INVALID"))
    refuse.append(("nine_partition_keys", d, [(0, 0)] * 9, [], [(RANK, None)], "LDB_ERR_INVALID"))
    return out, refuse


def window_cases():
    """yields dicts: name, rel (a relation dict), part, order, fns, frames, spec (also run with specialised kernels and a pending lazy filter), narrow"""
    global _WIN, _WIN_REFUSE
    if _WIN is None:
        _WIN, _WIN_REFUSE = _build_window_cases()
    return iter(_WIN)


def window_refusals():
    window_cases()
    return iter(_WIN_REFUSE)


def arg_type(case, ref):
    return rel_tables(case["rel"])[ref[0]].schema.field(ref[1]).type


_EXPECT = {}


def window_layout(case, sides=None, n=None):
    """(order, part_start, part_end, {argument column: values in window order}) of a window case; computed once per case when the relation's
    row ids are the file's own (`sides` None), afresh when the caller read them from a device"""
    if sides is None and case["name"] in _EXPECT:
        return _EXPECT[case["name"]]
    own = sides is None
    if own:
        sides, n = rel_sides(case["rel"])
    part_vals = [rel_column(sides, c) for c in case["part"]]
    order = window_order_values(part_vals, [(rel_column(sides, (s, c)), d, nl) for s, c, d, nl in case["order"]], n)
    start, end = partitions(part_vals, order, n)
    args = {}
    for fn, col in case["fns"]:
        if col is not None and col not in args:
            vals = rel_column(sides, col)
            args[col] = [vals[int(r)] for r in order]
    res = (order, start, end, args)
    if own:
        _EXPECT[case["name"]] = res
    return res
