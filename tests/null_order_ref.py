"""Plain-Python statement of ORDER BY over NULLABLE keys — TEST INFRASTRUCTURE, order_ref.sort plus the reference's three NULL rules.

The reference rewrites the comparison of nullable operands before it lowers db.sort_compare (SimplifySortComparePattern,
src/compiler/Dialect/DB/Transforms/PrepareLowering.cpp:106-132):
  * left NULL, right not: +1        * right NULL, left not: -1        * both NULL: 0        * otherwise: db.sort_compare on the values
and a DESC key swaps the operands (createSortedView, RelAlgToSubOp.cpp:1646-1653), i.e. negates the result, the NULL rules included.
So NULL is the largest value of every type: last ascending, first descending; NULLs tie, the next key and then the input position decide.
oracle/ldb_oracle.c's sort ignores validity, so for nullable inputs this file is the expected order.

Values are Python objects as in order_ref (ints, floats, bytes) and None stands for NULL; whatever an Arrow array stores under a NULL
slot is never looked at.  A relation is a list of sides (pyarrow table, row-id vector or None); a row id of 0xFFFFFFFF is outer-join
padding: every column of that side is NULL in that row.  `cases()` owns the seeded inputs of tests/test_null_order.py (no device) and
tests/test_gpu_null_order.py (device): both see the same tables.  Nothing here reads a clock or the environment."""
import functools

import numpy as np
import pyarrow as pa

import order_ref

NULL_ROW = 0xFFFFFFFF
ROWS = (3000, 4097, 8193)  # the one-workgroup sort, the first radix size, just above a radix block boundary
N_MAX = max(ROWS)
I64_MIN, I64_MAX = order_ref.I64_MIN, order_ref.I64_MAX


# ------------------------------------------------------------------ arrow → Python values, None for NULL
def with_validity(arr, valid):
    """`arr` (no NULLs, offset 0) with the validity bitmap `valid` (bools) laid over it: the value buffers stay as they are, so a NULL slot
    keeps whatever raw value `arr` held there"""
    assert arr.null_count == 0 and arr.offset == 0 and len(valid) == len(arr)
    bitmap = np.packbits(np.asarray(valid, dtype=bool), bitorder="little").tobytes()
    return pa.Array.from_buffers(arr.type, len(arr), [pa.py_buffer(bitmap)] + arr.buffers()[1:], null_count=int(len(arr) - np.count_nonzero(valid)))


def column_values(col):
    """one column as Python values; None where the validity bitmap says NULL"""
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if isinstance(arr, pa.ChunkedArray):
        arr = pa.concat_arrays(arr.chunks)
    valid = arr.is_valid().to_pylist()
    bufs = arr.buffers()
    raw = pa.Array.from_buffers(arr.type, len(arr), [None] + bufs[1:], null_count=0, offset=arr.offset)  # the same slots, all readable
    vals = order_ref.column_values(raw) if not pa.types.is_floating(arr.type) else [float(v) for v in raw.to_numpy(zero_copy_only=False)]
    out = [v if ok else None for v, ok in zip(vals, valid)]
    assert all(v == v for v in out if isinstance(v, float)), "NaN among the valid values: the comparator is not an order"
    return out


def side_values(table, col, rowids):
    vals = column_values(table.column(col))
    if rowids is None:
        return vals
    return [None if int(r) == NULL_ROW else vals[int(r)] for r in rowids]


def compare(x, y):
    """the reference's comparator on two values of one key, ascending: -1, 0, +1"""
    if x is None or y is None:
        if x is None and y is None:
            return 0
        return 1 if x is None else -1
    if x < y:
        return -1
    if y < x:
        return 1
    return 0


def sort_values(keys, n):
    """positions 0..n-1 in ORDER BY order; keys = [(values, descending)]"""
    keys = [(vals, -1 if desc else 1) for vals, desc in keys]

    def cmp(a, b):
        for vals, sign in keys:
            c = compare(vals[a], vals[b])
            if c:
                return sign * c
        return a - b  # input position

    return np.array(sorted(range(n), key=functools.cmp_to_key(cmp)), dtype=np.uint32)


def sort_rel(sides, n, specs):
    """positions of the relation's rows in ORDER BY order; sides = [(table, rowids or None)], specs = [(side, column, descending)]"""
    return sort_values([(side_values(sides[s][0], c, sides[s][1]), desc) for s, c, desc in specs], n)


def sort(table, specs):
    """row numbers of `table` in ORDER BY specs = [(column index, descending)] order, as uint32 (the signature of order_ref.sort)"""
    return sort_rel([(table, None)], table.num_rows, [(0, c, desc) for c, desc in specs])


def topk(table, specs, k):
    return sort(table, specs)[: max(k, 0)]


def sort_specs(specs, nulls=1, side=0):
    from lingodb_amd import api

    return [api.sort_spec((side, c), bool(desc), nulls) for c, desc in specs]


# ------------------------------------------------------------------ inputs
TYPE_NAMES = ("int32", "int64", "date32", "dec12_2", "dec38_0", "float64", "char1", "utf8")
PATTERNS = ("one", "third", "all", "allset")  # one NULL, about a third NULL, all NULL, a validity bitmap with every bit set
_CASES = None
_EXTRA = {}  # case name → the k values of its top-k checks


def _pattern(rng, name, n):
    if name == "one":
        v = np.ones(n, dtype=bool)
        v[1234] = False
        return v
    if name == "third":
        return rng.random(n) >= 1 / 3
    return np.zeros(n, dtype=bool) if name == "all" else np.ones(n, dtype=bool)


def _under_null_tables():
    """NULL slots that hold extreme and mutually different raw values; a valid INT64_MAX / b"\\xff\\xff" / +inf must sort before every NULL,
    the NULLs must tie (the `tie` column, then the position, orders them), and NULL, b"" and b"\\0" are three distinct string keys.
    The 41 hand rows are repeated to 4100 rows (the radix path); the first 41 are the one-workgroup case."""
    reps = 100
    ints = [(I64_MAX, 1), (I64_MAX, 0), (I64_MIN, 0), (I64_MIN, 1), (0, 1), (0, 0), (-1, 1), (1, 0), (I64_MAX - 1, 1), (I64_MAX, 0), (-1, 0)]
    strs = [(b"\xff\xff", 1), (b"\xff" * 256, 0), (b"\xff\xff\xff", 0), (b"", 1), (b"", 0), (b"\0", 1), (b"\0", 0), (b"\xff", 1), (b"a", 0), (b"\xff\xff", 0), (b"\0\0", 1), (b"Z" * 256, 1)]
    flts = [(float("inf"), 1), (float("inf"), 0), (float("-inf"), 0), (float("nan"), 0), (0.0, 1), (-0.0, 1), (0.0, 0), (1.5, 1), (float("-inf"), 1), (1.5, 0), (5e-324, 0)]
    out = {}
    for name, rows, make in (("int64", ints, lambda v: pa.array(v, pa.int64())), ("utf8", strs, order_ref.str_array), ("float64", flts, lambda v: pa.array(np.array(v, dtype=np.float64)))):
        rows = (rows * 4)[:41] * reps
        n = len(rows)
        tie = pa.array(((np.arange(n) * 7) % 3).astype(np.int32))
        out[name] = pa.table({"k": with_validity(make([v for v, _ in rows]), [bool(ok) for _, ok in rows]), "tie": tie})
    return out


def _build_cases():
    rng = np.random.default_rng(20261021)
    out = []
    cols = order_ref._type_columns(rng)
    tie = pa.array(rng.integers(-2, 3, N_MAX), pa.int32())
    # ---- one nullable key of every type + an int32 tie key, every NULL pattern, every row count, both directions.  The raw values under the
    # NULLs are the pool's (extremes of the type among them).  Tables of fewer rows are prefixes of the 8193-row one.
    for ty in TYPE_NAMES:
        for pat in PATTERNS:
            full = pa.table({"k": with_validity(cols[ty].slice(0, N_MAX), _pattern(rng, pat, N_MAX)), "tie": tie})
            for n in ROWS:
                t = full.slice(0, n)
                for way, specs in (("asc", [(0, False), (1, False)]), ("desc", [(0, True), (1, True)])):
                    out.append(("%s_%s_%d_%s" % (ty, pat, n, way), t, specs))
    # ---- bytes under a NULL
    for ty, t in _under_null_tables().items():
        for n in (41, t.num_rows):
            out.append(("under_null_%s_%d_asc" % (ty, n), t.slice(0, n), [(0, False), (1, False)]))
            out.append(("under_null_%s_%d_desc" % (ty, n), t.slice(0, n), [(0, True), (1, False)]))
    # ---- two nullable keys, the first ties on NULL for two rows in five
    n = 4097
    two = pa.table({"a": with_validity(pa.array(rng.integers(-3, 4, n), pa.int64()), rng.random(n) >= 0.4), "b": with_validity(pa.array(rng.integers(-50, 50, n), pa.int32()), rng.random(n) >= 0.2)})
    out.append(("two_keys_4097", two, [(0, False), (1, True)]))
    out.append(("two_keys_3000", two.slice(0, 3000), [(0, True), (1, False)]))
    # ---- eight nullable keys (the limit), directions mixed, every key of a handful of values and one NULL in four
    def nul(arr):
        return with_validity(arr, rng.random(len(arr)) >= 0.25)

    eight = pa.table({
        "a": nul(pa.array(rng.integers(-1, 2, n), pa.int8())),
        "b": nul(pa.array([bytes([c, 0, 0, 0]) for c in rng.choice(list(b"NR"), n)], pa.binary(4))),
        "c": nul(pa.array(rng.integers(-1, 1, n), pa.int32()).cast(pa.date32())),
        "d": nul(order_ref.dec_array([int(v) for v in rng.integers(-1, 2, n)], 12, 2)),
        "e": nul(pa.array(rng.choice([0.0, -0.0, -1.5], n))),
        "f": nul(order_ref.str_array([[b"", b"a", b"a\0"][i] for i in rng.integers(0, 3, n)])),
        "g": nul(order_ref.dec_array([int(v) * 2 ** 64 for v in rng.integers(-1, 2, n)], 38, 0)),
        "h": nul(pa.array(rng.integers(0, 2, n), pa.int64())),
    })
    out.append(("eight_keys_4097", eight, [(0, False), (1, True), (2, False), (3, True), (4, False), (5, True), (6, False), (7, True)]))
    # ---- top-k above 4096 rows (the radix select runs): 2000 of 6000 rows NULL in the leading key, all eight of its value bytes vary
    n = 6000
    lead = rng.integers(I64_MIN, I64_MAX, n, endpoint=True)
    valid = np.ones(n, dtype=bool)
    valid[rng.permutation(n)[:2000]] = False
    second = pa.array(rng.integers(-(2 ** 31), 2 ** 31, n), pa.int32())
    t = pa.table({"k": with_validity(pa.array(lead), valid), "v": second})
    out.append(("topk_third_null_asc", t, [(0, False), (1, False)]))
    _EXTRA["topk_third_null_asc"] = (3999, 4000, 4001, 5000)  # non-NULL count - 1, that count, + 1, + 1000
    out.append(("topk_third_null_desc", t, [(0, True), (1, False)]))
    _EXTRA["topk_third_null_desc"] = (1, 1999, 2000, 2001)
    # 5000 of 6000 NULL, descending: the NULLs come first and the second key decides among more than 4096 candidates
    valid = np.ones(n, dtype=bool)
    valid[rng.permutation(n)[:5000]] = False
    out.append(("topk_most_null_desc", pa.table({"k": with_validity(pa.array(lead), valid), "v": second}), [(0, True), (1, False)]))
    _EXTRA["topk_most_null_desc"] = (10,)
    return out


def cases():
    """yields (name, pyarrow table, specs = [(column index, descending)]); tables are shared between cases and must not be changed"""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return iter(_CASES)


def topk_ks(name):
    cases()
    return _EXTRA.get(name, (7,))


_ORDERS = {}


def expected(name):
    """the expected row order of a case, computed once and shared"""
    if name not in _ORDERS:
        _, table, specs = {c[0]: c for c in cases()}[name]
        _ORDERS[name] = sort(table, specs)
    return _ORDERS[name]
