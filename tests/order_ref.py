"""Plain-Python statement of the library's ORDER BY — TEST INFRASTRUCTURE, a second opinion beside oracle/ldb_oracle.c.

The comparator of db.sort_compare, written over Python values with nothing clever in it:
  * ints, dates (days) and decimals (unscaled) are Python ints, floats are Python floats (so -0.0 == +0.0 and no NaN is allowed),
  * strings and char(n) values are bytes: unsigned byte order, a proper prefix first (= bytes.__lt__),
  * a DESC key negates its comparison, the first key that differs decides, rows equal on every key keep their input order.
`cases()` is the one source of inputs for tests/test_order_edges.py (oracle against this file, no device) and tests/test_gpu_order_edges.py
(device against oracle): both see the same tables.  Seeds are fixed; nothing here reads a clock or the environment."""
import decimal
import functools

import numpy as np
import pyarrow as pa

ROWS = (3000, 4096, 4097, 8193, 20000)  # padded one-workgroup sort, its last size, the first radix size, just above a radix block boundary, many blocks
N_MAX = max(ROWS)
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
PREFIX40 = b"forty bytes that every value starts with"
assert len(PREFIX40) == 40


# ------------------------------------------------------------------ arrow → Python values
def str_array(vals):
    """utf8 column from bytes objects without validation (bytes >= 0x80 that are no UTF-8 stay as they are)"""
    return pa.array(vals, pa.binary()).view(pa.string())


def dec_array(unscaled, precision, scale):
    """decimal128 column from unscaled ints, exact at any precision (no decimal context is involved)"""
    vals = [decimal.Decimal((1 if v < 0 else 0, tuple(int(ch) for ch in str(abs(v))), -scale)) for v in unscaled]
    return pa.array(vals, pa.decimal128(precision, scale))


def column_values(col):
    """one column as the Python values the comparator works on"""
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if isinstance(arr, pa.ChunkedArray):
        arr = pa.concat_arrays(arr.chunks)
    t = arr.type
    assert arr.null_count == 0, "the comparator is defined for non-NULL keys only"
    if pa.types.is_decimal(t):
        raw = arr.buffers()[1].to_pybytes()[arr.offset * 16 : (arr.offset + len(arr)) * 16]
        return [int.from_bytes(raw[16 * i : 16 * i + 16], "little", signed=True) for i in range(len(arr))]
    if pa.types.is_date32(t):
        return arr.cast(pa.int32()).to_pylist()
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        return arr.view(pa.binary() if pa.types.is_string(t) else pa.large_binary()).to_pylist()
    if pa.types.is_floating(t):
        vals = [float(v) for v in arr.to_numpy(zero_copy_only=False)]
        assert all(v == v for v in vals), "NaN: the comparator is not an order"
        return vals
    return arr.to_pylist()  # ints → int, fixed_size_binary → bytes


def sort(table, specs):
    """row numbers of `table` in ORDER BY specs = [(column index, descending)] order, as uint32"""
    cols = [(column_values(table.column(c)), -1 if desc else 1) for c, desc in specs]

    def cmp(a, b):
        for vals, sign in cols:
            x, y = vals[a], vals[b]
            if x < y:
                return -sign
            if y < x:
                return sign
        return a - b  # input position

    return np.array(sorted(range(table.num_rows), key=functools.cmp_to_key(cmp)), dtype=np.uint32)


def topk(table, specs, k):
    return sort(table, specs)[: max(k, 0)]


def partition_ids(oracle, rel, keys, nparts):
    """destination of every row of a host relation: the oracle's db.hash of the keys (tested elsewhere), bits 16.. modulo nparts"""
    return oracle.partition_ids(rel, keys, nparts)


def sort_specs(specs):
    from lingodb_amd import api

    return [api.sort_spec((0, c), bool(desc)) for c, desc in specs]


# ------------------------------------------------------------------ inputs
def _draw(rng, pool, n):
    """n values drawn from `pool`, every pool value at least once among the first len(pool) rows (so every row-count prefix holds all of them)"""
    assert len(pool) <= min(ROWS)
    idx = np.concatenate([rng.permutation(len(pool)), rng.integers(0, len(pool), n - len(pool))])
    return [pool[i] for i in idx]


def _int_pool(rng, bits):
    lo, hi = -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
    edge = [lo, lo + 1, hi, hi - 1, -1, 0, 1, -2, 2]
    if bits > 8:
        edge += [-256, 255, 256, -257]  # sign and carry across a key byte
    if bits > 32:
        edge += [-(2 ** 32), 2 ** 32, 2 ** 32 - 1, -(2 ** 32) - 1, -(2 ** 31), 2 ** 31]
    return edge + [int(v) for v in rng.integers(lo, hi, 200, endpoint=True)]


def _float_pool(rng, dtype):
    f = np.dtype(dtype).type
    tiny = float(np.nextafter(f(0), f(1)))  # the smallest subnormal: 5e-324 / 1.4e-45
    one_ulp = float(np.nextafter(f(1.5), f(2)))
    edge = [0.0, -0.0] * 8 + [tiny, -tiny, float("inf"), float("-inf"), 1.5, one_ulp, -1.5, -one_ulp, -0.5, -0.25, -0.75, 0.5, float(np.finfo(dtype).max), float(np.finfo(dtype).min),
                              float(np.finfo(dtype).tiny), -float(np.finfo(dtype).tiny)]
    rand = [float(f(v)) for v in rng.normal(0, 100, 150)] + [float(f(v)) for v in -rng.random(50)]
    return edge + rand


UTF8_POOL = [b"", b"a", b"ab", b"ab\0", b"a\0", b"a\0\0", b"b", b"\x7f", b"\x80", b"\xff", b"\x7f\xff", b"\xff\x00", b"\xff\xff", "é".encode(), "e".encode(), "日本語".encode(),
             "日本".encode(), "ß".encode(), "z".encode(), "𝄞".encode(), b"Z" * 256, b"Z" * 255, b"Z" * 255 + b"Y", b"Z" * 254 + b"\xff", b"abc", b"abd", b"ab ", b" ", b"A", b"aB"]
assert len(set(UTF8_POOL)) == len(UTF8_POOL) and max(len(v) for v in UTF8_POOL) == 256
PREFIX_POOL = [PREFIX40 + s for s in UTF8_POOL if len(s) < 200] + [PREFIX40[:39], PREFIX40[:39] + b"\xff", PREFIX40]


def _type_columns(rng):
    """{type name: one key column of N_MAX rows}: few distinct values per column, so ties on the first key are the rule"""
    n = N_MAX
    big38 = [10 ** 38 - 1, -(10 ** 38 - 1), 2 ** 63, -(2 ** 63), 2 ** 64, -(2 ** 64), 2 ** 64 + 1, -(2 ** 64 + 1), 2 ** 64 - 1, -(2 ** 64 - 1), -1, 0, 1, 2 ** 63 - 1, -(2 ** 63) - 1,
             2 ** 126, -(2 ** 126), 10 ** 37, -(10 ** 37)]
    big38 += [int(a) * 2 ** 64 + int(b) for a, b in zip(rng.integers(-(2 ** 60), 2 ** 60, 100), rng.integers(0, 2 ** 63, 100))]
    dec33 = [int(a) * 10 ** 15 + int(b) for a, b in zip(rng.integers(-(10 ** 17), 10 ** 17, 300), rng.integers(0, 10 ** 15, 300))] + [0, -1, 1, 2 ** 64, -(2 ** 64)]
    dec12 = [int(v) for v in rng.integers(-(10 ** 12) + 1, 10 ** 12, 200)] + [0, -1, 1, 10 ** 12 - 1, -(10 ** 12) + 1, -100, 100, 2 ** 32, -(2 ** 32)]
    dates = [-25567, -1, 0, 1, -365, 365, 10957, 19000, -719162, 2932896] + [int(v) for v in rng.integers(-40000, 40000, 100)]  # days before 1970 are negative
    chars = [bytes([c, 0, 0, 0]) for c in b"AFNORZaz09 ~!"]
    return {
        "int8": pa.array(_draw(rng, sorted(set(_int_pool(rng, 8))), n), pa.int8()),
        "int16": pa.array(_draw(rng, _int_pool(rng, 16), n), pa.int16()),
        "int32": pa.array(_draw(rng, _int_pool(rng, 32), n), pa.int32()),
        "int64": pa.array(_draw(rng, _int_pool(rng, 64), n), pa.int64()),
        "date32": pa.array(_draw(rng, dates, n), pa.int32()).cast(pa.date32()),
        "dec12_2": dec_array(_draw(rng, dec12, n), 12, 2),
        "dec38_0": dec_array(_draw(rng, big38, n), 38, 0),
        "dec33_4": dec_array(_draw(rng, dec33, n), 33, 4),
        "float64": pa.array(np.array(_draw(rng, _float_pool(rng, np.float64), n), dtype=np.float64)),
        "float32": pa.array(np.array(_draw(rng, _float_pool(rng, np.float32), n), dtype=np.float32)),
        "char1": pa.array(_draw(rng, chars, n), pa.binary(4)),
        "utf8": str_array(_draw(rng, UTF8_POOL, n)),
        "utf8_prefix40": str_array(_draw(rng, PREFIX_POOL, n)),
    }


TYPE_NAMES = ("int8", "int16", "int32", "int64", "date32", "dec12_2", "dec38_0", "dec33_4", "float64", "float32", "char1", "utf8", "utf8_prefix40")
TOPK_KS = {}  # case name → the k values of its top-k checks (every other case: DEFAULT_KS)
DEFAULT_KS = (7,)
_CASES = None


def _build_cases():
    rng = np.random.default_rng(20261019)
    out = []
    # ---- one key of every type + an int32 key of five values, at every row count, both directions
    cols = _type_columns(rng)
    tie = pa.array(rng.integers(-2, 3, N_MAX), pa.int32())
    for ty in TYPE_NAMES:
        full = pa.table({"k": cols[ty], "tie": tie})
        for n in ROWS:
            t = full.slice(0, n)
            out.append(("%s_%d_asc" % (ty, n), t, [(0, False), (1, False)]))
            out.append(("%s_%d_desc" % (ty, n), t, [(0, True), (1, True)]))
    # ---- eight keys (the limit), directions mixed, each key of a handful of values so that all eight decide somewhere
    n = N_MAX
    eight = pa.table({
        "a": pa.array(rng.integers(-1, 2, n), pa.int8()),
        "b": pa.array([bytes([c, 0, 0, 0]) for c in rng.choice(list(b"NR"), n)], pa.binary(4)),
        "c": pa.array(rng.integers(-1, 1, n), pa.int32()).cast(pa.date32()),
        "d": dec_array([int(v) for v in rng.integers(-1, 2, n)], 12, 2),
        "e": pa.array(rng.choice([0.0, -0.0, -1.5], n)),
        "f": str_array([[b"", b"a", b"a\0"][i] for i in rng.integers(0, 3, n)]),
        "g": dec_array([int(v) * 2 ** 64 for v in rng.integers(-1, 2, n)], 38, 0),
        "h": pa.array(rng.integers(0, 2, n), pa.int64()),
        "i": pa.array(rng.integers(0, 3, n), pa.int16()),  # the ninth column: one key too many for the device
    })
    for n in (3000, 4097, 20000):
        out.append(("eight_keys_%d" % n, eight.slice(0, n), [(0, False), (1, True), (2, False), (3, True), (4, False), (5, True), (6, False), (7, True)]))
    # ---- radix digit skipping and stability
    for n in (4097, 20000):
        r = rng.integers(0, 16, n)
        tie_n = tie.slice(0, n)
        out.append(("all_equal_%d" % n, pa.table({"k": pa.array(np.full(n, 42, np.int64)), "tie": pa.array(np.full(n, -7, np.int32))}), [(0, False), (1, True)]))
        hi = pa.array((r.astype(np.uint64) << np.uint64(60)).view(np.int64))  # only bits 60..63 differ (the sign bit among them)
        out.append(("bits_60_63_%d_asc" % n, pa.table({"k": hi, "tie": tie_n}), [(0, False), (1, False)]))
        out.append(("bits_60_63_%d_desc" % n, pa.table({"k": hi, "tie": tie_n}), [(0, True), (1, False)]))
        lo = pa.array(np.int64(0x0123456789ABCDE0) + r)  # only bits 0..3 differ
        out.append(("bits_0_3_%d" % n, pa.table({"k": lo, "tie": tie_n}), [(0, False), (1, False)]))
        out.append(("const_first_%d" % n, pa.table({"k": pa.array(np.full(n, I64_MIN, np.int64)), "v": pa.array(rng.integers(-(2 ** 31), 2 ** 31, n), pa.int32())}), [(0, False), (1, False)]))
    # ---- top-k: what the radix select in front of it can get wrong (all inputs > 4096 rows)
    n = 6000
    # (a) nothing to select on within the first four key words: every row is a candidate
    a = pa.table({"c0": pa.array(np.full(n, 5, np.int64)), "c1": pa.array(np.full(n, -5, np.int64)), "c2": pa.array(np.full(n, I64_MAX, np.int64)),
                  "c3": pa.array(np.full(n, 0, np.int64)), "v": pa.array(rng.integers(-50, 50, n), pa.int64())})
    out.append(("topk_a_const_words", a, [(0, False), (1, False), (2, True), (3, False), (4, False)]))
    TOPK_KS["topk_a_const_words"] = (10, 100, 4097)
    # (b) all eight bytes of the leading key vary (the pass budget is spent on it) and one value is shared by 5000 rows: the second key decides
    lead = rng.integers(I64_MIN, I64_MAX, n, endpoint=True)
    shared = rng.permutation(n)[:5000]
    lead[shared] = 0x0102030405060708
    below = int((lead < 0x0102030405060708).sum())
    b = pa.table({"k": pa.array(lead), "v": pa.array(rng.integers(-(2 ** 31), 2 ** 31, n), pa.int32())})
    out.append(("topk_b_shared_lead", b, [(0, False), (1, False)]))
    TOPK_KS["topk_b_shared_lead"] = (below, below + 1, below + 2500, below + 5000, below + 5001)
    assert 0 < below and below + 5000 < n
    # (c) exactly 4096 / 4097 rows hold the smallest leading value
    for cand in (4096, 4097):
        m = 9000
        lead = rng.integers(-1000, 1000, m).astype(np.int32)
        lead[rng.permutation(m)[:cand]] = -1001
        assert int((lead == lead.min()).sum()) == cand
        out.append(("topk_c_%d_candidates" % cand, pa.table({"k": pa.array(lead), "v": pa.array(rng.integers(-(2 ** 31), 2 ** 31, m), pa.int32())}), [(0, False), (1, False)]))
        TOPK_KS["topk_c_%d_candidates" % cand] = (10, cand, cand + 1)
    # (d) 128-bit decimals of both signs, descending
    out.append(("topk_d_dec33_desc", pa.table({"k": cols["dec33_4"].slice(0, n), "tie": tie.slice(0, n)}), [(0, True), (1, False)]))
    TOPK_KS["topk_d_dec33_desc"] = (10, 4096, 4097)
    # (e) a string key whose first 40 bytes say nothing
    out.append(("topk_e_prefix40", pa.table({"k": cols["utf8_prefix40"].slice(0, n), "tie": tie.slice(0, n)}), [(0, False), (1, True)]))
    TOPK_KS["topk_e_prefix40"] = (10, 1000)
    # (f) k at the ends
    m = 8193
    out.append(("topk_f_k_ends", pa.table({"k": cols["int32"].slice(0, m), "tie": tie.slice(0, m)}), [(0, True), (1, False)]))
    TOPK_KS["topk_f_k_ends"] = (0, 1, m - 1, m, m + 1)
    # zeros of both signs around the k-th row: equal keys, the second key and the input order decide
    z = rng.choice([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324], n, p=[0.3, 0.3, 0.1, 0.1, 0.1, 0.1])
    out.append(("topk_zero_signs", pa.table({"k": pa.array(z), "tie": tie.slice(0, n)}), [(0, False), (1, False)]))
    TOPK_KS["topk_zero_signs"] = (int((z < 0).sum()) + 50, n // 2)
    return out


def cases():
    """yields (name, pyarrow table, specs = [(column index, descending)]); tables are shared between cases and must not be changed"""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return iter(_CASES)


def topk_ks(name):
    return TOPK_KS.get(name, DEFAULT_KS)
