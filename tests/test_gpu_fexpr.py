"""f32 / f64 scalar expressions: ldb_gpu_map_expr with float columns, the F* instructions and float results (k_map_fexpr),
and the plan language's float operators, literals and casts.

Every result is compared BIT-EXACTLY (through .view(uint32 / uint64): -0.0, infinities and denormals included) with a plain
numpy evaluator of the postfix program that computes each instruction in the slot's own dtype, step by step — elementwise
IEEE operations have one correct answer, so there is no tolerance.  The one exception is NaN: only NaN-ness is compared
(payloads are not specified).  Validity is compared exactly.  Each case runs on the ahead-of-time kernel and on the run-time
specialised one."""
import ctypes as C
import decimal
import itertools
import json
import math

import numpy as np
import pyarrow as pa
import pytest

from lingodb_amd import api, capi

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 257, 100_003]  # bitmap word boundaries, a partial last wave, more rows than one pass of the small grid
F = {32: np.float32, 64: np.float64}
U = {32: np.uint32, 64: np.uint64}
T_OF = {32: capi.T_FLOAT32, 64: capi.T_FLOAT64}
CMP = {capi.F_EQ: lambda a, b: a == b, capi.F_NEQ: lambda a, b: (a < b) | (a > b), capi.F_LT: lambda a, b: a < b,
       capi.F_LTE: lambda a, b: a <= b, capi.F_GT: lambda a, b: a > b, capi.F_GTE: lambda a, b: a >= b}


# ------------------------------------------------------------------ the reference evaluator
def int_to_float(v, bits):
    """sitofp of an exact Python integer with ONE rounding, to nearest even (never through f64 for f32)"""
    if bits == 64:
        return np.float64(float(v))  # CPython rounds int → float correctly
    m = abs(int(v))
    sh = max(m.bit_length() - 24, 0)
    q, rem = m >> sh, m & ((1 << sh) - 1)
    if sh and (rem > (1 << (sh - 1)) or (rem == (1 << (sh - 1)) and (q & 1))):
        q += 1
    r = np.float32(math.ldexp(q, sh))  # q <= 2^24: exact in f64 and in f32
    return np.float32(-r) if v < 0 else r


def float_to_int(v):
    """fptosi to i64: None (NULL) for NaN and values outside [-2^63, 2^63)"""
    x = float(v)  # exact
    if x != x or not (-(2.0 ** 63) <= x < 2.0 ** 63):
        return None
    return int(x)


class Slot:
    def __init__(self, kind, val, nul):  # kind: "i" (object array of Python ints), 32, 64
        self.kind, self.val, self.nul = kind, val, nul


def eval_prog(prog, cols, n):
    """prog: the postfix list Rel.map_expr takes; cols: {(side, col): (kind, values, valid)} → (kind, values, valid)"""
    st = []
    ints = lambda xs: np.array([int(x) for x in xs], dtype=object)  # noqa: E731
    with np.errstate(all="ignore"):
        for ins in prog:
            op = ins[0]
            if op == "col":
                kind, v, ok = cols[tuple(ins[1])]
                st.append(Slot(kind, v.copy() if kind != "i" else ints(v), ~ok))
            elif op == "const":
                st.append(Slot("i", ints([ins[1]] * n), np.zeros(n, bool)))
            elif op == "fconst":
                st.append(Slot(ins[2], np.full(n, np.float64(ins[1]).astype(F[ins[2]]), F[ins[2]]), np.zeros(n, bool)))
            elif op in ("fadd", "fsub", "fmul", "fdiv"):
                b, a = st.pop(), st.pop()
                assert a.kind == b.kind and a.kind in (32, 64)
                r = {"fadd": np.add, "fsub": np.subtract, "fmul": np.multiply, "fdiv": np.divide}[op](a.val, b.val)
                assert r.dtype == F[a.kind]
                st.append(Slot(a.kind, r, a.nul | b.nul))
            elif op == "fcmp":
                b, a = st.pop(), st.pop()
                assert a.kind == b.kind and a.kind in (32, 64)
                st.append(Slot("i", ints(CMP[ins[1]](a.val, b.val)), a.nul | b.nul))
            elif op == "cmp":
                b, a = st.pop(), st.pop()
                st.append(Slot("i", ints([CMP[ins[1]](x, y) for x, y in zip(a.val, b.val)]), a.nul | b.nul))
            elif op in ("add", "sub", "mul"):
                b, a = st.pop(), st.pop()
                r = a.val + b.val if op == "add" else a.val - b.val if op == "sub" else a.val * b.val
                st.append(Slot("i", r, a.nul | b.nul))
            elif op == "i2f":
                a = st.pop()
                st.append(Slot(ins[1], np.array([int_to_float(x, ins[1]) for x in a.val], F[ins[1]]), a.nul))
            elif op == "f2i":
                a = st.pop()
                r = [float_to_int(x) for x in a.val]
                st.append(Slot("i", ints([0 if x is None else x for x in r]), a.nul | np.array([x is None for x in r], bool)))
            elif op == "fcvt":
                a = st.pop()
                st.append(Slot(ins[1], a.val.astype(F[ins[1]]), a.nul))
            elif op == "isnull":
                a = st.pop()
                st.append(Slot("i", ints(a.nul), np.zeros(n, bool)))
            elif op == "select":
                b, a, c = st.pop(), st.pop(), st.pop()
                assert a.kind == b.kind
                t = ~c.nul & (c.val != 0)
                st.append(Slot(a.kind, np.where(t, a.val, b.val), np.where(t, a.nul, b.nul)))
            elif op == "coalesce":
                b, a = st.pop(), st.pop()
                assert a.kind == b.kind
                st.append(Slot(a.kind, np.where(a.nul, b.val, a.val), a.nul & b.nul))
            else:
                raise KeyError(op)
    assert len(st) == 1
    return st[0].kind, st[0].val, ~st[0].nul


# ------------------------------------------------------------------ inputs
def triple(bits):
    """a = b, c with a*b + c = 0 in two roundings and 2^-24 (f32) / 2^-54 (f64) fused"""
    k = 12 if bits == 32 else 27
    t = F[bits]
    return t(1) + t(2.0 ** -k), t(1) + t(2.0 ** -k), -(t(1) + t(2.0 ** -(k - 1)))


def specials(bits):
    t = F[bits]
    fi = np.finfo(t)
    return [t(0.0), t(-0.0), t(np.inf), t(-np.inf), t(np.nan), t(fi.tiny / 4), t(fi.max), t(-fi.max), t(1.0), t(-fi.tiny / 4)]


def float_cols(bits, n, seed):
    """three columns: row 0 holds the fused / unfused triple, then every special of `a` meets a rotation of the specials in b and c,
    then seeded random values; about 10 % NULLs behind the specials"""
    rng = np.random.default_rng(seed)
    t = F[bits]
    sp = specials(bits)
    cols = []
    for j in range(3):
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(t)
        head = [triple(bits)[j]] + sp[j * 3:] + sp[:j * 3]
        k = min(n, len(head))
        v[:k] = head[:k]
        ok = rng.random(n) >= 0.1
        ok[:k] = True
        cols.append((v, ok))
    return cols


_seq = itertools.count()


def register(ctx, cols):
    """cols: [(name, arrow type, values, valid)] → device table"""
    arrays = {name: pa.array(v, type=ty, mask=None if ok is None else ~np.asarray(ok)) for name, ty, v, ok in cols}
    return ctx.register("fx_%d" % next(_seq), pa.table(arrays))


def column_of(table, i=0):
    """(values with NULLs zeroed, validity) of column i of a result table"""
    col = table.to_arrow().column(i).combine_chunks()
    valid = np.asarray(col.is_valid().to_numpy(zero_copy_only=False), bool)
    if pa.types.is_decimal(col.type):
        vals = np.array([0 if x is None else int(x.scaleb(col.type.scale, context=_WIDE)) for x in col.to_pylist()], dtype=object)
    elif pa.types.is_boolean(col.type):
        vals = np.array([bool(x) for x in col.fill_null(False).to_pylist()], dtype=object)
    elif pa.types.is_floating(col.type):
        vals = np.asarray(col.fill_null(0.0).to_numpy(zero_copy_only=False))
    else:
        vals = np.array([0 if x is None else int(x) for x in col.cast(pa.int64()).to_pylist()], dtype=object)
    return vals, valid


def assert_same(got, got_valid, kind, want, want_valid, what=""):
    assert np.array_equal(got_valid, want_valid), f"{what}: validity differs at rows {np.nonzero(got_valid != want_valid)[0][:8]}"
    ok = want_valid
    if kind == "i":
        bad = [i for i in np.nonzero(ok)[0] if int(got[i]) != int(want[i])]
        assert not bad, f"{what}: rows {bad[:8]}: got {[got[i] for i in bad[:8]]} want {[want[i] for i in bad[:8]]}"
        return
    assert got.dtype == F[kind], (what, got.dtype)
    g, w = got[ok], want[ok].astype(F[kind])
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: NaN-ness differs"
    num = ~np.isnan(w)
    gb, wb = g[num].view(U[kind]), w[num].view(U[kind])
    bad = np.nonzero(gb != wb)[0]
    assert bad.size == 0, f"{what}: {bad.size} values differ in their bits, first: got {g[num][bad[:4]]!r} want {w[num][bad[:4]]!r}"


def run_and_check(rel, prog, cols, n, out_type, p=0, s=0, what=""):
    kind, want, want_valid = eval_prog(prog, cols, n)
    got, got_valid = column_of(rel.map_expr(prog, out_type, p, s))
    assert len(got) == n
    assert_same(got, got_valid, kind, want, want_valid, what)


# ------------------------------------------------------------------ generic / specialised
def _jit_launches():
    a, b, ms = C.c_int64(), C.c_int64(), C.c_double()
    capi.gpu_lib().ldb_gpu_jit_stats(C.byref(a), C.byref(b), C.byref(ms))
    return a.value + b.value


@pytest.fixture(scope="module", params=["generic", "spec"])
def mode(request):
    """'spec': every launch specialised at run time (this module is not in conftest's fixed list, so it switches itself)"""
    lib = capi.gpu_lib()
    if request.param == "generic":
        yield "generic"
        return
    lib.ldb_gpu_set_option(b"jit_min_rows", 0)
    before = _jit_launches()
    yield "spec"
    lib.ldb_gpu_set_option(b"jit_min_rows", 4000000)
    assert _jit_launches() > before, "spec mode ran without a single specialised kernel"


ABC = [("col", (0, 0)), ("col", (0, 1)), ("fmul",), ("col", (0, 2)), ("fadd",)]


# ------------------------------------------------------------------ 1. arithmetic
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("bits", [32, 64])
def test_arithmetic(ctx, mode, bits, n):
    """a*b + c in two roundings (row 0 tells a fused multiply-add apart), (a - b) / c, a / ±0: IEEE, never NULL"""
    (a, oa), (b, ob), (c, oc) = float_cols(bits, n, 100 + bits)
    ty = pa.float32() if bits == 32 else pa.float64()
    rel = register(ctx, [("a", ty, a, oa), ("b", ty, b, ob), ("c", ty, c, oc)]).rel()
    cols = {(0, 0): (bits, a, oa), (0, 1): (bits, b, ob), (0, 2): (bits, c, oc)}
    run_and_check(rel, ABC, cols, n, T_OF[bits], what="a*b+c")
    run_and_check(rel, [("col", (0, 0)), ("col", (0, 1)), ("fsub",), ("col", (0, 2)), ("fdiv",)], cols, n, T_OF[bits], what="(a-b)/c")
    for zero in (0.0, -0.0):
        run_and_check(rel, [("col", (0, 0)), ("fconst", zero, bits), ("fdiv",)], cols, n, T_OF[bits], what=f"a/{zero}")
    if oa[0] and ob[0] and oc[0]:
        got, _ = column_of(rel.map_expr(ABC, T_OF[bits]))
        assert got[0] == 0.0, "a*b+c was contracted into a fused multiply-add"


def test_more_rows_than_one_grid_pass(ctx, mode):
    """the grid is capped at 8 workgroups per CU and a lane takes two rows per step: 1.2 M rows make every lane loop (MI355X: 256 CUs → 1 M rows per pass)"""
    n = 1_200_003
    (a, oa), (b, ob), (c, oc) = float_cols(32, n, 132)
    rel = register(ctx, [("a", pa.float32(), a, oa), ("b", pa.float32(), b, ob), ("c", pa.float32(), c, oc)]).rel()
    run_and_check(rel, ABC, {(0, 0): (32, a, oa), (0, 1): (32, b, ob), (0, 2): (32, c, oc)}, n, capi.T_FLOAT32, what="a*b+c, 1.2 M rows")


# ------------------------------------------------------------------ 2. comparisons, SELECT, COALESCE, ISNULL
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("bits", [32, 64])
def test_compare_select_coalesce(ctx, mode, bits, n):
    (a, oa), (b, ob), (c, oc) = float_cols(bits, n, 200 + bits)
    b = b.copy()
    b[n // 2:] = a[n // 2:]  # equal pairs too (NaN = NaN among them)
    ty = pa.float32() if bits == 32 else pa.float64()
    rel = register(ctx, [("a", ty, a, oa), ("b", ty, b, ob), ("c", ty, c, oc)]).rel()
    cols = {(0, 0): (bits, a, oa), (0, 1): (bits, b, ob), (0, 2): (bits, c, oc)}
    for op in (capi.F_EQ, capi.F_NEQ, capi.F_LT, capi.F_LTE, capi.F_GT, capi.F_GTE):  # NaNs on either side: ordered → false
        run_and_check(rel, [("col", (0, 0)), ("col", (0, 1)), ("fcmp", op)], cols, n, capi.T_BOOL8, what=f"fcmp {op}")
    run_and_check(rel, [("col", (0, 0)), ("col", (0, 1)), ("fcmp", capi.F_LT), ("col", (0, 0)), ("col", (0, 2)), ("select",)], cols, n, T_OF[bits], what="select")
    run_and_check(rel, [("col", (0, 0)), ("col", (0, 2)), ("coalesce",), ("fconst", 1.5, bits), ("coalesce",)], cols, n, T_OF[bits], what="coalesce")
    run_and_check(rel, [("col", (0, 0)), ("col", (0, 1)), ("fadd",), ("isnull",)], cols, n, capi.T_BOOL8, what="isnull")


# ------------------------------------------------------------------ 3. casts
_WIDE = decimal.Context(prec=60)  # the default context keeps 28 digits: too few for a decimal(38, 2)


def _dec(v, s):
    return decimal.Decimal(int(v)).scaleb(-s, context=_WIDE)


@pytest.mark.parametrize("n", ROWS)
def test_casts(ctx, mode, n):
    rng = np.random.default_rng(300)
    ok = rng.random(n) >= 0.1
    i32 = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    i64 = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
    head64 = [2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 63 - 1, -2 ** 63, 0, (1 << 25) + (1 << 1)]
    i64[:min(n, len(head64))] = head64[:n]
    d32 = rng.integers(-50_000, 50_000, n).astype(np.int32)
    d12 = [int(x) for x in rng.integers(-10 ** 12 + 1, 10 ** 12, n)]
    # decimal(38,2): |v| up to 2^100 with low bits set — the lost bits decide the rounding (sticky bit); exact ties as well
    big = [int(rng.integers(1, 2 ** 62)) << int(rng.integers(0, 39)) | int(rng.integers(0, 2 ** 20)) for _ in range(n)]
    big = [(-v if rng.random() < 0.5 else v) for v in big]
    head = [2 ** 100 - 1, (1 << 100) + (1 << 76), (1 << 100) + (1 << 76) + 1, (3 << 99) + (1 << 75), -((1 << 100) + (1 << 47) + 1), (1 << 100) + (1 << 47), (1 << 64), (1 << 64) - 1]
    big[:min(n, len(head))] = head[:n]
    f64 = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 8, n)).astype(np.float64)  # (times 10^6 stays inside decimal(15, 6))
    hf = [1e30, -1e30, np.nan, np.inf, -np.inf, -(2.0 ** 63), 2.0 ** 63, np.nextafter(2.0 ** 63, 0), -0.0, 0.999, -0.999, 1e300, np.finfo(np.float32).max * 2.0, 5e-324]
    f64[:min(n, len(hf))] = hf[:n]
    with np.errstate(all="ignore"):
        f32 = f64.astype(np.float32)
    t = register(ctx, [("i32", pa.int32(), i32, ok), ("i64", pa.int64(), i64, ok), ("d32", pa.date32(), d32, ok),
                       ("d12", pa.decimal128(12, 2), [_dec(v, 2) for v in d12], ok), ("big", pa.decimal128(38, 2), [_dec(v, 2) for v in big], ok),
                       ("f64", pa.float64(), f64, ok), ("f32", pa.float32(), f32, ok), ("d6", pa.decimal128(15, 6), [_dec(v, 6) for v in d12], ok)])
    rel = t.rel()
    cols = {(0, 0): ("i", i32, ok), (0, 1): ("i", i64, ok), (0, 2): ("i", d32, ok), (0, 3): ("i", np.array(d12, object), ok), (0, 4): ("i", np.array(big, object), ok),
            (0, 5): (64, f64, ok), (0, 6): (32, f32, ok), (0, 7): ("i", np.array(d12, object), ok)}
    for c in range(5):  # sitofp from int32, int64, date32, decimal(12,2), decimal(38,2)
        for bits in (32, 64):
            run_and_check(rel, [("col", (0, c)), ("i2f", bits)], cols, n, T_OF[bits], what=f"i2f col {c} → f{bits}")
    run_and_check(rel, [("col", (0, 6)), ("fcvt", 64)], cols, n, capi.T_FLOAT64, what="extf")
    run_and_check(rel, [("col", (0, 5)), ("fcvt", 32)], cols, n, capi.T_FLOAT32, what="truncf")
    run_and_check(rel, [("col", (0, 5)), ("f2i",)], cols, n, capi.T_INT64, what="f2i f64")
    run_and_check(rel, [("col", (0, 6)), ("f2i",)], cols, n, capi.T_INT64, what="f2i f32")
    for c, s in ((3, 2), (7, 6)):  # decimal → f64: sitofp(v) / (double) powf(10, s); f64 → decimal(15, s): fptosi(v * (double) powf(10, s))
        p10 = float(np.float32(10.0) ** np.float32(s))
        run_and_check(rel, [("col", (0, c)), ("i2f", 64), ("fconst", p10, 64), ("fdiv",)], cols, n, capi.T_FLOAT64, what=f"decimal scale {s} → f64")
        run_and_check(rel, [("col", (0, 5)), ("fconst", p10, 64), ("fmul",), ("f2i",)], cols, n, capi.T_DECIMAL128, 15, s, what=f"f64 → decimal(15,{s})")


# ------------------------------------------------------------------ 4. row ids and NULL rows
def test_rowids_and_null_rows(ctx, mode):
    """the input is a selection (row ids) and the build side of a LEFT OUTER join with unmatched probe rows (LDB_NULL_ROW → NULL)"""
    n = 5_000
    (a, oa), (b, ob), _ = float_cols(32, n, 400)
    k = np.arange(n, dtype=np.int32)
    t = register(ctx, [("k", pa.int32(), k, None), ("a", pa.float32(), a, oa), ("b", pa.float32(), b, ob)])
    sel = t.rel().scan_filter([api.pred((0, 0), capi.F_GTE, 7), api.pred((0, 0), capi.F_LT, 4_100)])
    ids = sel.rowids(0).astype(np.int64)
    assert len(ids) == 4_093
    prog = [("col", (0, 1)), ("col", (0, 2)), ("fmul",), ("col", (0, 1)), ("fsub",)]
    cols = {(0, 1): (32, a[ids], oa[ids]), (0, 2): (32, b[ids], ob[ids])}
    run_and_check(sel, prog, cols, len(ids), capi.T_FLOAT32, what="over row ids")
    pk = np.arange(0, 6_000, 3, dtype=np.int32)  # every third key; those < 7 or >= 4100 find no build row
    probe = register(ctx, [("pk", pa.int32(), pk, None)])
    out = sel.join_build([(0, 0)], unique=True).probe(probe.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    bid = out.rowids(1)
    miss = bid == capi.LDB_NULL_ROW
    assert miss.any() and not miss.all()
    at = np.where(miss, 0, bid).astype(np.int64)
    prog1 = [("col", (1, 1)), ("col", (1, 2)), ("fmul",), ("col", (1, 1)), ("fsub",)]
    cols1 = {(1, 1): (32, a[at], oa[at] & ~miss), (1, 2): (32, b[at], ob[at] & ~miss)}
    kind, want, want_valid = eval_prog(prog1, cols1, len(bid))
    got, got_valid = column_of(out.map_expr(prog1, capi.T_FLOAT32))
    assert not got_valid[miss].any(), "an unmatched row must be NULL"
    assert_same(got, got_valid, kind, want, want_valid, "over an outer join's build side")


# ------------------------------------------------------------------ 5. consumers of a mapped float column
def test_mapped_column_feeds_groupby_filter_sort(ctx, mode):
    n = 20_000
    rng = np.random.default_rng(500)
    g = rng.integers(0, 7, n).astype(np.int32)
    x = rng.integers(-40, 41, n).astype(np.float64)  # small integers: every sum is exact whatever the order of the atomics
    y = rng.integers(1, 5, n).astype(np.float64)
    ok = rng.random(n) >= 0.1
    t = register(ctx, [("g", pa.int32(), g, None), ("x", pa.float64(), x, ok), ("y", pa.float64(), y, None)])
    rel = t.rel()
    m = rel.map_expr([("col", (0, 1)), ("col", (0, 2)), ("fmul",), ("fconst", 2.0, 64), ("fadd",)], capi.T_FLOAT64)
    z = x * y + 2.0
    zr = rel.zip(m)
    res = zr.groupby([(0, 0)], [api.agg(capi.AGG_SUM, api.col_expr((1, 0), is_float=True), out_type=capi.T_FLOAT64)], est_groups=8).to_arrow()
    got = dict(zip(res.column(0).to_pylist(), res.column(1).to_pylist()))
    assert got == {int(k): float(z[(g == k) & ok].sum()) for k in range(7)}
    kept = zr.scan_filter([api.pred((1, 0), capi.F_GT, 50.5)]).rowids(0)
    assert sorted(kept.tolist()) == np.nonzero(ok & (z > 50.5))[0].tolist()
    only = zr.scan_filter([api.pred((1, 0), capi.F_NOTNULL)])
    order = only.sort([api.sort_spec((1, 0)), api.sort_spec((0, 0))]).rowids(0).astype(np.int64)
    assert len(order) == int(ok.sum()) and np.all(np.diff(z[order]) >= 0), "sort by the mapped column"


# ------------------------------------------------------------------ 6. plan language
def test_plan_language(ctx, mode):
    n = 3_000
    rng = np.random.default_rng(600)
    g = rng.integers(0, 11, n).astype(np.int32)
    cents = rng.integers(-10 ** 7, 10 ** 7, n)
    x = rng.random(n).astype(np.float32)
    y = (rng.random(n) * 8).astype(np.float32)
    okx = rng.random(n) >= 0.1
    t = register(ctx, [("g", pa.int32(), g, None), ("d", pa.decimal128(12, 2), [_dec(v, 2) for v in cents], None), ("x", pa.float32(), x, okx), ("y", pa.float32(), y, None),
                       ("k_int", pa.int32(), g, None)])
    avg = {"steps": [{"op": "groupby", "in": "t", "keys": ["g"], "aggs": [{"fn": "sum", "expr": "d", "as": "sum_dec"}, {"fn": "count_star", "as": "n"}], "est_groups": 16, "out": "a"},
                     {"op": "map", "in": "a", "expr": {"div": [{"cast": ["f64", "sum_dec"]}, {"cast": ["f64", "n"]}]}, "as": "avg", "out": "m"},
                     {"op": "sort", "in": "m", "by": ["g"], "out": "s"}, {"op": "materialize", "in": "s", "cols": ["g", "avg"], "out": "result"}], "result": "result"}
    want_avg = []
    for k in range(11):  # sitofp(sum) / (double) powf(10, 2), then / sitofp(n)
        s, c = int(cents[g == k].sum()), int((g == k).sum())
        want_avg.append(np.float64(float(s)) / np.float64(np.float32(10.0) ** np.float32(2)) / np.float64(c))
    case = {"steps": [{"op": "map", "in": "t", "expr": {"case": [{"cmp": ["LT", "x", {"f32": "0.5"}]}, "x", "y"]}, "as": "z", "out": "m"},
                      {"op": "materialize", "in": "m", "cols": ["z"], "out": "result"}], "result": "result"}
    want_case = np.where(okx & (x < np.float32(0.5)), x, y)
    want_case_valid = np.where(okx & (x < np.float32(0.5)), okx, True)

    def check_avg(table):
        res = table.to_arrow()
        assert res.schema.field(1).type == pa.float64() and res.column(0).to_pylist() == list(range(11))
        got = np.asarray(res.column(1).to_numpy(zero_copy_only=False))
        assert np.array_equal(got.view(np.uint64), np.array(want_avg, np.float64).view(np.uint64))

    def check_case(table):
        got, valid = column_of(table)
        assert_same(got, valid, 32, want_case, want_case_valid, "case")

    check_avg(ctx.run_plan(json.dumps(avg), {"t": t}))
    check_case(ctx.run_plan(json.dumps(case), {"t": t}))
    for plan, check_fn in ((avg, check_avg), (case, check_case)):
        prepared = ctx.prepare_plan(json.dumps(plan))
        for _ in range(2):
            check_fn(prepared.execute({"t": t}))
        assert prepared.stats()["misses"] == 0
        prepared.release()
    mixed = {"steps": [{"op": "map", "in": "t", "expr": {"add": ["x", "k_int"]}, "as": "z", "out": "m"}, {"op": "materialize", "in": "m", "cols": ["z"], "out": "result"}], "result": "result"}
    with pytest.raises(capi.LdbError, match="cast"):
        ctx.run_plan(json.dumps(mixed), {"t": t})


# ------------------------------------------------------------------ 7. the verifier
def test_verifier_rejects_ill_typed_programs(ctx, mode):
    t = register(ctx, [("i", pa.int64(), np.arange(4, dtype=np.int64), None), ("f", pa.float32(), np.ones(4, np.float32), None), ("d", pa.float64(), np.ones(4, np.float64), None)])
    rel = t.rel()
    bad = [([("col", (0, 0)), ("col", (0, 1)), ("fadd",)], capi.T_FLOAT32, "instruction 2"),  # FADD over an int and a float
           ([("col", (0, 1)), ("col", (0, 2)), ("fmul",)], capi.T_FLOAT64, "instruction 2"),  # f32 mixed with f64
           ([("col", (0, 0)), ("i2f", 16)], capi.T_FLOAT32, "instruction 1"),  # arg = 16
           ([("col", (0, 1)), ("col", (0, 1)), ("add",)], capi.T_FLOAT32, "instruction 2"),  # floats under an integer op
           ([("col", (0, 1)), ("col", (0, 1)), ("fadd",)], capi.T_INT64, "instruction 2"),  # a float result with out_type INT64
           ([("col", (0, 0)), ("const", 1), ("add",)], capi.T_FLOAT64, "instruction 2")]  # an integer result with a float out_type
    for prog, out_type, where in bad:
        with pytest.raises(capi.LdbError) as e:
            rel.map_expr(prog, out_type)
        assert e.value.status == capi.LDB_ERR_INVALID and where in str(e.value), str(e.value)


# ------------------------------------------------------------------ 8. the integer path is where it was
def test_integer_programs_keep_their_kernel(ctx, mode):
    n = 1_000
    i = np.arange(n, dtype=np.int64)
    f = np.ones(n, np.float32)
    rel = register(ctx, [("i", pa.int64(), i, None), ("f", pa.float32(), f, None)]).rel()
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        rel.map_expr([("col", (0, 1)), ("col", (0, 1)), ("fadd",)], capi.T_FLOAT32)
        fl = ctx.prof_all()
        assert fl.get("k_map_fexpr", (0, 0.0))[0] == 1 and fl.get("k_map_expr", (0, 0.0))[0] == 0
        got, valid = column_of(rel.map_expr([("col", (0, 0)), ("const", 3), ("mul",), ("const", 1), ("add",)], capi.T_INT64))
        after = ctx.prof_all()
        assert after.get("k_map_expr", (0, 0.0))[0] == 1 and after.get("k_map_fexpr", (0, 0.0))[0] == 1
        assert valid.all() and [int(v) for v in got] == (i * 3 + 1).tolist()
    finally:
        ctx.prof_enable(False)
