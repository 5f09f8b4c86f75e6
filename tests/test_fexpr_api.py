"""f32 / f64 expression programs without a device: the instruction encoder of Rel.map_expr, and the numpy reference
evaluator of tests/test_gpu_fexpr.py against hand-computed cases (the GPU tests compare the kernels with that evaluator
bit for bit, so it is pinned here on its own)."""
import struct

import numpy as np

from lingodb_amd import api, capi

import test_gpu_fexpr as fx


def bits64(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def test_encoder_fills_the_float_instructions():
    prog = [("col", (0, 2)), ("fconst", 0.85, 64), ("fmul",), ("fconst", -1.5, 32), ("fcvt", 64), ("fadd",), ("col", (1, 0)), ("i2f", 64), ("fsub",),
            ("fconst", 3.0, 64), ("fdiv",), ("f2i",), ("col", (0, 0)), ("fcvt", 32), ("fconst", 0.0, 32), ("fcmp", capi.F_GTE), ("const", -7), ("cmp", capi.F_LT)]
    arr = api.encode_xprog(prog)
    assert len(arr) == len(prog)
    assert [x.op for x in arr] == [capi.X_COL, capi.X_FCONST, capi.X_FMUL, capi.X_FCONST, capi.X_FCVT, capi.X_FADD, capi.X_COL, capi.X_I2F, capi.X_FSUB, capi.X_FCONST,
                                   capi.X_FDIV, capi.X_F2I, capi.X_COL, capi.X_FCVT, capi.X_FCONST, capi.X_FCMP, capi.X_CONST, capi.X_CMP]
    assert (capi.X_FCONST, capi.X_FADD, capi.X_FSUB, capi.X_FMUL, capi.X_FDIV, capi.X_FCMP, capi.X_I2F, capi.X_F2I, capi.X_FCVT) == tuple(range(17, 26))
    assert arr[1].lo == struct.unpack("<q", struct.pack("<d", 0.85))[0] and arr[1].arg == 64
    assert arr[3].lo == bits64(-1.5) and arr[3].arg == 32  # always the f64 bits: the library rounds to the slot's width
    assert arr[4].arg == 64 and arr[7].arg == 64 and arr[13].arg == 32
    assert arr[15].arg == capi.F_GTE and arr[17].arg == capi.F_LT
    assert (arr[6].col.side, arr[6].col.col) == (1, 0)
    assert (arr[16].lo, arr[16].hi) == (-7, -1)
    assert api.encode_xprog([("fconst", 1, 64)])[0].lo == bits64(1.0)  # a Python int is a float constant too


def cols_of(bits, *vals):
    return {(0, j): (bits, np.array(v, fx.F[bits]), np.ones(len(v), bool)) for j, v in enumerate(vals)}


def test_reference_keeps_two_roundings():
    """a = b = 1 + 2^-12, c = -(1 + 2^-11) in f32: a*b rounds to 1 + 2^-11 (a tie, to even), so a*b + c = 0; one fused rounding gives 2^-24.
    The f64 triple at 2^-27 / 2^-26: 0 against 2^-54."""
    for bits, fused in ((32, 2.0 ** -24), (64, 2.0 ** -54)):
        a, b, c = fx.triple(bits)
        kind, v, ok = fx.eval_prog(fx.ABC, cols_of(bits, [a], [b], [c]), 1)
        assert kind == bits and ok.all() and v.dtype == fx.F[bits]
        assert v[0] == 0.0
        exact = (int(a * 2 ** 60) * int(b * 2 ** 60) + int(c * 2 ** 60) * 2 ** 60)  # the operands are exact multiples of 2^-60
        assert exact == int(fused * 2 ** 120) and exact != 0, "what a fused multiply-add would return differs from the two-rounding result"


def test_reference_compares_ordered():
    nan = float("nan")
    a, b = [nan, 1.0, nan, 1.0, 2.0, -0.0], [1.0, nan, nan, 1.0, 1.0, 0.0]
    want = {capi.F_EQ: [0, 0, 0, 1, 0, 1], capi.F_NEQ: [0, 0, 0, 0, 1, 0], capi.F_LT: [0, 0, 0, 0, 0, 0], capi.F_LTE: [0, 0, 0, 1, 0, 1],
            capi.F_GT: [0, 0, 0, 0, 1, 0], capi.F_GTE: [0, 0, 0, 1, 1, 1]}
    for bits in (32, 64):
        for op, w in want.items():
            kind, v, ok = fx.eval_prog([("col", (0, 0)), ("col", (0, 1)), ("fcmp", op)], cols_of(bits, a, b), 6)
            assert kind == "i" and ok.all() and [int(x) for x in v] == w, (bits, op)


def test_reference_f2i_limits():
    vals = [-(2.0 ** 63), 2.0 ** 63, float(np.nextafter(2.0 ** 63, 0)), float("nan"), float("inf"), float("-inf"), 1e30, -1e30, -0.999, 2.5, -2.5, -0.0]
    kind, v, ok = fx.eval_prog([("col", (0, 0)), ("f2i",)], cols_of(64, vals), len(vals))
    assert kind == "i"
    assert ok.tolist() == [True, False, True, False, False, False, False, False, True, True, True, True]
    assert [int(x) for x in v[ok]] == [-2 ** 63, 2 ** 63 - 1024, 0, 2, -2, 0]
    kind, v, ok = fx.eval_prog([("col", (0, 0)), ("f2i",)], cols_of(32, [-(2.0 ** 63), 2.0 ** 63, 2.0 ** 63 - 2.0 ** 39, -7.75]), 4)
    assert ok.tolist() == [True, False, True, True] and [int(x) for x in v[ok]] == [-2 ** 63, 2 ** 63 - 2 ** 39, -7]


def test_reference_i2f_rounds_once():
    """100-bit integers.  f32 keeps 24 bits: ulp(2^99 … 2^100) = 2^76, half = 2^75.  Rounding through f64 first (ulp 2^47) would
    turn 2^99 + 2^75 + 1 into the tie 2^99 + 2^75 and then round it DOWN to even — one rounding goes up."""
    one = fx.int_to_float
    v = (1 << 99) + (1 << 75) + 1
    assert float(one(v, 32)) == float((1 << 99) + (1 << 76))
    assert float(np.float32(np.float64(float(v)))) == float(1 << 99), "the double rounding this case tells apart"
    assert float(one((1 << 99) + (1 << 75), 32)) == float(1 << 99)  # an exact tie: to even
    assert float(one((1 << 99) + (3 << 75), 32)) == float((1 << 99) + (2 << 76))  # a tie above an odd mantissa: up
    assert float(one(-v, 32)) == -float((1 << 99) + (1 << 76))
    assert float(one((1 << 100) - 1, 32)) == float(1 << 100)
    assert one(0, 32) == 0 and float(one((1 << 24) + 1, 32)) == float(1 << 24) and float(one((1 << 24) + 3, 32)) == float((1 << 24) + 4)
    # f64 keeps 53 bits: ulp = 2^47, half = 2^46
    w = (1 << 99) + (1 << 46) + 1
    assert float(one(w, 64)) == float((1 << 99) + (1 << 47)) and float(one(w - 1, 64)) == float(1 << 99)
    assert float(one(-((1 << 99) + (3 << 46)), 64)) == -float((1 << 99) + (2 << 47))
    assert one(v, 32).dtype == np.float32 and one(w, 64).dtype == np.float64
    kind, got, ok = fx.eval_prog([("col", (0, 0)), ("i2f", 32)], {(0, 0): ("i", np.array([v, -v], object), np.array([True, False]))}, 2)
    assert kind == 32 and ok.tolist() == [True, False] and float(got[0]) == float((1 << 99) + (1 << 76))


def test_reference_nulls_select_coalesce():
    a = (32, np.array([1.0, 2.0, 3.0], np.float32), np.array([True, False, True]))
    b = (32, np.array([9.0, 8.0, 7.0], np.float32), np.array([True, True, False]))
    kind, v, ok = fx.eval_prog([("col", (0, 0)), ("col", (0, 1)), ("coalesce",)], {(0, 0): a, (0, 1): b}, 3)
    assert ok.tolist() == [True, True, True] and v.tolist() == [1.0, 8.0, 3.0]
    kind, v, ok = fx.eval_prog([("col", (0, 0)), ("col", (0, 1)), ("fcmp", capi.F_LT), ("col", (0, 0)), ("col", (0, 1)), ("select",)], {(0, 0): a, (0, 1): b}, 3)
    assert ok.tolist() == [True, True, False] and v[:2].tolist() == [1.0, 8.0]  # a NULL condition takes the else branch
    kind, v, ok = fx.eval_prog([("col", (0, 0)), ("fconst", 0.0, 32), ("fdiv",)], {(0, 0): a}, 3)
    assert ok.tolist() == [True, False, True] and np.isinf(v[0])  # IEEE, not NULL
