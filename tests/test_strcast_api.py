"""Casts between text and int / decimal / date (ldb_gpu_map_strparse, the DECIMAL / DATE parts of ldb_gpu_map_strcat), the
CPU half: tests/strcast_eval.py — the plain-Python restatement the device results are compared with — agrees with pyarrow
(whose Decimal128::FromString / ToString and date parser the reference's StringRuntime calls), the new symbol and enum
values are exported and bound, and the plan checker knows the new `map` forms.  The device half is tests/test_gpu_strcast.py.

Where pyarrow is NOT the yardstick (each such string is asserted to be bad in the restatement instead of being compared):
  - a decimal text outside the domain of arrow's own arithmetic: more than 38 significant digits (the accumulator wraps:
    '9' * 39 casts to -20847100762815390390123822295304634369 at (38, 0)), a scale-to-zero product past 2^127 ('99e37' casts
    to a negative number; its overflow check compares the wrapped product with the operand and can miss), a parsed scale more
    than 38 above the target (Rescale reads past its table of multipliers);
  - a date in year 0000, which arrow parses and include/lingodb_gpu.h refuses: the text form is defined for 0001 … 9999."""
import ctypes as C
import decimal
import json
import os
import random
import subprocess
import tempfile

import pyarrow as pa
import pyarrow.compute as pc
import pytest

from lingodb_amd import api, capi
import strcast_eval as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEC_TABLE = [("+1.5", 150), ("-.5", -50), ("1.", 100), ("1e2", 10000), ("00012.30", 1230), ("-0", 0), (" 1.5", None), ("1.5 ", None), (".", None), ("", None), ("1_0", None), ("1.23E-1", None)]
DEC_MORE = ["9" * 38, "9" * 39, "1e37", "1e38", "1E-38", "1.230", "1.234", "1e2000000000", "0e2000000000", "1e-2000000000", "999999999999", "9999999999.99", "10000000000", "1e+-2", "1e-+2",
            "1e+", "1e", "e1", ".e1", "1.e1", ".1e1", "00e1", "1e01", "1e-0", "0e38", "0e39", "0." + "0" * 39, "0." + "0" * 37 + "1", "0" * 50 + "1", "1" + "0" * 38, "99e37", "+", "-", "+-1", "1+", "1e2147483647",
            "1e2147483648", "1e-2147483648", "1e-2147483649", "1E5", "１"]
DATE_CASES = ["0001-01-01", "9999-12-31", "1970-01-01", "1900-02-29", "2000-02-29", "2004-02-29", "2100-02-29", "1998-04-31", "1998-06-31", "1998-09-31", "1998-11-31", "1998-02-30", "1998-13-01",
              "1998-00-10", "1998-01-00", "1998-1-011", "1998-01-0", "1998-01-011", "1998 01-01", "1998-01-0 ", " 998-01-01", "+998-01-01", "199a-01-01", "1998/01/01", "", "0000-01-01", "0000-12-31"]
ALPHABET = "0123456789+-.eE "
TYPES = [(12, 2), (38, 0), (38, 38), (20, 8), (1, 0), (5, 5)]


def random_strings(seed, n):
    """seeded: plain draws over the alphabet at lengths 0 … 45 (nearly all bad), and draws shaped like numbers and dates"""
    rng = random.Random(seed)
    out = ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 45))) for _ in range(n)]
    dig = lambda k: "".join(rng.choice("0123456789") for _ in range(k))  # noqa: E731
    for _ in range(n):
        s = rng.choice(["", "", "+", "-"]) + dig(rng.randint(0, 22))
        if rng.random() < .6:
            s += "." + dig(rng.randint(0, 22))
        if rng.random() < .4:
            s += rng.choice("eE") + rng.choice(["", "+", "-", "+-"]) + dig(rng.randint(0, 3))
        if rng.random() < .15:
            k = rng.randint(0, len(s))
            s = s[:k] + rng.choice(ALPHABET) + s[k + rng.randint(0, 1):]
        out.append(s[:45])
    for _ in range(n // 2):
        out.append("%04d-%02d-%02d" % (rng.randint(0, 9999), rng.randint(0, 13), rng.randint(0, 32)))
    return out


def arrow_or_none(s, typ):
    try:
        return pc.cast(pa.array([s], pa.string()), typ)[0]
    except pa.ArrowInvalid:
        return None


def in_arrow_decimal_domain(s, scale):
    p = E.decimal_parts(s)
    if p is None:
        return True  # arrow refuses the text itself
    _, whole, frac, exp = p
    digits = (whole + frac).lstrip(b"0")
    parsed_scale = len(frac) - exp
    if len(digits) > 38 or parsed_scale - scale > 38:
        return False
    return not (-38 <= parsed_scale < scale and int(digits or b"0") * 10 ** (scale - parsed_scale) >= 2 ** 127)  # (an int128 wraps)


def test_to_decimal_against_pyarrow():
    for s, want in DEC_TABLE:
        assert E.to_decimal(s, 12, 2) == want, s
    compared = accepted = 0
    for s in [c[0] for c in DEC_TABLE] + DEC_MORE + random_strings(11, 1500):
        for p, sc in TYPES:
            got = E.to_decimal(s, p, sc)
            if not in_arrow_decimal_domain(s, sc):
                assert got is None, (s, p, sc)
                continue
            ref = arrow_or_none(s, pa.decimal128(p, sc))
            want = None if ref is None else int(ref.as_py().scaleb(sc, context=decimal.Context(prec=80)))
            assert got == want, (s, p, sc, got, want)
            compared += 1
            accepted += want is not None
    assert compared > 15000 and accepted > 1000  # (the shaped draws: not everything is bad)


def test_to_date_against_pyarrow():
    ok = 0
    for s in DATE_CASES + random_strings(12, 1500):
        got = E.to_date(s)
        if s.startswith("0000-"):
            assert got is None, s
            continue
        ref = arrow_or_none(s, pa.date32())
        assert got == (None if ref is None else ref.value), s
        ok += got is not None
    assert ok > 300 and E.to_date("0001-01-01") == E.DATE_MIN and E.to_date("9999-12-31") == E.DATE_MAX and E.to_date("1970-01-01") == 0


def stoll(s):
    """std::stoll(s, &pos) with pos == len(s), restated directly: strtoll's subject sequence in base 10, then the range"""
    b = s.encode() if isinstance(s, str) else s
    k = 0
    while k < len(b) and b[k:k + 1].isspace() and b[k] < 0x80:
        k += 1
    j = k + (1 if b[k:k + 1] in (b"+", b"-") else 0)
    e = j
    while e < len(b) and 0x30 <= b[e] <= 0x39:
        e += 1
    if e == j or e != len(b):
        return None  # invalid_argument, or pos != len
    v = int(b[k:e])  # (Python's int only ever sees sign? digits+)
    return v if -(2 ** 63) <= v <= 2 ** 63 - 1 else None  # out_of_range


def test_to_int_against_stoll():
    cases = ["9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "+0", "-0", "0" * 30 + "12", "\t\n 12", "12 ", "1 2", "0x10", "+", "", " " * 4096 + "7", "- 1", "+-1",
             "\v\f\r-77", "1e2", "1.0", "１", b"\xa0" + b"1", b"\x1c1", "99999999999999999999999"]
    seen = 0
    for s in cases + random_strings(13, 1500):
        assert E.to_int(s) == stoll(s), s
        seen += E.to_int(s) is not None
    assert seen > 100
    assert E.to_int("-9223372036854775808") == -(2 ** 63) and E.to_int("9223372036854775808") is None and E.to_int("\t\n 12") == 12 and E.to_int(" " * 4096 + "7") == 7


DEC_VALUES = sorted({0} | {s * v for k in (1, 2, 5, 7, 8, 18, 19, 20, 37) for v in (1, 10 ** k - 1, 10 ** k) for s in (1, -1)} | {10 ** 38 - 1, -(10 ** 38 - 1), 5, -5, 12, -12, 99, 100})


def test_from_decimal_and_from_date_against_pyarrow():
    for (p, sc), vals, texts in [((12, 2), [5, -5, 0, -100], ["0.05", "-0.05", "0.00", "-1.00"]), ((20, 8), [1, 99, 100, 0, -12], ["1E-8", "9.9E-7", "0.00000100", "0E-8", "-1.2E-7"])]:
        assert [E.from_decimal(v, sc).decode() for v in vals] == texts
    rng = random.Random(3)
    for sc in (0, 2, 6, 7, 8, 19, 38):
        vals = DEC_VALUES + [rng.randrange(-10 ** 38 + 1, 10 ** 38) // 10 ** rng.randint(0, 37) for _ in range(300)]
        with decimal.localcontext() as c:
            c.prec = 60
            arr = pa.array([decimal.Decimal(v).scaleb(-sc) for v in vals], pa.decimal128(38, sc))
        assert [E.from_decimal(v, sc).decode() for v in vals] == pc.cast(arr, pa.string()).to_pylist(), sc
    days = [E.DATE_MIN, E.DATE_MAX, 0, 11016, -25509, 59, 60, -1] + [rng.randint(E.DATE_MIN, E.DATE_MAX) for _ in range(2000)]
    assert [E.from_date(d).decode() for d in days] == pc.cast(pa.array(days, pa.int32()).cast(pa.date32()), pa.string()).to_pylist()
    assert E.from_date(E.DATE_MIN - 1) is None and E.from_date(E.DATE_MAX + 1) is None
    # the round trips the device test relies on
    assert all(E.to_date(E.from_date(d)) == d for d in days)
    assert all(E.to_decimal(E.from_decimal(v, sc), 38, sc) == v for sc in (0, 2, 6, 7, 8, 38) for v in DEC_VALUES)
    assert all(E.to_int(E.from_int(v)) == v for v in (0, -1, 2 ** 63 - 1, -(2 ** 63)))


def test_symbol_and_enum_values():
    lib = capi.gpu_lib()
    assert hasattr(lib, "ldb_gpu_map_strparse") and "ldb_gpu_map_strparse" in capi.GPU_API
    prog = r'''
#include "lingodb_gpu.h"
#include <stdio.h>
#ifdef CHECK_PROTOTYPE /* (compiled only: an incompatible prototype is an error) */
int32_t (*f)(ldb_ctx*, ldb_rel*, ldb_colref, int32_t, int32_t, int32_t, const char*, ldb_table**, int64_t*) = ldb_gpu_map_strparse;
#endif
int main(void){ printf("%d %d %d %d %d %d %d %d %zu\n", LDB_SP_COL, LDB_SP_CONST, LDB_SP_INT, LDB_SP_DECIMAL, LDB_SP_DATE, LDB_PARSE_INT64, LDB_PARSE_DECIMAL, LDB_PARSE_DATE, sizeof(ldb_strpart)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-Werror", "-DCHECK_PROTOTYPE", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", os.path.join(d, "s.o")])
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [capi.SP_COL, capi.SP_CONST, capi.SP_INT, capi.SP_DECIMAL, capi.SP_DATE, capi.PARSE_INT64, capi.PARSE_DECIMAL, capi.PARSE_DATE, C.sizeof(capi.StrPart)]
    assert (capi.SP_DECIMAL, capi.SP_DATE) == (3, 4) and (capi.PARSE_INT64, capi.PARSE_DECIMAL, capi.PARSE_DATE) == (0, 1, 2)
    arr, n, _ = api.str_parts(["x", {"dec": (0, 1)}, {"date": (1, 2)}, {"int": (0, 3)}])
    assert n == 4 and [(a.kind, a.col.side, a.col.col) for a in arr[1:4]] == [(capi.SP_DECIMAL, 0, 1), (capi.SP_DATE, 1, 2), (capi.SP_INT, 0, 3)]
    assert all((a.strcase, a.from_, a.for_len) == (capi.SC_NONE, 1, capi.STR_WHOLE) for a in arr[1:4])


def check(plan, inputs=("t",)):
    lib = capi.host_lib()
    arr = (C.c_char_p * len(inputs))(*[n.encode() for n in inputs])
    st = lib.ldb_plan_json_check(json.dumps(plan).encode(), arr, len(inputs))
    return st, lib.ldb_plan_json_last_error().decode()


def plan_of(step):
    return {"inputs": ["t"], "steps": [{"op": "scan", "table": "t", "out": "r"}, dict(step, **{"op": "map", "in": "r", "out": "r2"})], "result": "r2"}


@pytest.mark.parametrize("step", [
    {"fn": "to_varchar", "col": "o_totalprice", "as": "v"},
    {"fn": "to_int", "col": "s", "as": "v"},
    {"fn": "to_int", "col": "s", "as": "v", "on_error": "null"},
    {"fn": "to_decimal", "col": "s", "as": "v", "precision": 12, "scale": 2},
    {"fn": "to_decimal", "col": "s", "as": "v", "precision": 38, "scale": 0, "on_error": "fail"},
    {"fn": "to_date", "col": "s", "as": "v", "on_error": "null"},
    {"fn": "concat", "as": "k", "parts": [{"const": "#"}, {"dec": "o_totalprice"}, {"col": "c"}, {"date": "o_orderdate"}, {"int": "k"}]},
])
def test_checker_accepts_the_new_forms(step):
    st, err = check(plan_of(step))
    assert st == capi.LDB_OK, err


@pytest.mark.parametrize("step, word", [
    ({"fn": "to_decimal", "col": "s", "as": "v", "precision": 12}, "scale"),
    ({"fn": "to_decimal", "col": "s", "as": "v", "scale": 2}, "precision"),
    ({"fn": "to_int", "col": "s", "as": "v", "scale": 2}, "scale"),
    ({"fn": "to_date", "col": "s", "as": "v", "precision": 2}, "precision"),
    ({"fn": "to_int", "col": "s", "as": "v", "on_error": "skip"}, "skip"),
    ({"fn": "to_int", "as": "v"}, "col"),
    ({"fn": "to_varchar", "as": "v"}, "col"),
    ({"fn": "concat", "as": "k", "parts": [{"dec": "a", "col": "b"}]}, "exactly one of"),
    ({"fn": "concat", "as": "k", "parts": [{"date": "a", "int": "b"}]}, "exactly one of"),
    ({"fn": "concat", "as": "k", "parts": [{"date": "a", "case": "upper"}]}, "case"),
    ({"fn": "concat", "as": "k", "parts": [{"dec": "a", "from": 2}]}, "from"),
])
def test_checker_rejects_malformed_forms(step, word):
    st, err = check(plan_of(step))
    assert st == capi.LDB_ERR_INVALID and word in err, err
