"""String expressions as computed columns (ldb_gpu_map_strcat / ldb_gpu_map_strlen), the CPU half: the Python restatement of
the reference's string runtime reproduces every recorded output of tests/golden/ref_strfn.json (written by
tests/golden/make_ref_strfn.py from the reference's own StringRuntime), the new symbols are exported and bound, the plan
checker knows the four new `map` forms, and the sub-operator translator turns ToUpper / ToLower / StringLength / Concatenate
into them.  The device half is tests/test_gpu_strfn.py."""
import ctypes as C
import copy
import json
import os
import subprocess
import tempfile

import pytest

from lingodb_amd import api, capi
import strfn_eval as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fx():
    return E.load_fixture()


def test_fixture_covers_what_it_must(fx):
    s = fx["strings"]
    assert 200 <= len(s) <= 400 and os.path.getsize(E.FIXTURE) < 100 << 10
    assert {0, 11, 12, 13} <= {len(b) for b in s}
    seen = set().union(*[set(b) for b in s])
    assert set(range(0x61, 0x7B)) | set(range(0x41, 0x5B)) | set(range(0x30, 0x3A)) <= seen
    lead = {b[i] for b in s for i in range(len(b)) if b[i] >= 0xC0}
    assert any(0xC2 <= c <= 0xDF for c in lead) and any(0xE0 <= c <= 0xEF for c in lead) and any(c >= 0xF0 for c in lead)
    assert "ß".encode() in s and "É".encode() in s and len({c for c in seen if c >= 0x80}) >= 64
    for b in s:
        b.decode("utf-8")  # valid sequences only
    assert {0, 1, -1, 2 ** 63 - 1, -(2 ** 63)} <= set(fx["ints"]) and all(10 ** k in fx["ints"] and -(10 ** k) in fx["ints"] and 10 ** k - 1 in fx["ints"] for k in range(1, 19))


def test_evaluator_reproduces_the_reference(fx):
    s = fx["strings"]
    for i, b in enumerate(s):
        assert E.upper(b) == fx["upper"][i], b
        assert E.lower(b) == fx["lower"][i], b
        assert E.length(b) == fx["length"][i], b
    for i in range(len(s) - 1):
        assert s[i] + s[i + 1] == fx["concat_next"][i]
        assert E.strcat_row([{"col": s}, {"col": s[1:]}], i) == fx["concat_next"][i]
    for v, t in zip(fx["ints"], fx["from_int"]):
        assert E.from_int(v) == t
    assert len(fx["substr"]) >= 200
    for c in fx["substr"]:
        assert E.substr(s[c["i"]], c["from"], c["for"]) == c["out"], c
    # bytes >= 0x80 pass through the case mappings (the header says so because the reference does)
    assert E.upper("straße é".encode()) == "STRAßE é".encode() and fx["upper"][s.index("ß".encode())] == "ß".encode()


def test_symbols_and_struct_layout():
    lib = capi.gpu_lib()
    for n in ("ldb_gpu_map_strcat", "ldb_gpu_map_strlen"):
        assert hasattr(lib, n) and n in capi.GPU_API
    prog = r'''
#include "lingodb_gpu.h"
#include <stdio.h>
#include <stddef.h>
int main(void){ printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d %lld\n", sizeof(ldb_strpart), offsetof(ldb_strpart, col), offsetof(ldb_strpart, str), offsetof(ldb_strpart, str_len),
  offsetof(ldb_strpart, for_len), LDB_MAX_STRPARTS, LDB_SP_COL, LDB_SP_CONST, LDB_SP_INT, LDB_SC_NONE, LDB_SC_UPPER, LDB_SC_LOWER, (long long) LDB_STR_WHOLE); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        with open(src, "w") as f:
            f.write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P = capi.StrPart
    assert got == [C.sizeof(P), P.col.offset, P.str.offset, P.str_len.offset, P.for_len.offset, capi.LDB_MAX_STRPARTS, capi.SP_COL, capi.SP_CONST, capi.SP_INT, capi.SC_NONE, capi.SC_UPPER,
                   capi.SC_LOWER, capi.STR_WHOLE]
    arr, n, _ = api.str_parts(["store", {"col": (0, 1), "case": "upper", "from": 1, "for": 4}, {"int": (0, 2)}])
    assert n == 3 and (arr[0].kind, arr[0].str_len, arr[0].str) == (capi.SP_CONST, 5, b"store")
    assert (arr[1].kind, arr[1].strcase, arr[1].col.col, arr[1].from_, arr[1].for_len) == (capi.SP_COL, capi.SC_UPPER, 1, 1, 4)
    assert (arr[2].kind, arr[2].col.col, arr[2].from_, arr[2].for_len) == (capi.SP_INT, 2, 1, capi.STR_WHOLE)


def check(plan, inputs=("t",)):
    lib = capi.host_lib()
    arr = (C.c_char_p * len(inputs))(*[n.encode() for n in inputs])
    st = lib.ldb_plan_json_check(json.dumps(plan).encode(), arr, len(inputs))
    return st, lib.ldb_plan_json_last_error().decode()


def plan_of(step):
    return {"inputs": ["t"], "steps": [{"op": "scan", "table": "t", "out": "r"}, dict(step, **{"op": "map", "in": "r", "out": "r2"})], "result": "r2"}


CONCAT = {"fn": "concat", "as": "k", "parts": [{"const": "store"}, {"col": "s_id", "case": "upper", "from": 1, "for": 4}, {"int": "s_key"}]}


@pytest.mark.parametrize("step", [{"fn": "upper", "col": "c_name", "as": "u"}, {"fn": "lower", "col": "c_name", "as": "u"}, {"fn": "length", "col": "c_name", "as": "u"}, CONCAT,
                                  {"fn": "concat", "as": "k", "parts": [{"col": "a"}]}])
def test_checker_accepts_the_new_map_forms(step):
    st, err = check(plan_of(step))
    assert st == capi.LDB_OK, err


def without(d, k):
    return {a: b for a, b in d.items() if a != k}


@pytest.mark.parametrize("step, word", [
    (without(CONCAT, "parts"), "parts"),
    (dict(CONCAT, parts="abc"), "parts"),
    (dict(CONCAT, parts=[]), "parts"),
    (dict(CONCAT, parts=[{"const": "x"}] * 9), "9 parts"),
    (dict(CONCAT, parts=[{"col": "a", "case": "title"}]), "case"),
    (dict(CONCAT, parts=[{"const": "x"}, {}]), "part 1"),
    (dict(CONCAT, parts=[{"const": "x", "col": "a"}]), "exactly one"),
    (dict(CONCAT, parts=[{"col": "a", "int": "b"}]), "exactly one"),
    (dict(CONCAT, parts=[{"const": "x", "case": "upper"}]), "case"),
    (dict(CONCAT, parts=[{"int": "k", "from": 2}]), "from"),
    ({"fn": "upper", "as": "u"}, "col"),
    ({"fn": "initcap", "col": "a", "as": "u"}, "initcap"),
])
def test_checker_rejects_malformed_forms(step, word):
    st, err = check(plan_of(step))
    assert st == capi.LDB_ERR_INVALID and word in err, err


# ---------------------------------------------------------------- translator: the dump of Q22 with its Substring node replaced, in memory
def leaf(name):
    return {"datatype": "str", "type": "expression_leaf", "leaf_type": "column", "displayName": name}


def const(v, t="str"):
    return {"type": "expression_leaf", "leaf_type": "constant", "data_type": t, "value": v}


def call(fn, *args):
    return {"type": "expression_inner", "strings": [fn + "("] + [", "] * (len(args) - 1) + [")"], "subExpressions": list(args)}


def q22_with(node):
    with open(os.path.join(GOLD, "subop_tpch_q22.json")) as f:
        doc = json.load(f)
    hits = []

    def walk(x):
        if isinstance(x, dict):
            for k, v in x.items():
                if isinstance(v, dict) and v.get("strings", [None])[0] == "Substring(":
                    hits.append(copy.deepcopy(v))
                    x[k] = node(v)
                else:
                    walk(v)
        elif isinstance(x, list):
            for i, v in enumerate(x):
                if isinstance(v, dict) and v.get("strings", [None])[0] == "Substring(":
                    hits.append(copy.deepcopy(v))
                    x[i] = node(v)
                else:
                    walk(v)

    walk(doc)
    assert len(hits) == 1
    return json.dumps(doc)


def fn_steps(text):
    plan = json.loads(text)
    ins = plan["inputs"]
    arr = (C.c_char_p * len(ins))(*[n.encode() for n in ins])
    assert capi.host_lib().ldb_plan_json_check(text.encode(), arr, len(ins)) == capi.LDB_OK, capi.host_lib().ldb_plan_json_last_error()
    return [s for s in plan["steps"] if s["op"] == "map" and "fn" in s]


@pytest.mark.parametrize("fn, want", [("ToUpper", "upper"), ("ToLower", "lower"), ("StringLength", "length")])
def test_translator_one_column_forms(fn, want):
    text, report = api.translate_subop_dump(q22_with(lambda sub: call(fn, leaf("customer::c_phone"))), "q22_" + want)
    assert all(r["target"] == "gpu" for r in report)
    maps = fn_steps(text)
    assert len(maps) == 1 and maps[0]["fn"] == want and maps[0]["col"] == "c_phone" and "parts" not in maps[0]


def test_translator_flattens_a_concatenate_nest():
    phone = leaf("customer::c_phone")
    nest = lambda sub: call("Concatenate", call("Concatenate", const("tel:"), call("ToUpper", sub)), call("Concatenate", phone, call("Concatenate", const("-"), call("ToLower", phone))))  # noqa: E731
    text, report = api.translate_subop_dump(q22_with(nest), "q22_concat")
    assert all(r["target"] == "gpu" for r in report)
    maps = fn_steps(text)
    assert len(maps) == 1 and maps[0]["fn"] == "concat"
    assert maps[0]["parts"] == [{"const": "tel:"}, {"col": "c_phone", "case": "upper", "from": 1, "for": 2}, {"col": "c_phone"}, {"const": "-"}, {"col": "c_phone", "case": "lower"}]


def test_translator_leaves_other_operands_to_the_cpu():
    phone = leaf("customer::c_phone")
    for inner in (call("Replace", phone, const("a"), const("b")), call("cast", phone), call("ToUpper", call("Concatenate", phone, phone))):
        if inner["strings"][0] == "cast(":
            inner["strings"] = ["cast(", ")"]
        with pytest.raises(capi.LdbError) as e:
            api.translate_subop_dump(q22_with(lambda sub: call("Concatenate", const("x"), inner)), "q22_cpu")
        assert e.value.status == capi.LDB_ERR_UNSUPPORTED and any(r["target"] == "cpu" for r in e.value.report), str(e.value)
