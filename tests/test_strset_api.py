"""The host half of the string-set scan (csrc/ldb_strset.hip) without a device: ldb_gpu_strset_plan sorts and deduplicates the constants of a
string IN list in the reference's string order (unsigned bytes, then length — Python's order on bytes), gives each its 64-bit prefix key and
says whether the workgroups stage the table in LDS.  The library's own host code lays the device table out from exactly this function.
Also: the option that routes small lists to the kernel is known, the plan checker takes a ten-string list, and the sub-operator translator
turns a string IN restriction of any size into one filter step."""
import ctypes as C
import json

import pytest

from lingodb_amd import api, capi

A40 = b"0123456789abcdefghijklmnopqrstuvwxyz!+-" + b"A"  # two 40-byte strings sharing their first 39 bytes
B40 = A40[:39] + b"B"
POOL = [b"abc", b"", b"ab\0", b"a", B40, b"ab", "é…".encode(), b"\xff", A40, b"ab", b"", b"\xff", A40]  # (duplicates included, not sorted)
assert len(A40) == len(B40) == 40 and A40[:39] == B40[:39]


def plan(consts):
    lib = capi.gpu_lib()
    n = len(consts)
    ptrs = (C.c_char_p * max(n, 1))(*consts)
    lens = (C.c_int32 * max(n, 1))(*[len(c) for c in consts])
    order = (C.c_int32 * max(n, 1))()
    keys = (C.c_uint64 * max(n, 1))()
    m, in_lds, lds_max = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    st = lib.ldb_gpu_strset_plan(ptrs, lens, n, order, keys, C.byref(m), C.byref(in_lds), C.byref(lds_max))
    assert st == capi.LDB_OK, lib.ldb_gpu_last_error()
    return list(order[: m.value]), list(keys[: m.value]), in_lds.value, lds_max.value


def key_of(b):
    return int.from_bytes(b[:8].ljust(8, b"\0"), "big")


def test_order_is_sorted_distinct_bytes():
    order, keys, in_lds, _ = plan(POOL)
    got = [POOL[i] for i in order]
    assert got == sorted(set(POOL))
    assert got[0] == b"" and got[-1] == b"\xff" and got.index(A40) + 1 == got.index(B40)
    assert order == [POOL.index(c) for c in got]  # of equal constants the first one listed
    assert in_lds == 1


def test_keys_are_the_big_endian_prefix_and_monotone():
    order, keys, _, _ = plan(POOL)
    got = [POOL[i] for i in order]
    assert keys == [key_of(c) for c in got]
    assert all(a <= b for a, b in zip(keys, keys[1:]))
    assert keys[got.index(b"\xff")] == 0xFF << 56 and keys[got.index(b"")] == 0


def test_nul_tail_ties_on_the_key_and_both_stay():
    order, keys, _, _ = plan(POOL)
    got = [POOL[i] for i in order]
    i, j = got.index(b"ab"), got.index(b"ab\0")
    assert j == i + 1 and keys[i] == keys[j]
    assert keys[got.index(A40)] == keys[got.index(B40)]  # (they differ behind the eighth byte)


def test_empty_list_and_single_constant():
    assert plan([])[:2] == ([], [])
    assert plan([b"x" * 100])[:2] == ([0], [key_of(b"x" * 8)])


def test_lds_decision_flips_at_the_documented_size():
    _, _, _, lds_max = plan([b"a"])
    assert lds_max == 5376  # (64 KB - 1 KB) / 12 bytes per constant, a multiple of the 256-thread block (ldb_strset.hip)
    consts = [b"%05d" % i for i in range(lds_max + 1)]
    order, keys, in_lds, _ = plan(consts[:lds_max])
    assert in_lds == 1 and len(order) == lds_max
    order, keys, in_lds, _ = plan(consts)
    assert in_lds == 0 and len(order) == lds_max + 1 and order == list(range(lds_max + 1))
    # duplicates do not count: the decision is taken over the distinct constants
    assert plan(consts[:lds_max] + consts[:50])[2] == 1


def test_bad_arguments_are_refused():
    lib = capi.gpu_lib()
    m = C.c_int32()
    assert lib.ldb_gpu_strset_plan(None, None, 3, None, None, C.byref(m), None, None) == capi.LDB_ERR_INVALID
    assert lib.ldb_gpu_strset_plan(None, None, -1, None, None, C.byref(m), None, None) == capi.LDB_ERR_INVALID
    assert lib.ldb_gpu_strset_plan(None, None, 0, None, None, None, None, None) == capi.LDB_ERR_INVALID
    assert lib.ldb_gpu_strset_plan(None, None, 0, None, None, C.byref(m), None, None) == capi.LDB_OK and m.value == 0


def test_routing_option_is_known():
    lib = capi.gpu_lib()
    assert lib.ldb_gpu_set_option(b"scan_strset_min_in", 9) == capi.LDB_OK  # (9 is the default: nothing changes)
    assert lib.ldb_gpu_get_option(b"scan_strset_min_in") == 9


def test_pred_passes_any_number_of_strings():
    vals = [b"c%03d" % i for i in range(300)] + [b"x" * 500]
    d, keep = api.pred((0, 2), capi.F_IN, values=vals)
    assert d.n_in == 301 and d.rhs_kind == capi.RHS_STRING
    assert [d.in_strs[k] for k in (0, 299)] == [vals[0], vals[299]] and d.in_str_lens[300] == 500
    d, keep = api.pred((0, 2), capi.F_GTE, b"y" * 100)
    assert d.str_len == 100 and d.rhs_kind == capi.RHS_STRING


COUNTRIES = ["ALGERIA", "ARGENTINA", "BRAZIL", "CANADA", "EGYPT", "ETHIOPIA", "FRANCE", "GERMANY", "INDIA", "UNITED KINGDOM, THE ISLE OF MAN AND THE CHANNEL ISLANDS OF"]


def string_in_dump():
    """SELECT n_nationkey FROM nation WHERE n_name IN (ten strings, one of 60 bytes) as the reference's sub-operator dump: the restriction is pushed
    into the scan's datasource properties"""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [p for p in (os.path.join(root, "tools"),) if p not in sys.path]
    import subop_lower as L

    cx = L.Cx("str_in")
    t = L.Table("nation", filters=[("n_name", "IN", COUNTRIES)])
    return L.result(cx, t, [("n_nationkey", t["n_nationkey"])], write=False)


def test_string_in_restriction_translates_to_one_filter_step():
    assert len(COUNTRIES) == 10 and len(COUNTRIES[-1]) > 48
    text, report = api.translate_subop_dump(string_in_dump(), "str_in")
    assert report and all(r["target"] == "gpu" for r in report), report
    steps = json.loads(text)["steps"]
    filters = [s for s in steps if s["op"] == "filter"]
    assert len(filters) == 1
    assert filters[0]["preds"] == [{"col": "n_name", "op": "IN", "values": COUNTRIES}]


def test_plan_checker_takes_a_ten_string_list_and_a_long_constant():
    plan_text = json.dumps({"name": "strset", "inputs": ["t"], "steps": [
        {"op": "filter", "in": "t", "out": "f", "preds": [{"col": "s", "op": "IN", "values": COUNTRIES}, {"col": "s", "op": "GTE", "value": "A" * 60}]},
        {"op": "materialize", "in": "f", "cols": ["i"], "out": "r"}], "result": "r"})
    lib = capi.host_lib()
    arr = (C.c_char_p * 1)(b"t")
    assert lib.ldb_plan_json_check(plan_text.encode(), arr, 1) == capi.LDB_OK, lib.ldb_plan_json_last_error()
