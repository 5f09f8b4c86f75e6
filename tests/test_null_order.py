"""ORDER BY over nullable keys, without a device: the plain-Python comparator of tests/null_order_ref.py — what tests/test_gpu_null_order.py
compares the device with — against (a) ORDER BY cases transcribed from the reference's own SQL suite (tests/golden/ref_null_order.json, made
by tests/golden/make_ref_null_order.py), (b) order_ref.sort on NULL-free input, (c) hand cases of the three NULL rules; and (d) the NULL
order field of api.sort_spec."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

import null_order_ref
import order_ref
from lingodb_amd import api, capi

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_null_order.json")) as f:
    FIXTURE = json.load(f)
NULL_FREE = [(name, table, specs) for name, table, specs in order_ref.cases() if table.num_rows <= 4097]


def fixture_table(case, order):
    """the rows a fixture case expects, rearranged by `order`, as a table: column 0 is the sort key; further columns are kept where they are
    integers or NULL throughout (they serve as extra keys)"""
    rows = [case["expected"][i] for i in order]
    key = [r[0] for r in rows]
    cols = {"key": order_ref.str_array([v.encode() if v is not None else b"" for v in key]) if case["key_type"] == "utf8" else pa.array([v or 0 for v in key], pa.int32())}
    cols["key"] = null_order_ref.with_validity(cols["key"], [v is not None for v in key])
    for c in range(1, len(rows[0]) if rows else 1):
        vals = [r[c] for r in rows]
        if all(v is None or (isinstance(v, int) and not isinstance(v, bool)) for v in vals):
            cols["c%d" % c] = pa.array(vals, pa.int64())
    return pa.table(cols)


def fixture_orders(case):
    """input orders to sort a fixture case from: as expected, reversed, and two seeded shuffles"""
    n = len(case["expected"])
    rng = np.random.default_rng(n + 1)
    return [list(range(n)), list(range(n))[::-1], rng.permutation(n).tolist(), rng.permutation(n).tolist()]


def test_fixture_has_the_cases_it_is_for():
    assert len(FIXTURE) >= 6
    ints = [c for c in FIXTURE if c["table"] == "integers"]
    assert len(ints) >= 6 and all(c["input"] == [1, 2, 3, None] for c in ints)
    assert all(c["sql"].endswith("ORDER BY i;") and [r[0] for r in c["expected"]][-1] is None for c in ints)  # the NULL row is last, every time
    assert sum(1 for c in ints if all(r[1] is None for r in c["expected"])) >= 2  # a second column that is NULL in every row
    assert any(c["table"] == "strings" and c["expected"][-1] == [None] for c in FIXTURE)
    assert any(c["limit"] is not None for c in FIXTURE)


@pytest.mark.parametrize("case", FIXTURE, ids=[c["source"].rsplit(":", 1)[1] for c in FIXTURE])
def test_comparator_reproduces_the_reference_suite(case):
    for order in fixture_orders(case):
        table = fixture_table(case, order)
        got = null_order_ref.sort(table, [(0, False)])
        if case["limit"] is not None:
            got = got[: case["limit"]]
        # the keys of the fixture are distinct, so the expected order is the only one: row `order[p]` of the expected rows stands at position p
        assert [order[p] for p in got] == list(range(len(case["expected"]))), order
        if table.num_columns > 1 and table.column(1).null_count == table.num_rows and table.num_rows:
            assert np.array_equal(null_order_ref.sort(table, [(1, False), (0, False)]), got)  # an all-NULL leading key: the next key decides alone
            assert np.array_equal(null_order_ref.sort(table, [(1, True), (0, False)]), got)


@pytest.mark.parametrize("name", [c[0] for c in NULL_FREE])
def test_equals_order_ref_on_null_free_input(name):
    _, table, specs = next(c for c in NULL_FREE if c[0] == name)
    assert np.array_equal(null_order_ref.sort(table, specs), order_ref.sort(table, specs))


def test_desc_puts_nulls_first():
    t = pa.table({"k": pa.array([5, None, -3, None, 9], pa.int64())})
    assert null_order_ref.sort(t, [(0, False)]).tolist() == [2, 0, 4, 1, 3]
    assert null_order_ref.sort(t, [(0, True)]).tolist() == [1, 3, 4, 0, 2]


def test_two_nulls_tie_and_the_second_key_decides():
    t = pa.table({"k": pa.array([None, 1, None, None], pa.int32()), "v": pa.array([7, 0, -7, 7], pa.int32())})
    assert null_order_ref.sort(t, [(0, False), (1, False)]).tolist() == [1, 2, 0, 3]  # rows 0 and 3 tie on both keys: input order
    assert null_order_ref.sort(t, [(0, False), (1, True)]).tolist() == [1, 0, 3, 2]
    assert null_order_ref.sort(t, [(0, True), (1, False)]).tolist() == [2, 0, 3, 1]


def test_all_null_key_leaves_the_order_to_the_next_key():
    t = pa.table({"k": pa.array([None] * 5, pa.float64()), "v": order_ref.str_array([b"b", b"", b"\0", b"a", b""])})
    for desc in (False, True):
        assert null_order_ref.sort(t, [(0, desc), (1, False)]).tolist() == [1, 4, 2, 3, 0]
    nulls = pa.table({"k": t.column(0), "v": null_order_ref.with_validity(t.column(1).chunk(0), [True, False, True, True, True])})
    assert null_order_ref.sort(nulls, [(0, False), (1, False)]).tolist() == [4, 2, 3, 0, 1]  # NULL, b"" and b"\0" are three keys


def test_bytes_under_a_null_are_not_looked_at():
    cases = {name: (table, specs) for name, table, specs in null_order_ref.cases()}
    for ty, top in (("int64", null_order_ref.I64_MAX), ("utf8", b"\xff\xff"), ("float64", float("inf"))):
        table, specs = cases["under_null_%s_41_asc" % ty]
        vals = null_order_ref.column_values(table.column(0))
        order = null_order_ref.expected("under_null_%s_41_asc" % ty).tolist()
        n_valid = sum(v is not None for v in vals)
        assert all(vals[r] is not None for r in order[:n_valid]) and all(vals[r] is None for r in order[n_valid:])
        assert vals[order[n_valid - 1]] == top  # the largest valid value stands right before the NULLs
        ties = table.column(1).to_pylist()
        tail = [(ties[r], r) for r in order[n_valid:]]
        assert tail == sorted(tail)  # the NULLs tie: the tie key, then the input position


def test_padding_row_ids_are_null():
    t = pa.table({"k": pa.array([10, 20, 30], pa.int32())})
    rowids = np.array([2, 0xFFFFFFFF, 0, 1, 0xFFFFFFFF], dtype=np.uint32)
    assert null_order_ref.sort_rel([(t, rowids)], 5, [(0, 0, False)]).tolist() == [2, 3, 0, 1, 4]
    assert null_order_ref.sort_rel([(t, rowids)], 5, [(0, 0, True)]).tolist() == [1, 4, 0, 3, 2]


def test_sort_spec_carries_the_null_order():
    assert (capi.NULLS_REFUSE, capi.NULLS_LARGEST) == (0, 1)
    s = api.sort_spec((1, 2))
    assert (s.col.side, s.col.col, s.descending, s.nulls) == (1, 2, 0, capi.NULLS_REFUSE)
    s = api.sort_spec((0, 3), True)
    assert (s.descending, s.nulls) == (1, 0)
    s = api.sort_spec((0, 3), nulls=capi.NULLS_LARGEST)
    assert (s.descending, s.nulls) == (0, 1)
    assert api.sort_spec((0, 0), True, capi.NULLS_LARGEST).nulls == 1
    assert [f[0] for f in capi.SortSpec._fields_] == ["col", "descending", "nulls"]
