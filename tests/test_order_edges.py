"""The inputs of tests/test_gpu_order_edges.py, before any device sees them: for every case of order_ref.cases() the oracle's sort and top-k
(oracle/ldb_oracle.c, the checker of the GPU suite) must give exactly the row order of order_ref's comparator — a second, plainer statement
of db.sort_compare.  No GPU; what is proven here is that the generator produces what it claims and that the two references agree on it."""
import numpy as np
import pyarrow as pa
import pytest

import order_ref
from oracle_bind import HostTable

CASES = {name: (table, specs) for name, table, specs in order_ref.cases()}
_want = {}


def want_order(name):
    if name not in _want:
        _want[name] = order_ref.sort(*CASES[name])
    return _want[name]


def test_the_generator_holds_what_it_claims():
    names = list(CASES)
    assert len(names) == len(set(names)) == sum(1 for _ in order_ref.cases())
    for ty in order_ref.TYPE_NAMES:
        for n in order_ref.ROWS:
            assert CASES["%s_%d_asc" % (ty, n)][0].num_rows == n
    f64 = order_ref.column_values(CASES["float64_3000_asc"][0].column(0))
    f32 = order_ref.column_values(CASES["float32_3000_asc"][0].column(0))
    for vals, tiny in ((f64, 5e-324), (f32, float(np.float32(1e-45)))):
        signs = [bool(np.signbit(v)) for v in vals if v == 0.0]
        steps = set(zip(signs, signs[1:]))
        assert (True, False) in steps and (False, True) in steps  # zeros of both signs, met in both input orders
        assert {tiny, -tiny, float("inf"), float("-inf")} <= set(vals) and tiny > 0.0
    assert min(order_ref.column_values(CASES["date32_3000_asc"][0].column(0))) < 0
    d38 = set(order_ref.column_values(CASES["dec38_0_3000_asc"][0].column(0)))
    assert {10 ** 38 - 1, 1 - 10 ** 38, 2 ** 63, -(2 ** 63), 2 ** 64, -(2 ** 64), 2 ** 64 + 1, -(2 ** 64) - 1, 2 ** 64 - 1, 1 - 2 ** 64, -1, 0} <= d38
    s = set(order_ref.column_values(CASES["utf8_3000_asc"][0].column(0)))
    assert {b"", b"a", b"ab", b"ab\0", b"a\0", b"\x7f", b"\x80", b"\xff", b"Z" * 256, b"Z" * 255} <= s
    assert all(v.startswith(order_ref.PREFIX40[:39]) for v in order_ref.column_values(CASES["utf8_prefix40_3000_asc"][0].column(0)))
    assert CASES["eight_keys_4097"][0].num_columns == 9 and len(CASES["eight_keys_4097"][1]) == 8
    assert all(t.num_rows <= 20000 for t, _ in CASES.values())
    assert all(CASES[name][0].num_rows > 4096 for name in order_ref.TOPK_KS)


def test_comparator_on_hand_made_rows():
    t = pa.table({"f": pa.array([0.0, -0.0, -0.0, 0.0, -1.0]), "id": pa.array([1, 2, 0, 0, 9], pa.int32()), "s": order_ref.str_array([b"ab", b"a", b"a\0", b"", b"\xff"])})
    assert order_ref.sort(t, [(0, False), (1, False)]).tolist() == [4, 2, 3, 0, 1]  # the zeros are one key: id decides, then position
    assert order_ref.sort(t, [(0, True)]).tolist() == [0, 1, 2, 3, 4]
    assert order_ref.sort(t, [(2, False)]).tolist() == [3, 1, 2, 0, 4]
    assert order_ref.sort(t, [(2, True)]).tolist() == [4, 0, 2, 1, 3]
    assert order_ref.topk(t, [(1, True)], 2).tolist() == [4, 1]


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_sort_and_topk_equal_the_plain_comparator(oracle, name):
    table, specs = CASES[name]
    rel = HostTable(table).rel()
    want = want_order(name)
    ospecs = order_ref.sort_specs(specs)
    assert np.array_equal(oracle.sort(rel, ospecs), want)
    for k in order_ref.topk_ks(name):
        assert np.array_equal(oracle.topk(rel, ospecs, k), want[:k]), k
