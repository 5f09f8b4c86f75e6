"""The inputs of tests/test_gpu_join_edges.py, before any device sees them: for every case of join_ref.cases() the oracle's join
(oracle/ldb_oracle.c, no residuals, eight kinds) must give what join_ref's dict-and-walk join gives, and join_ref's partner lists — with
residual conjuncts, and key-less as the nested-loop join — must be those of a two-loop brute force over all pairs.  No GPU; what is proven
here is that the generator produces what it claims and that the references agree on it."""
import numpy as np
import pyarrow as pa
import pytest

import join_ref as J
import order_ref
from oracle_bind import HostRel, HostTable

CASES = {c.name: c for c in J.cases()}
NL = {name: (b, p, r) for name, b, p, r in J.nl_cases()}
_host = {}


def host_rel(rel):
    sides = []
    for t, r in rel.sides:
        if id(t) not in _host:
            _host[id(t)] = (t, HostTable(t))
        sides.append((_host[id(t)][1], r))
    return HostRel(sides, rel.n)


def sorted_rows(*cols):
    m = np.stack([np.asarray(c, dtype=np.int64) for c in cols], axis=1) if len(cols[0]) else np.zeros((0, len(cols)), np.int64)
    return m[np.lexsort(m.T[::-1])]


def test_the_generator_holds_what_it_claims():
    assert len(CASES) == sum(1 for _ in J.cases())
    for n in (0, 1, 63, 64, 65, 2047, 2048, 2049):
        assert CASES["probe_rows_%d" % n].probe.num_rows == n
    lazy = [c for c in CASES.values() if c.via and c.via[0] == "lazy"]
    assert len(lazy) >= 4 * 4
    for c in lazy:  # every lazily filtered probe has the five tiles: none, all, one queue round, two rounds (the second of one entry), a last row
        assert c.probe.num_rows == 4 * J.TILE + 1, c.name
        f = np.array(J.values(c.probe.column(5)))
        assert [int((f[t * J.TILE : (t + 1) * J.TILE] >= 1).sum()) for t in range(5)] == [0, 2048, 1024, 1025, 1] and int((f == 2).sum()) == 1, c.name
    for c in CASES.values():  # the radix-clustered probe takes one 4-byte key column without NULLs
        if "join_radix" in c.options:
            assert len(c.pkeys) == 1 and c.probe.column(0).null_count == 0 and c.probe.column(0).type == pa.int32(), c.name
    ends = set(J.values(CASES["int32_ends"].build.column(0)))
    assert {J.I32_MIN, J.I32_MAX} <= ends
    assert max(J.values(CASES["int32_ends_wide_probe"].probe.column(0))) > J.I32_MAX
    for name in ("float32_key", "float64_key"):
        for t in (CASES[name].build, CASES[name].probe):
            a = t.column(0).to_numpy()
            assert np.isnan(a).any() and ((a == 0) & np.signbit(a)).any() and ((a == 0) & ~np.signbit(a)).any()
    nb = J.values(CASES["null_keys_unique"].build.column(0))
    assert nb[0] is None and nb[-1] is None and nb[63] is None and nb[64] is None
    npk = J.values(CASES["null_keys_unique"].probe.column(0))
    assert npk[0] is None and npk[-1] is None and npk[63] is None and npk[64] is None
    lens = sorted({len(r) for r in J.partners(CASES["hashed_to_chained"].build_rel(), [(0, 0)], CASES["hashed_to_chained"].probe_rel(), [(0, 0)])})
    assert lens == [0, 1, 600]
    assert all(c.build.num_rows <= 4000 and c.probe.num_rows <= 10000 for c in CASES.values())
    for name in ("all_match_rank", "all_match_rank/rowid", "all_match_rank/joined"):
        c = CASES[name]
        assert all(len(r) == 1 for r in J.partners(c.build_rel(), c.bkeys, c.probe_rel(), c.pkeys))
        c = CASES[name.replace("all_match", "one_miss")]
        assert sum(1 for r in J.partners(c.build_rel(), c.bkeys, c.probe_rel(), c.pkeys) if not r) == 1
    assert len(CASES["all_match_rank/joined"].probe_rel().sides) == 2
    c = CASES["only_partner_fails"]
    part = J.partners(c.build_rel(), c.bkeys, c.probe_rel(), c.pkeys, c.residuals[0])
    assert all(not r for r in part) and any(J.partners(c.build_rel(), c.bkeys, c.probe_rel(), c.pkeys))
    c = CASES["direct_chained"]  # the first partner fails a residual that a later one passes
    plain, res = J.partners(c.build_rel(), c.bkeys, c.probe_rel(), c.pkeys), J.partners(c.build_rel(), c.bkeys, c.probe_rel(), c.pkeys, J.RESID_SET[2])
    assert any(a and b and a[0] != b[0] for a, b in zip(plain, res))


def test_join_on_hand_made_rows():
    b = pa.table({"k": pa.array([1, 2, None, 2, 5], pa.int32()), "x": pa.array([10, None, 30, 40, 50], pa.int64())})
    p = pa.table({"k": pa.array([2, None, 7, 1, 2], pa.int64()), "y": pa.array([40, 1, 2, None, 5], pa.int32())})
    B, P, k = J.Rel([(b, None)]), J.Rel([(p, None)]), [(0, 0)]
    N = J.NULL_ROW
    assert [a.tolist() for a in J.join(B, k, P, k, J.INNER)] == [[0, 0, 3, 4, 4], [1, 3, 0, 1, 3]]
    assert [a.tolist() for a in J.join(B, k, P, k, J.LEFT_OUTER)] == [[0, 0, 1, 2, 3, 4, 4], [1, 3, N, N, 0, 1, 3]]
    assert J.join(B, k, P, k, J.SEMI).tolist() == [0, 3, 4] and J.join(B, k, P, k, J.ANTI).tolist() == [1, 2]
    assert J.join(B, k, P, k, J.MARK).tolist() == [1, 0, 0, 1, 1]
    assert J.join(B, k, P, k, J.SINGLE) == [[1, 3], [], [], [0], [1, 3]]
    assert J.join(B, k, P, k, J.SEMI_BUILD).tolist() == [0, 1, 3] and J.join(B, k, P, k, J.ANTI_BUILD).tolist() == [2, 4]
    assert [a.tolist() for a in J.join(B, k, P, k, J.RIGHT_OUTER)] == [[0, 0, 3, 4, 4], [1, 3, 0, 1, 3], [2, 4]]
    assert [a.tolist() for a in J.join(B, k, P, k, J.FULL_OUTER)] == [[0, 0, 1, 2, 3, 4, 4], [1, 3, N, N, 0, 1, 3], [2, 4]]
    res = [((0, 1), J.GTE, (0, 1))]  # y >= x: NULL on either side fails
    assert [a.tolist() for a in J.join(B, k, P, k, J.INNER, res)] == [[0], [3]]
    assert J.join(B, k, P, k, J.ANTI, res).tolist() == [1, 2, 3, 4]
    assert J.join(B, k, P, k, J.INNER, anti_preds=[((0, 1), J.LT, 10)]).tolist() == [0]  # rows 1, 3 have the partner y = 5
    assert [a.tolist() for a in J.join(B, [], P, [], J.INNER, [((0, 1), J.EQ, (0, 1))])] == [[0], [3]]  # nested loop
    assert len(J.join(B, [], P, [], J.INNER)[0]) == 25
    z = pa.table({"k": pa.array([0.0, -0.0, float("nan")])})
    Z = J.Rel([(z, None)])
    assert [a.tolist() for a in J.join(Z, k, Z, k, J.INNER)] == [[0, 1], [0, 1]]


def test_the_tags_still_collide(oracle):
    for kind, pair, ty in (("int64", J.COLLIDING_INT64, pa.int64()), ("utf8", J.COLLIDING_UTF8, None)):
        assert pair is not None and pair[0] != pair[1]
        col = pa.array(list(pair), ty) if ty else order_ref.str_array(list(pair))
        h = oracle.hash_keys(HostTable(pa.table({"k": col})).rel(), [(0, 0)])
        assert h[0] >> np.uint64(32) == h[1] >> np.uint64(32)
        assert J.find_tag_collision(oracle, kind) == pair


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_join_equals_the_plain_join(oracle, name):
    c = CASES[name]
    B, P = c.build_rel(), c.probe_rel()
    part = J.partners(B, c.bkeys, P, c.pkeys)
    hb, hp = host_rel(B), host_rel(P)
    for kind in J.ORACLE_KINDS:
        want = J.from_partners(part, B.n, kind)
        op, ob, mk = oracle.join(hb, c.bkeys, hp, c.pkeys, kind)
        tag = J.KIND_NAMES[kind]
        if kind in (J.INNER, J.LEFT_OUTER):
            assert np.array_equal(sorted_rows(op, ob), sorted_rows(*want)), tag
        elif kind == J.SINGLE:
            assert np.array_equal(op, np.arange(P.n, dtype=np.uint32)), tag
            assert all((b in rows) if rows else b == J.NULL_ROW for b, rows in zip(ob.tolist(), want)), tag
        elif kind == J.MARK:
            assert np.array_equal(mk, want), tag
        else:
            assert np.array_equal(op, want), tag


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.residuals] + list(NL))
def test_plain_join_equals_two_loops(name):
    if name in NL:
        b, p, r = NL[name]
        B, P = J.Rel([(b, None)]), J.Rel([(p, None)])
        assert J.partners(B, [], P, [], r) == J.brute(B, [], P, [], r)
        return
    c = CASES[name]
    B, P = c.build_rel(), c.probe_rel()
    if P.n > 200:  # (every 31st row or so, the key edges in front among them: the two loops are slow)
        P = P.select(np.unique(np.concatenate([np.arange(8), np.arange(0, P.n, P.n // 150 + 1)])))
    for r in [[]] + c.residuals:
        assert J.partners(B, c.bkeys, P, c.pkeys, r) == J.brute(B, c.bkeys, P, c.pkeys, r), r
