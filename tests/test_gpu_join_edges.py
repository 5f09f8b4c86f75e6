"""The hash join (csrc/ldb_join.hip, ldb_join_kernel.h) and the nested-loop join at the edges of their build layouts, key types, probe paths
and sizes: every kind over every layout, residual conjuncts against an independent answer, NULL and float keys, keys at the ends of int32
and on the layout thresholds, tag collisions, tile and queue boundaries of the fused-filter probe, the radix-clustered probe.  Every
comparison is bit-exact equality of row-id vectors with tests/join_ref.py (a plain-Python join) and, where the oracle can express the
case, with oracle/ldb_oracle.c; tests/test_join_edges.py checks those two against each other without a device.  Row order is compared
wherever include/lingodb_gpu.h promises one (the radix-clustered probe promises none for the pair-shaped kinds), sorted rows everywhere
else.  Inputs come from join_ref.cases(); every table is registered once per module, every case builds its table once and probes it with
all its kinds.  A lazily filtered probe relation is made anew for every probe (the kinds that need the row set apply the filter to the
relation they are given, and it would stay applied), and the profile's launch counts tell whether the filter was still pending when the
probe kernel ran and whether the probe side was clustered.  debug_check is on for the whole module."""
import gc

import numpy as np
import pyarrow as pa
import pytest

import join_ref as J
from lingodb_amd import api, capi
from oracle_bind import HostRel, HostTable

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in J.cases()}
NL = {name: (b, p, r) for name, b, p, r in J.nl_cases()}
PAIR_KINDS = (J.INNER, J.LEFT_OUTER, J.RIGHT_OUTER, J.FULL_OUTER)
# the host code in front of the probe kernels (probe_impl, radix_prepare):
FORCING_KINDS = (J.LEFT_OUTER, J.SINGLE, J.MARK, J.FULL_OUTER)  # emit a row per probe row (FULL_OUTER through LEFT_OUTER): a pending filter is applied first, by a scan
UNCLUSTERED_KINDS = (J.SEMI, J.ANTI, J.MARK)  # promise probe order: never radix-clustered


def live(ctx):
    gc.collect()
    return ctx.mem_stats()["live_blocks"]


class World:
    """device tables, host tables and reference answers, each made once"""

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle, self.lib = ctx, oracle, capi.gpu_lib()
        self.dev, self.host, self.parts, self.keep = {}, {}, {}, []

    def table(self, table, form="plain"):
        key = (id(table), form)
        if key not in self.dev:
            self.lib.ldb_gpu_set_option(b"dict_encode", 0)  # only what a case asks for gets a dictionary (1, like debug_check's 0 below, is the default)
            try:
                t = self.ctx.register("je_%d" % len(self.dev), table)
            finally:
                self.lib.ldb_gpu_set_option(b"dict_encode", 1)
            for c, f in enumerate(table.schema):
                if pa.types.is_string(f.type):
                    if form == "dict":
                        assert t.dict_encode(c) > 0 and t.dict_size(c) > 0
                    else:
                        assert t.dict_size(c) == -1
            self.dev[key] = t
            self.keep.append(table)
        return self.dev[key]

    def host_rel(self, rel):
        sides = []
        for t, r in rel.sides:
            if id(t) not in self.host:
                self.host[id(t)] = HostTable(t)
                self.keep.append(t)
            sides.append((self.host[id(t)], r))
        return HostRel(sides, rel.n)

    def partners(self, c, B, P, resid):
        key = (id(c.build), repr(c.build_via), id(c.probe), repr(c.via[1:]) if c.via and c.via[0] != "joined" else repr(c.via and (id(c.via[1]), c.via[2])), repr(c.bkeys), repr(c.pkeys), repr(resid))
        if key not in self.parts:
            self.parts[key] = J.partners(B, c.bkeys, P, c.pkeys, resid)
        return self.parts[key]

    def close(self):
        for t in self.dev.values():
            t.release()
        self.dev.clear()


@pytest.fixture(scope="module")
def world(ctx, oracle):
    lib = capi.gpu_lib()
    start = live(ctx)
    lib.ldb_gpu_set_option(b"debug_check", 1)
    w = World(ctx, oracle)
    try:
        yield w
    finally:
        lib.ldb_gpu_set_option(b"debug_check", 0)
        w.close()
    assert live(ctx) == start, "the module leaves device blocks behind"


def preds_of(preds):
    return [api.pred(col, op, const) for col, op, const in preds]


def sides_of(rel):
    return [rel.rowids(s) for s in range(rel.sides)]


def sorted_rows(cols, n):
    m = np.stack([np.asarray(c, dtype=np.int64) for c in cols], axis=1) if n else np.zeros((0, len(cols)), np.int64)
    return m[np.lexsort(m.T[::-1])]


def same_rows(got, want, n, ordered):
    if ordered:
        return all(np.array_equal(g, w) for g, w in zip(got, want))
    return np.array_equal(sorted_rows(got, n), sorted_rows(want, n))


def check(kind, out, mark, B, P, want, ordered, tag):
    """the device's result `out` (+ `mark`) of `kind` against `want` in logical rows (join_ref.from_partners)"""
    n_p, n_b = len(P.sides), len(B.sides)
    got = sides_of(out)
    if kind in PAIR_KINDS:
        p, b = want[0], want[1]
        tail = want[2] if kind in (J.RIGHT_OUTER, J.FULL_OUTER) else np.zeros(0, np.uint32)
        assert out.rows == len(p) + len(tail) and len(got) == n_p + n_b, tag
        exp = P.expand(p) + B.expand(b)
        assert same_rows([g[: len(p)] for g in got], exp, len(p), ordered), tag
        if kind in (J.RIGHT_OUTER, J.FULL_OUTER):  # then the unmatched build rows, ascending, their probe sides padded
            for g in got[:n_p]:
                assert (g[len(p) :] == J.NULL_ROW).all(), tag
            assert all(np.array_equal(g[len(p) :], w) for g, w in zip(got[n_p:], B.expand(tail))), tag
    elif kind == J.SINGLE:  # one row per probe row, in probe order, with an admissible partner or none
        assert out.rows == P.n and len(got) == n_p + n_b, tag
        if not ordered and P.n:  # (the radix-clustered probe gives its rows cluster after cluster: put them back into probe order)
            perm = np.lexsort([g.astype(np.int64) for g in got[:n_p]][::-1])
            got = [g[perm] for g in got]
        assert all(np.array_equal(g, w) for g, w in zip(got[:n_p], P.expand(np.arange(P.n)))), tag
        phys = [B.phys(s) for s in range(n_b)]
        for i, rows in enumerate(want):
            mine = tuple(int(g[i]) for g in got[n_p:])
            if rows is None:  # (the oracle's answer: it says only whether there is a partner)
                continue
            if not rows:
                assert all(v == J.NULL_ROW for v in mine), (tag, i)
            else:
                assert mine in {tuple(int(ph[r]) for ph in phys) for r in rows}, (tag, i, mine)
    elif kind in (J.SEMI, J.ANTI):
        assert out.rows == len(want) and len(got) == n_p, tag
        assert all(np.array_equal(g, w) for g, w in zip(got, P.expand(want))), tag
    elif kind == J.MARK:
        assert out.rows == P.n and len(got) == n_p, tag
        assert all(np.array_equal(g, w) for g, w in zip(got, P.expand(np.arange(P.n)))), tag
        flags = mark.read_fixed(0).view(np.uint8)[: P.n] if P.n else np.zeros(0, np.uint8)
        assert np.array_equal(flags, want), tag
    else:  # SEMI_BUILD, ANTI_BUILD, semi_anti_build: ascending build rows
        assert out.rows == len(want) and len(got) == n_b, tag
        assert all(np.array_equal(g, w) for g, w in zip(got, B.expand(want))), tag


def device_rels(world, c):
    """the case's build and probe relations on the device → (build rel, probe rel, handles to release)"""
    hold = []
    bt = world.table(c.build, c.build_form)
    brel = bt.rel()
    hold.append(brel)
    if c.build_via:
        brel = brel.scan_filter(preds_of(c.build_via[1]))
        hold.append(brel)
    prel = world.table(c.probe, c.probe_form).rel()
    hold.append(prel)
    if c.via and c.via[0] == "lazy":
        pass  # (the case sets lazy_min_rows = 0: probe_once filters this dense relation anew for every probe)
    elif c.via and c.via[0] == "rowid":
        prel = prel.scan_filter(preds_of(c.via[1]))
        hold.append(prel)
    elif c.via:
        drel = world.table(c.via[1]).rel()
        dht = drel.join_build([(0, 0)], unique=True)
        prel = dht.probe(prel, [(0, c.via[2])], capi.JOIN_LEFT_OUTER)
        hold += [drel, dht, prel]
    return brel, prel, hold


def launches(prof, prefix):
    return sum(n for name, (n, _) in prof.items() if name.startswith(prefix))


def probe_once(ctx, ht, prel, c, kind, resid, anti_preds=None, wrong=None):
    """one probe → (result, mark table | None, the relation to release after them | None, clustered).  A lazy case filters the dense `prel`
    here, so that every kind and every residual meets a pending filter.  For the lazy and the radix cases the launches under the profile
    are compared with what the path admits; a difference goes into `wrong` (asserted empty at the end of the case, so that one run names all)."""
    lazy = bool(c.via) and c.via[0] == "lazy"
    radix = c.options.get("join_radix", (0, 0))[0] == 1
    own = prel.scan_filter(preds_of(c.via[1])) if lazy else None
    p = own if lazy else prel
    try:
        if lazy or radix:
            ctx.prof_reset()
            ctx.prof_enable(True)
        try:
            if anti_preds is None:
                r = ht.probe(p, c.pkeys, kind, residual=resid)
            else:
                r = ht.probe_semi_anti_build(p, c.pkeys, preds_of(anti_preds), residual=resid)
        finally:
            if lazy or radix:
                ctx.prof_enable(False)
    except BaseException:
        if own is not None:
            own.release()
        raise
    out, mark = r if kind == J.MARK and anti_preds is None else (r, None)
    clustered = False
    if lazy or radix:
        prof = ctx.prof_all()
        tag = (c.name, "semi_anti_build" if anti_preds is not None else J.KIND_NAMES[kind], resid)
        scans, hists = launches(prof, "k_scan_bitmap"), launches(prof, "k_radix_hist")
        clustered = hists > 0
        if lazy and (scans > 0) != (kind in FORCING_KINDS or anti_preds is not None):
            wrong.append(tag + ("%d scan launches before the probe" % scans,))
        if radix and clustered != (anti_preds is None and kind not in UNCLUSTERED_KINDS):
            wrong.append(tag + ("%d k_radix_hist launches" % hists,))
    return out, mark, own, clustered


@pytest.mark.parametrize("name", list(CASES))
def test_join_case(world, ctx, oracle, name):
    c = CASES[name]
    lib = world.lib
    B, P = c.build_rel(), c.probe_rel()
    ordered_kinds = (J.LEFT_OUTER, J.SINGLE) if c.unique and "promise" not in c.name else (J.SINGLE,)  # (unless clustered: cluster after cluster)
    hold, wrong = [], []
    for k, (val, _) in c.options.items():
        lib.ldb_gpu_set_option(k.encode(), val)
    try:
        brel, prel, hold = device_rels(world, c)
        if c.via and c.via[0] == "joined":  # a unique LEFT_OUTER join: one row per probe row, in order
            assert all(np.array_equal(g, w) for g, w in zip(sides_of(prel), P.expand(np.arange(P.n))))
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            ht = brel.join_build(c.bkeys, unique=c.unique)
        finally:
            ctx.prof_enable(False)
        hold.append(ht)
        if c.evidence is not None:  # the cheap evidence of the layout the case claims
            got = {"slots": ht.slots, "bytes": ht.table_bytes, "builds": ctx.prof_all().get("k_join_build", (0, 0))[0]}
            print(f"{name}: {c.layout}: {got}")
            assert got == c.evidence, c.layout
        hb, hp = world.host_rel(B), world.host_rel(P)
        for resid in [[]] + c.residuals:
            part = world.partners(c, B, P, resid)
            for kind in c.kinds:
                tag = (J.KIND_NAMES[kind], resid)
                out, mark, own, clustered = probe_once(ctx, ht, prel, c, kind, resid, wrong=wrong)
                try:
                    check(kind, out, mark, B, P, J.from_partners(part, B.n, kind), kind in ordered_kinds and not clustered, tag)
                    if not resid and kind in J.ORACLE_KINDS:
                        op, ob, mk = oracle.join(hb, c.bkeys, hp, c.pkeys, kind)
                        want = {J.INNER: (op, ob), J.LEFT_OUTER: (op, ob), J.MARK: mk, J.SINGLE: [None if b != J.NULL_ROW else [] for b in ob.tolist()]}.get(kind, op)
                        check(kind, out, mark, B, P, want, kind == J.SINGLE and not clustered, ("oracle",) + tag)
                finally:
                    out.release()
                    if mark is not None:
                        mark.release()
                    if own is not None:
                        own.release()
        for ap in c.anti_preds:
            for resid in [[]] + c.residuals[1:2]:
                out, _, own, _ = probe_once(ctx, ht, prel, c, J.SEMI_BUILD, resid, anti_preds=ap, wrong=wrong)
                try:
                    check(J.SEMI_ANTI_BUILD, out, None, B, P, J.from_partners(world.partners(c, B, P, resid), B.n, J.SEMI_ANTI_BUILD, P.filter(ap).tolist()), True, ("semi_anti_build", ap, resid))
                finally:
                    out.release()
                    if own is not None:
                        own.release()
        assert not wrong, wrong
    finally:
        for k, (_, restore) in c.options.items():
            lib.ldb_gpu_set_option(k.encode(), restore)
        for h in reversed(hold):
            h.release()


@pytest.mark.parametrize("name", list(NL))
def test_nested_loop_join(world, name):
    b, p, resid = NL[name]
    B, P = J.Rel([(b, None)]), J.Rel([(p, None)])
    part = J.partners(B, [], P, [], resid)
    brel, prel = world.table(b).rel(), world.table(p).rel()
    try:
        for kind in J.NL_KINDS:
            r = prel.join_nl(brel, resid, kind)
            out, mark = r if kind == J.MARK else (r, None)
            try:
                check(kind, out, mark, B, P, J.from_partners(part, B.n, kind), kind == J.SINGLE, (J.KIND_NAMES[kind], resid))
            finally:
                out.release()
                if mark is not None:
                    mark.release()
    finally:
        brel.release(), prel.release()


def test_three_conjuncts_are_refused(world, ctx):
    c = CASES["rank_sorted"]
    brel, prel = world.table(c.build).rel(), world.table(c.probe).rel()
    ht = brel.join_build(c.bkeys, unique=True)
    calls = [lambda: ht.probe(prel, c.pkeys, capi.JOIN_INNER, residual=J.THREE_CONJUNCTS), lambda: ht.probe(prel, c.pkeys, capi.JOIN_ANTI, residual=J.THREE_CONJUNCTS),
             lambda: ht.probe_semi_anti_build(prel, c.pkeys, preds_of(J.ANTI_PREDS[0]), residual=J.THREE_CONJUNCTS), lambda: prel.join_nl(brel, J.THREE_CONJUNCTS, capi.JOIN_INNER)]
    try:
        for call in calls:
            before = live(ctx)
            with pytest.raises(capi.LdbError) as e:
                call()
            assert e.value.status == capi.LDB_ERR_UNSUPPORTED, e.value
            del e
            assert live(ctx) == before
    finally:
        ht.release(), brel.release(), prel.release()
