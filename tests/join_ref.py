"""Plain-Python statement of the library's joins — TEST INFRASTRUCTURE, a second opinion beside oracle/ldb_oracle.c (whose ora_join
knows neither residual conjuncts nor the right / full outer kinds nor the nested-loop form).

The rule, written over Python values with nothing clever in it:
  * key columns become Python values through order_ref.column_values: ints, dates (days) and decimals (unscaled) are ints, strings are bytes;
    a float key is its bit pattern (db.hash hashes the bits and the compare is ==: +0.0 and -0.0 are two keys), a NaN matches nothing,
  * a NULL key part never matches; a residual (probe_col, op, build_col) holds only when both operands are non-NULL and the comparison holds,
  * a dict from key tuple to the build rows in ascending order, the probe rows walked in order.
With an empty key list every build row is a candidate: the reference of ldb_gpu_join_nl.

`cases()` is the one source of inputs for tests/test_join_edges.py (oracle and a two-loop brute force against this file, no device) and
tests/test_gpu_join_edges.py (device against this file and the oracle).  Seeds are fixed; nothing here reads a clock or the environment."""
import operator
import os
import re

import numpy as np
import pyarrow as pa

import order_ref

NULL_ROW = 0xFFFFFFFF
INNER, SEMI, ANTI, LEFT_OUTER, MARK, SINGLE, SEMI_BUILD, ANTI_BUILD, RIGHT_OUTER, FULL_OUTER = range(10)  # = LDB_JOIN_*
SEMI_ANTI_BUILD = 10  # ldb_gpu_join_probe_semi_anti_build (no value of ldb_join_kind)
KIND_NAMES = ("INNER", "SEMI", "ANTI", "LEFT_OUTER", "MARK", "SINGLE", "SEMI_BUILD", "ANTI_BUILD", "RIGHT_OUTER", "FULL_OUTER", "SEMI_ANTI_BUILD")
ALL_KINDS = tuple(range(10))
NL_KINDS = (INNER, LEFT_OUTER, SEMI, ANTI, MARK, SINGLE, SEMI_BUILD, ANTI_BUILD)
ORACLE_KINDS = (INNER, SEMI, ANTI, LEFT_OUTER, MARK, SINGLE, SEMI_BUILD, ANTI_BUILD)
EQ, NEQ, LT, LTE, GT, GTE = range(6)  # = LDB_F_EQ .. LDB_F_GTE
OPS = (operator.eq, operator.ne, operator.lt, operator.le, operator.gt, operator.ge)
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
TILE = 2048  # rows per tile of the fused-filter probe kernels; their LDS queue is drained 1024 entries at a time


# ------------------------------------------------------------------ arrow → Python values
def values(col):
    """one column as Python values, None for NULL (and for a float NaN: as a key it matches nothing)"""
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if isinstance(arr, pa.ChunkedArray):
        arr = pa.concat_arrays(arr.chunks) if arr.num_chunks else pa.array([], type=arr.type)
    valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
    dense_arr = arr.drop_null()
    if pa.types.is_floating(arr.type):
        a = dense_arr.to_numpy(zero_copy_only=False)
        bits = a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
        dense = [None if x != x else int(b) for x, b in zip(a.tolist(), bits.tolist())]
    else:
        dense = order_ref.column_values(dense_arr)
    it = iter(dense)
    return [next(it) if v else None for v in valid]


class Rel:
    """a host relation: sides = [(pyarrow table, row ids | None)]; a row id of NULL_ROW is an outer join's padding (every column NULL)"""

    def __init__(self, sides, n=None):
        self.sides = [(t, None if r is None else np.asarray(r, dtype=np.uint32)) for t, r in sides]
        t, r = self.sides[0]
        self.n = int(n if n is not None else (t.num_rows if r is None else len(r)))
        self._cols = {}

    def phys(self, side):
        r = self.sides[side][1]
        return np.arange(self.n, dtype=np.uint32) if r is None else r

    def col(self, ref):
        """the values of column ref = (side, col) per logical row"""
        if ref not in self._cols:
            t, r = self.sides[ref[0]]
            base = _table_values(t, ref[1])
            self._cols[ref] = base if r is None else [None if p == NULL_ROW else base[p] for p in r.tolist()]
        return self._cols[ref]

    def select(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        return Rel([(t, self.phys(s)[rows]) for s, (t, _) in enumerate(self.sides)], len(rows))

    def filter(self, preds):
        """the logical rows on which every (column ref, op, constant) holds; NULL fails"""
        cols = [(self.col(c), OPS[op], const) for c, op, const in preds]
        return np.array([i for i in range(self.n) if all(v[i] is not None and f(v[i], const) for v, f, const in cols)], dtype=np.int64)

    def expand(self, rows):
        """physical row ids per side for logical rows `rows` (NULL_ROW stays NULL_ROW): what the device reports"""
        rows = np.asarray(rows, dtype=np.int64)
        pad = rows == NULL_ROW
        out = []
        for s in range(len(self.sides)):
            got = np.full(len(rows), NULL_ROW, dtype=np.uint32)
            got[~pad] = self.phys(s)[rows[~pad]]
            out.append(got)
        return out


_TABLE_VALUES = {}


def _table_values(table, c):
    key = (id(table), c)
    if key not in _TABLE_VALUES:
        _TABLE_VALUES[key] = (table, values(table.column(c)))  # (the table is kept: id() stays unique)
    return _TABLE_VALUES[key][1]


# ------------------------------------------------------------------ the join
def partners(build, bkeys, probe, pkeys, residual=()):
    """per probe row the ascending list of build rows it joins with"""
    assert len(bkeys) == len(pkeys)
    bk, pk = [build.col(k) for k in bkeys], [probe.col(k) for k in pkeys]
    index = {}
    for r in range(build.n):
        key = tuple(c[r] for c in bk)
        if None not in key:
            index.setdefault(key, []).append(r)
    every = list(range(build.n))
    res = [(probe.col(pc), OPS[op], build.col(bc)) for pc, op, bc in residual]
    out = []
    for i in range(probe.n):
        if bkeys:
            key = tuple(c[i] for c in pk)
            cand = [] if None in key else index.get(key, [])
        else:
            cand = every
        for pv, f, bv in res:
            x = pv[i]
            cand = [] if x is None else [r for r in cand if bv[r] is not None and f(x, bv[r])]
        out.append(cand)
    return out


def _u32(v):
    return np.array(v, dtype=np.uint32).reshape(-1)


def from_partners(part, n_build, kind, anti_rows=None):
    """the result of `kind` in LOGICAL rows of the two relations:
    INNER / LEFT_OUTER → (probe rows, build rows | NULL_ROW), probe order, partners ascending;  SINGLE → the partner lists themselves (one output row
    per probe row; which member is returned the ABI leaves open);  SEMI / ANTI → ascending probe rows;  MARK → one flag per probe row;
    SEMI_BUILD / ANTI_BUILD → ascending build rows;  RIGHT_OUTER / FULL_OUTER → (probe rows, build rows, ascending unmatched build rows);
    SEMI_ANTI_BUILD → ascending build rows with a partner and none among the probe rows `anti_rows`"""
    if kind == SINGLE:
        return part
    if kind in (INNER, LEFT_OUTER, RIGHT_OUTER, FULL_OUTER):
        pad = kind in (LEFT_OUTER, FULL_OUTER)
        p, b = [], []
        for i, rows in enumerate(part):
            for r in rows:
                p.append(i), b.append(r)
            if pad and not rows:
                p.append(i), b.append(NULL_ROW)
        if kind in (INNER, LEFT_OUTER):
            return _u32(p), _u32(b)
        hit = {r for rows in part for r in rows}
        return _u32(p), _u32(b), _u32([r for r in range(n_build) if r not in hit])
    if kind == SEMI:
        return _u32([i for i, rows in enumerate(part) if rows])
    if kind == ANTI:
        return _u32([i for i, rows in enumerate(part) if not rows])
    if kind == MARK:
        return np.array([1 if rows else 0 for rows in part], dtype=np.uint8)
    hit = {r for rows in part for r in rows}
    if kind == SEMI_BUILD:
        return _u32([r for r in range(n_build) if r in hit])
    if kind == ANTI_BUILD:
        return _u32([r for r in range(n_build) if r not in hit])
    assert kind == SEMI_ANTI_BUILD
    barred = {r for i in anti_rows for r in part[i]}
    return _u32([r for r in range(n_build) if r in hit and r not in barred])


def join(build, bkeys, probe, pkeys, kind, residual=(), anti_preds=None):
    """what include/lingodb_gpu.h promises for the ten kinds, and with anti_preds = [(probe column ref, op, constant)] for the one-pass
    semi_anti_build form (kind is then ignored); see from_partners for the shape of the answer"""
    part = partners(build, bkeys, probe, pkeys, residual)
    if anti_preds is not None:
        return from_partners(part, build.n, SEMI_ANTI_BUILD, probe.filter(anti_preds).tolist())
    return from_partners(part, build.n, kind)


def brute(build, bkeys, probe, pkeys, residual=()):
    """partners() by two loops over all pairs and no dict"""
    out = []
    for i in range(probe.n):
        rows = []
        for r in range(build.n):
            ok = True
            for bk, pk in zip(bkeys, pkeys):
                x, y = probe.col(pk)[i], build.col(bk)[r]
                ok = ok and x is not None and y is not None and x == y
            for pc, op, bc in residual:
                x, y = probe.col(pc)[i], build.col(bc)[r]
                ok = ok and x is not None and y is not None and OPS[op](x, y)
            if ok:
                rows.append(r)
        out.append(rows)
    return out


# ------------------------------------------------------------------ two keys with one tag
# Distinct keys whose db.hash values agree in the upper 32 bits, the tag a hashed slot stores: only the key comparison tells them apart.
# Found once by find_tag_collision (below) over a seeded range; tests/test_join_edges.py asserts that they still collide.
COLLIDING_INT64 = (-1778341770789363651, -115872959296815129)
COLLIDING_UTF8 = (b"collide-0029868", b"collide-0044780")


def collision_candidates(kind, n=1 << 17):
    if kind == "int64":
        rng = np.random.default_rng(20261020)
        return pa.array(np.unique(rng.integers(-(2 ** 62), 2 ** 62, n)), pa.int64())
    return order_ref.str_array([b"collide-%07d" % i for i in range(n)])


def find_tag_collision(oracle, kind, n=1 << 17):
    """the first two candidates (in candidate order) whose hashes share the upper 32 bits"""
    from oracle_bind import HostTable

    col = collision_candidates(kind, n)
    h = oracle.hash_keys(HostTable(pa.table({"k": col})).rel(), [(0, 0)]) >> np.uint64(32)
    order = np.argsort(h, kind="stable")
    same = np.nonzero(h[order][1:] == h[order][:-1])[0]
    assert len(same), "no pair among %d candidates" % n
    vals = values(col)
    a, b = sorted((int(order[same[0]]), int(order[same[0] + 1])))
    return vals[a], vals[b]


# ------------------------------------------------------------------ inputs
class Case:
    """one build table, one probe table and how to join them.
    bkeys / pkeys: column refs (side, col);  unique: the promise given to join_build (it holds unless `layout` says otherwise);
    options: {option: (value for the case, value to restore)};  layout: the build layout the case claims to reach, evidence: the
    slots / table bytes / k_join_build launches that layout shows through the ABI (None: not claimed);
    via: how the probe relation is made — None (the plain table), ("rowid", preds) a materialised selection, ("lazy", preds) a filter fused
    into the probe, ("joined", dim table, fk column) the unique LEFT_OUTER join of the probe table with `dim` on dim column 0: two sides;
    build_via: None or ("rowid", preds);  residuals: the residual lists to run besides the empty one;  forms: registration of utf8 columns."""

    def __init__(self, name, build, bkeys, probe, pkeys, unique=False, options=None, layout="", evidence=None, via=None, build_via=None, residuals=(), kinds=ALL_KINDS,
                 build_form="plain", probe_form="plain", anti_preds=(), oracle_ok=True):
        self.name, self.build, self.bkeys, self.probe, self.pkeys, self.unique = name, build, list(bkeys), probe, list(pkeys), unique
        self.options, self.layout, self.evidence, self.via, self.build_via = dict(options or {}), layout, evidence, via, build_via
        self.residuals, self.kinds, self.build_form, self.probe_form, self.anti_preds, self.oracle_ok = list(residuals), tuple(kinds), build_form, probe_form, list(anti_preds), oracle_ok

    def build_rel(self):
        r = Rel([(self.build, None)])
        return r.select(r.filter(self.build_via[1])) if self.build_via else r

    def probe_rel(self):
        r = Rel([(self.probe, None)])
        if self.via is None:
            return r
        if self.via[0] in ("rowid", "lazy"):
            return r.select(r.filter(self.via[1]))
        dim, fk = self.via[1], self.via[2]
        p, b = join(Rel([(dim, None)]), [(0, 0)], r, [(0, fk)], LEFT_OUTER)
        assert np.array_equal(p, np.arange(r.n, dtype=np.uint32))  # dim's key is unique
        return Rel([(self.probe, None), (dim, b)], r.n)


LAZY = {"lazy_min_rows": (0, 1 << 20)}
RADIX = {"join_radix": (1, -1), "join_radix_part_bytes": (4096, 1 << 20)}
NO_RANK = {"join_rank": (0, 1)}


def _long_run():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lingo-db_amd", "csrc", "ldb_join_kernel.h")) as f:
        return int(re.search(r"#define\s+JOIN_LONG_RUN\s+(\d+)", f.read()).group(1))


def _pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _cap(n):
    return max(64, _pow2(2 * n))


def ev_rank(range0):
    return {"slots": range0, "bytes": 8 * (range0 // 32 + 1), "builds": 1}


def ev_direct(range0, builds=1):
    return {"slots": range0, "bytes": 4 * range0, "builds": builds}


def ev_slots(n, builds=1, pair32=False):
    return {"slots": _cap(n), "bytes": (16 if pair32 else 8) * _cap(n), "builds": builds if n else 0}


def _nulls(vals, every, first):
    """a Python list with None at rows first, first + every, …"""
    out = list(vals)
    for i in range(first, len(out), every):
        out[i] = None
    return out


def _payload(rng, n, probe):
    """the columns behind the key: 1 v int32 (a few values, some NULL), 2 w int64, 3 d date32, 4 m decimal(12,2) (some NULL), 5 f int32 (probe: the tile filter)"""
    v = _nulls([int(x) for x in rng.integers(0, 6, n)], 11, 5 if probe else 3)
    w = [int(x) for x in rng.integers(0, 6, n)]
    d = [int(x) for x in rng.integers(-3, 3, n)]
    m = _nulls([int(x) for x in rng.integers(-2, 3, n)], 13, 0 if probe else 7)
    cols = {"v": pa.array(v, pa.int32()), "w": pa.array(w, pa.int64()), "d": pa.array(d, pa.int32()).cast(pa.date32()),
            "m": pa.array([None if x is None else order_ref.decimal.Decimal(x).scaleb(-2) for x in m], pa.decimal128(12, 2))}
    if probe:
        cols["f"] = pa.array(tile_filter_column(n), pa.int32())
    return cols


def tile_filter_column(n):
    """f per probe row, tile after tile of TILE rows: tile 0 all 0; tile 1 all 1; tile 2 exactly 1024 ones (every second row); tile 3 exactly
    1025 ones; tile 4 … all 0; the last tile (partial unless n is a multiple of TILE) all 2.  `f >= 1` fills the queue of a tile not at all,
    fully, for one round and for two (the second holds one entry); `f == 2` selects rows of the last tile only.  The cases
    use n = 4 * TILE + 1: five tiles, the last of one row."""
    f = np.zeros(n, dtype=np.int32)
    tiles = (n + TILE - 1) // TILE
    if tiles > 1:
        f[TILE : 2 * TILE] = 1
    if tiles > 2:
        f[2 * TILE : min(n, 3 * TILE) : 2] = 1
    if tiles > 3:
        f[3 * TILE : min(n, 4 * TILE) : 2] = 1
        if n > 3 * TILE + 1:
            f[3 * TILE + 1] = 1
    f[(tiles - 1) * TILE :] = 2
    return f


F_GE1 = [((0, 5), GTE, 1)]
F_LAST = [((0, 5), EQ, 2)]
F_NONE = [((0, 5), EQ, 7)]
F_KEY = [((0, 0), GTE, 5)]  # on the key column itself: drops a few rows wherever they are


def _tab(key_arrays, rng, probe, names=None):
    n = len(key_arrays[0])
    cols = {(names[i] if names else "k%d" % i): a for i, a in enumerate(key_arrays)}
    pay = _payload(rng, n, probe)
    first = next(iter(cols))
    return pa.table({first: cols.pop(first), **pay, **cols})  # further key parts sit behind the payload: column 5 (build) / 6 (probe)


def _i(a, ty=pa.int32()):
    return pa.array(a, ty) if isinstance(a, list) else pa.array(np.asarray(a), ty)


def _probe_keys(rng, bk, n, lo=None, hi=None):
    """n probe keys for integer build keys bk: the ends of the build range and their outer neighbours first, then hits and misses mixed"""
    bk = np.asarray([k for k in bk if k is not None], dtype=np.int64)
    kmin, kmax = (int(bk.min()), int(bk.max())) if len(bk) else (0, 0)
    lo = kmin - 1 if lo is None else lo
    hi = kmax + 1 if hi is None else hi
    edge = [kmin - 1, kmin, kmax, kmax + 1, kmin, kmax]
    body = np.where(rng.random(n) < 0.6, rng.choice(bk, n) if len(bk) else 0, rng.integers(lo, hi, n, endpoint=True))
    out = np.concatenate([np.array(edge, dtype=np.int64), body])[:n]
    return np.clip(out, lo, hi)


RESID_SET = [
    [((0, 1), EQ, (0, 1))], [((0, 1), NEQ, (0, 1))], [((0, 1), LT, (0, 2))], [((0, 2), LTE, (0, 1))], [((0, 3), GT, (0, 3))], [((0, 4), GTE, (0, 4))],
    [((0, 1), LTE, (0, 2)), ((0, 4), NEQ, (0, 4))], [((0, 2), GTE, (0, 2)), ((0, 3), LT, (0, 3))],
]  # every operator; int32 v int64 both ways, date v date, decimal v decimal; NULL operands on either side (v, m); one and two conjuncts
THREE_CONJUNCTS = [((0, 1), EQ, (0, 1)), ((0, 2), EQ, (0, 2)), ((0, 3), EQ, (0, 3))]
ANTI_PREDS = [[((0, 2), LT, 3)], [((0, 2), LT, 4), ((0, 1), GTE, 1)]]
_CASES = None


def _build_cases():
    rng = np.random.default_rng(20261020)
    out = []
    NP = 4 * TILE + 1  # five tiles of the fused-filter probe: none / all / 1024 / 1025 selected, and a last tile of one row

    def add(name, bkeys, pkeys, **kw):
        """bkeys / pkeys: one pyarrow key column each (or lists of them: a composite key)"""
        bl, pl = (bkeys if isinstance(bkeys, list) else [bkeys]), (pkeys if isinstance(pkeys, list) else [pkeys])
        b, p = _tab(bl, rng, False), _tab(pl, rng, True)
        bk = [(0, 0)] + [(0, 4 + i) for i in range(1, len(bl))]
        pk = [(0, 0)] + [(0, 5 + i) for i in range(1, len(pl))]
        out.append(Case(name, b, bk, p, pk, **kw))
        return out[-1]

    def variants(base, **kw):
        """the same tables under other options / probe paths: one reference answer serves them all"""
        c = Case(kw.pop("name"), base.build, base.bkeys, base.probe, base.pkeys, **{**dict(unique=base.unique, build_form=base.build_form, probe_form=base.probe_form), **kw})
        out.append(c)
        return c

    def radix_paths(base, name, layout, evidence, options, residuals=()):
        """the radix-clustered probe, from a plain table and from row ids.  The library clusters only a single 4-byte key without NULLs
        probing a rank, direct unique or ordered-slot table (radix_prepare), so only those layouts get these variants"""
        kw = dict(layout=layout, evidence=evidence, options={**options, **RADIX})
        variants(base, name=name + "/radix", residuals=residuals, **kw)
        variants(base, name=name + "/radix_rowid", via=("rowid", F_GE1), **kw)

    def paths(base, layout, evidence, radix=False):
        """the probe paths over one layout: row ids, lazy filters and, where the layout admits it, the radix-clustered probe"""
        kw = dict(layout=layout, evidence=evidence, options=base.options)
        variants(base, name=base.name + "/rowid", via=("rowid", F_GE1), **kw)
        for tag, f in (("ge1", F_GE1), ("last", F_LAST), ("none", F_NONE)):
            variants(base, name=base.name + "/lazy_" + tag, via=("lazy", f), **{**kw, "options": {**base.options, **LAZY}})
        variants(base, name=base.name + "/lazy_resid", via=("lazy", F_GE1), residuals=RESID_SET[:2] + RESID_SET[6:7], **{**kw, "options": {**base.options, **LAZY}})
        if radix:
            radix_paths(base, base.name, layout, evidence, base.options, RESID_SET[1:3] + RESID_SET[6:7])

    # ---------------------------------------------------------------- layouts: 1000 keys 0..999 and what the options make of them
    asc = np.arange(1000)
    shuf = rng.permutation(1000)
    dup = asc.copy()
    dup[999] = 0
    pk1000 = _i(_probe_keys(rng, asc, NP, -50, 1100))
    c = add("rank_sorted", _i(asc), pk1000, unique=True, layout="rank", evidence=ev_rank(1000), residuals=RESID_SET, anti_preds=ANTI_PREDS)
    paths(c, "rank", ev_rank(1000), radix=True)
    variants(c, name="direct_unique", options=NO_RANK, layout="direct", evidence=ev_direct(1000))
    radix_paths(c, "direct_unique", "direct", ev_direct(1000), NO_RANK, RESID_SET[1:3] + RESID_SET[6:7])
    variants(c, name="ordered_unique", options={"join_direct": (0, 1)}, layout="ordered", evidence=ev_slots(1000))
    radix_paths(c, "ordered_unique", "ordered", ev_slots(1000), {"join_direct": (0, 1)}, RESID_SET[1:3] + RESID_SET[6:7])
    variants(c, name="hashed_unique", options={"join_ordered": (0, 1)}, layout="hashed", evidence=ev_slots(1000))
    variants(c, name="chained_forced_unique", options={"join_chained": (1, 0), "join_direct": (0, 1)}, layout="chained", evidence=ev_slots(1000))
    c = add("rank_shuffled", _i(shuf), pk1000, unique=True, layout="rank", evidence=ev_rank(1000), residuals=RESID_SET[:3])
    variants(c, name="rank_shuffled/radix", options=RADIX, layout="rank", evidence=ev_rank(1000), residuals=RESID_SET[2:3])
    c = add("rank_promise_broken", _i(dup), pk1000, unique=True, layout="direct chained (the promise does not hold)", evidence=ev_direct(999, builds=2))
    variants(c, name="direct_promise_broken", options=NO_RANK, layout="direct chained", evidence=ev_direct(999, builds=2))
    # direct, chained: 2000 rows over 300 key values, chains of 1 … ~15, the first partner of many keys fails a residual a later one passes
    bk = np.concatenate([[0, 299], rng.integers(0, 300, 1998)])
    c = add("direct_chained", _i(bk), _i(_probe_keys(rng, bk, NP, -20, 330)), layout="direct chained", evidence=ev_direct(300), residuals=RESID_SET, anti_preds=ANTI_PREDS)
    paths(c, "direct chained", ev_direct(300))
    # ordered slots: 1000 keys spread over 2^30 values
    sp = np.unique(np.concatenate([[0, (1 << 30) - 1], rng.integers(1, (1 << 30) - 1, 1200)]))[:1000]
    sp[-1] = (1 << 30) - 1
    sp = rng.permutation(sp)
    c = add("ordered", _i(sp), _i(_probe_keys(rng, sp, NP)), layout="ordered", evidence=ev_slots(1000))
    variants(c, name="forced_chained", options={"join_chained": (1, 0)}, layout="chained", evidence=ev_slots(1000))
    variants(c, name="hashed", options={"join_ordered": (0, 1)}, layout="hashed", evidence=ev_slots(1000))
    cluster = _long_run() + 88
    outlier = 1 << 30
    bk = np.concatenate([np.arange(cluster), [outlier]])
    add("ordered_to_hashed", _i(bk), _i(np.concatenate([_probe_keys(rng, np.arange(cluster), 2049, -5, cluster + 5), [outlier, outlier - 1, outlier + 1]])),
        layout="hashed after an ordered attempt", evidence=ev_slots(cluster + 1, builds=2))
    bk = np.concatenate([np.full(cluster, 7), [outlier]])
    add("hashed_to_chained", _i(bk), _i(np.concatenate([rng.integers(5, 10, 61), [outlier, 7, 7]])), layout="chained after ordered and hashed attempts",
        evidence=ev_slots(cluster + 1, builds=3), residuals=RESID_SET[:2])  # chains of 600
    add("all_rows_one_key", _i(np.full(64, -5)), _i(rng.integers(-7, -3, 65)), layout="direct chained", evidence=ev_direct(1), residuals=RESID_SET[2:3])  # chain of 64
    add("chains_of_two", _i(np.repeat(np.arange(500), 2)), _i(_probe_keys(rng, np.arange(500), 2047, -3, 503)), layout="direct chained", evidence=ev_direct(500))
    add("empty_build", _i(np.zeros(0, np.int64)), pk1000.slice(0, 65), layout="empty", evidence=ev_slots(0), residuals=RESID_SET[:1])
    add("empty_build_unique", _i(np.zeros(0, np.int64)), pk1000.slice(0, 65), unique=True, layout="empty", evidence=ev_slots(0))
    # int64 key: the slot holds a hash tag
    k64 = rng.permutation(1000).astype(np.int64) * 3 * (1 << 33) - (1 << 40)
    c = add("int64_key", _i(k64, pa.int64()), _i(np.where(rng.random(NP) < 0.5, rng.choice(k64, NP), rng.choice(k64, NP) + rng.choice([1, -1, 1 << 32, -(1 << 32)], NP)), pa.int64()),
            layout="hashed, tag", evidence=ev_slots(1000), residuals=RESID_SET[:3])
    variants(c, name="int64_key_chained", options={"join_chained": (1, 0)}, layout="chained, tag", evidence=ev_slots(1000))
    # two int32 keys: pair32 on and off (the probe's columns 4-byte and not)
    a, b = rng.integers(-3, 40, 1000), rng.integers(I32_MAX - 30, I32_MAX, 1000, endpoint=True)
    pa_, pb_ = rng.integers(-4, 41, NP), rng.integers(I32_MAX - 31, I32_MAX, NP, endpoint=True)
    c = add("pair32", [_i(a), _i(b)], [_i(pa_), _i(pb_)], layout="hashed, pair32", evidence=ev_slots(1000, pair32=True), residuals=RESID_SET, anti_preds=ANTI_PREDS)
    paths(c, "hashed, pair32", ev_slots(1000, pair32=True))
    variants(c, name="pair32_off", options={"join_pair32": (0, 1)}, layout="hashed", evidence=ev_slots(1000))
    add("pair32_wide_probe", [_i(a), _i(b)], [_i(np.where(rng.random(NP) < 0.2, pa_ + (1 << 32), pa_), pa.int64()), _i(pb_)], layout="hashed, pair32", evidence=ev_slots(1000, pair32=True))
    add("pair32_date_int", [_i(a).cast(pa.date32()), _i(b)], [_i(pa_).cast(pa.date32()), _i(pb_)], layout="hashed, pair32", evidence=ev_slots(1000, pair32=True))
    # strings, plain and dictionary-encoded
    words = [b"", b"a", b"a\0", b"ab", b"\xff", "日本".encode(), b"twelve bytes", b"thirteen byte", b"x" * 200] + [b"w%03d" % i for i in range(200)]
    bs = [words[i] for i in rng.integers(0, len(words) - 20, 700)]
    ps = _nulls([words[i] for i in rng.integers(0, len(words), NP)], 97, 0)
    c = add("utf8_key", order_ref.str_array(_nulls(bs, 101, 100)), order_ref.str_array(ps), layout="hashed, tag", evidence=ev_slots(700), residuals=RESID_SET[:3], anti_preds=ANTI_PREDS[:1])
    paths(c, "hashed, tag", ev_slots(700))
    variants(c, name="utf8_dict_build_plain_probe", build_form="dict", layout="hashed, tag", evidence=ev_slots(700))
    variants(c, name="utf8_plain_build_dict_probe", probe_form="dict", layout="hashed, tag", evidence=ev_slots(700))
    variants(c, name="utf8_dict_both", build_form="dict", probe_form="dict", layout="", evidence=None)
    add("utf8_int_key", [order_ref.str_array(bs), _i(rng.integers(0, 3, 700))], [order_ref.str_array(ps), _i(rng.integers(0, 3, NP))], layout="hashed, tag", evidence=ev_slots(700),
        residuals=RESID_SET[1:2])

    # ---------------------------------------------------------------- key edges
    ends = np.concatenate([[I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1, 0, -1], rng.integers(I32_MIN, I32_MAX, 500)])
    pe = np.concatenate([[I32_MAX, I32_MIN, I32_MAX - 1, I32_MIN + 1, 0, -1, 1], rng.choice(ends, 1000), rng.integers(I32_MIN, I32_MAX, 1042)])
    c = add("int32_ends", _i(ends), _i(pe), layout="ordered, slot32, range 2^32", evidence=ev_slots(506))
    variants(c, name="int32_ends_hashed", options={"join_ordered": (0, 1)}, layout="hashed", evidence=ev_slots(506))
    add("int32_ends_wide_probe", _i(ends), _i(np.concatenate([pe, ends[:300] + (1 << 32), ends[:300] - (1 << 32), [1 << 32, -(1 << 32) - 1, (1 << 31), -(1 << 31) - 1]]), pa.int64()),
        layout="ordered, slot32, range 2^32", evidence=ev_slots(506))
    # kmin = INT32_MIN and a probe key of INT32_MAX: key - kmin wraps in 32 bits
    low = np.concatenate([[I32_MIN, I32_MIN + 998], I32_MIN + rng.permutation(997)[:900] + 1])
    plow = np.concatenate([[I32_MAX, I32_MAX - 1, I32_MIN, I32_MIN + 998, I32_MIN + 999, 0, -1], I32_MIN + rng.integers(0, 1100, 500)])
    c = add("kmin_int32_min_unique", _i(low), _i(plow), unique=True, layout="rank", evidence=ev_rank(999))
    variants(c, name="kmin_int32_min_direct", options=NO_RANK, layout="direct", evidence=ev_direct(999))
    variants(c, name="kmin_int32_min_radix", options=RADIX, layout="rank", evidence=ev_rank(999))
    high = np.concatenate([[I32_MAX, I32_MAX - 998], I32_MAX - rng.integers(0, 999, 900)])
    add("kmax_int32_max_chained", _i(high), _i(np.concatenate([[I32_MIN, I32_MIN + 1, I32_MAX, I32_MAX - 998, I32_MAX - 999, 0], I32_MAX - rng.integers(0, 1100, 500)])),
        layout="direct chained", evidence=ev_direct(999))
    # thresholds of the key range: direct max(1024, 8 n) with n = 1000 rows that repeat; key bits from a range of 4096; rank up to 2^26 for promised keys.
    # The key-bits cases sit on a direct chained table, and the ABI shows nothing of the key bits (slots, bytes and builds are the same with and
    # without them): these three check results around the threshold, not where the threshold lies.  The rank threshold is taken at its second
    # arm, 2^26: for promised-unique keys max(4096, 64 n) lies below it whenever n is small, so the first arm cannot be reached on its own.
    for r0 in (7999, 8000, 8001, 4095, 4096, 4097):
        bk = np.concatenate([[10, 10 + r0 - 1], 10 + rng.integers(0, r0, 998)])
        direct = r0 <= 8000
        add("range_%d" % r0, _i(bk), _i(_probe_keys(rng, bk, 2049)), layout="direct chained" if direct else "ordered", evidence=ev_direct(r0) if direct else ev_slots(1000))
    for r0 in ((1 << 26) - 1, 1 << 26, (1 << 26) + 1):
        bk = np.unique(np.concatenate([[-7, -7 + r0 - 1], -7 + rng.integers(0, r0, 1000)]))
        rank = r0 <= 1 << 26
        add("unique_range_2p26%+d" % (r0 - (1 << 26)), _i(bk), _i(_probe_keys(rng, bk, 2049)), unique=True, layout="rank" if rank else "ordered", evidence=ev_rank(r0) if rank else ev_slots(len(bk)))
    # narrow and date key columns, either side
    k8 = rng.permutation(np.arange(-128, 128))[:200]
    k16 = rng.integers(-(2 ** 15), 2 ** 15, 900)
    add("int8_key", _i(k8, pa.int8()), _i(rng.integers(-128, 128, 2049), pa.int8()), unique=True, layout="rank", evidence=None)
    add("int8_build_int32_probe", _i(k8, pa.int8()), _i(rng.integers(-200, 200, 2049)), layout="direct chained", evidence=None)
    add("int32_build_int8_probe", _i(rng.integers(-200, 200, 300)), _i(rng.integers(-128, 128, 2049), pa.int8()), layout="direct chained", evidence=None)
    add("int16_key", _i(k16, pa.int16()), _i(rng.integers(-(2 ** 15), 2 ** 15, 2049), pa.int16()), layout="ordered", evidence=None)
    add("int16_build_int64_probe", _i(k16, pa.int16()), _i(np.where(rng.random(2049) < 0.5, rng.choice(k16, 2049), rng.choice(k16, 2049) + (1 << 32)), pa.int64()), layout="ordered", evidence=None)
    add("int64_build_int16_probe", _i(np.concatenate([k16[:500], k16[:300].astype(np.int64) + (1 << 32)]), pa.int64()), _i(rng.choice(k16, 2049), pa.int16()), layout="hashed, tag", evidence=ev_slots(800))
    add("int64_build_int32_probe", _i(np.concatenate([ends[:300], ends[:300].astype(np.int64) + (1 << 32)]), pa.int64()), _i(rng.choice(ends, 2049)), layout="hashed, tag", evidence=ev_slots(600))
    dk = rng.integers(-800, 800, 1000)
    add("date32_key", _i(dk).cast(pa.date32()), _i(_probe_keys(rng, dk, 2049)).cast(pa.date32()), layout="direct chained", evidence=ev_direct(int(dk.max() - dk.min()) + 1))
    # NULL keys: the first and the last row, across a 64-row word, with row-id inputs
    nb = [int(x) for x in rng.permutation(700)]
    for i in (0, 62, 63, 64, 65, 127, 128, 699):
        nb[i] = None
    npk = [int(x) for x in _probe_keys(rng, np.arange(700), NP, -5, 705)]
    for i in list(range(60, 70)) + [0, NP - 1, 2047, 2048]:
        npk[i] = None
    c = add("null_keys_unique", _i(nb), _i(npk), unique=True, layout="rank", evidence=None, residuals=RESID_SET[:1])
    variants(c, name="null_keys_unique/rowid", via=("rowid", F_GE1), layout="rank")
    variants(c, name="null_keys_unique/lazy", via=("lazy", F_GE1), options=LAZY, layout="rank")
    variants(c, name="null_keys_rowid_build", build_via=("rowid", [((0, 2), GTE, 2)]), unique=True, layout="")
    variants(c, name="null_keys_hashed", options={"join_ordered": (0, 1)}, layout="hashed")
    nb2 = nb + nb[100:300]
    add("null_keys_chained", _i(nb2), _i(npk), layout="direct chained", evidence=None)
    add("all_keys_null", _i([None] * 130), _i(npk[:200]), layout="", evidence=None)
    # decimal keys: 64-bit (precision 18) and 128-bit (precision 19) hashing
    d18 = [int(x) for x in rng.integers(-(10 ** 17), 10 ** 17, 300)] + [10 ** 18 - 1, -(10 ** 18) + 1, 0, -1, 1]
    d19 = d18 + [10 ** 19 - 1, -(10 ** 19) + 1, 2 ** 63, -(2 ** 63) - 1, 2 ** 63 + 2 ** 32]
    for prec, pool in ((18, d18), (19, d19)):
        bd = [pool[i] for i in rng.integers(0, len(pool), 600)]
        pd_ = [pool[i] + int(o) for i, o in zip(rng.integers(0, len(pool), 2049), rng.choice([0, 0, 1, 2 ** 32], 2049))]
        pd_ = [v if abs(v) < 10 ** prec else 0 for v in pd_]
        add("decimal%d_key" % prec, order_ref.dec_array(bd, prec, 0), order_ref.dec_array(pd_, prec, 0), layout="hashed, tag", evidence=ev_slots(600), residuals=RESID_SET[5:6])
    # float keys: +0.0 and -0.0 are two keys, NaN matches nothing (not even its own bit pattern)
    for ty in (np.float32, np.float64):
        pool = np.array([0.0, -0.0, np.nan, -np.nan, 1.5, -1.5, np.inf, -np.inf, 5e-324 if ty == np.float64 else 1e-45, 1e10, 0.1] + [float(x) for x in rng.normal(0, 3, 40)], dtype=ty)
        bf = np.concatenate([pool[:11], pool[rng.integers(0, len(pool), 300)]])
        pf = np.concatenate([pool[:11], pool[rng.integers(0, len(pool), 1500)], rng.normal(0, 3, 538).astype(ty)])
        c = add("%s_key" % np.dtype(ty).name, pa.array(bf), pa.array(pf), layout="hashed, tag", evidence=ev_slots(311))
        variants(c, name="%s_key_chained" % np.dtype(ty).name, options={"join_chained": (1, 0)}, layout="chained, tag", evidence=ev_slots(311))
    # two distinct keys under one 32-bit tag
    if COLLIDING_INT64:
        x, y = COLLIDING_INT64
        fill = [int(v) for v in rng.integers(-(2 ** 40), 2 ** 40, 60)]
        c = add("tag_collision_int64", _i([x] + fill, pa.int64()), _i([y, x, y, x] + fill[:20] + [x + 1, y - 1], pa.int64()), layout="hashed, tag", evidence=ev_slots(61))
        variants(c, name="tag_collision_int64_unique", unique=True, layout="hashed, tag", evidence=ev_slots(61))
        add("tag_collision_int64_both", _i([x, y, x] + fill, pa.int64()), _i([y, x, y, x] + fill[:20], pa.int64()), layout="hashed, tag", evidence=ev_slots(63))
    if COLLIDING_UTF8:
        x, y = COLLIDING_UTF8
        fill = [b"fill-%d" % i for i in range(60)]
        add("tag_collision_utf8", order_ref.str_array([x] + fill), order_ref.str_array([y, x, y, x] + fill[:20]), layout="hashed, tag", evidence=ev_slots(61))
        add("tag_collision_utf8_both", order_ref.str_array([y, x, y] + fill), order_ref.str_array([y, x, y, x] + fill[:20]), layout="hashed, tag", evidence=ev_slots(63))
    # a build table registered in several batches
    parts = [pa.table({n_: col.slice(s, ln) for n_, col in zip(out[0].build.schema.names, out[0].build.columns)}) for s, ln in ((0, 1), (1, 63), (64, 64), (128, 872))]
    out.append(Case("build_in_batches", pa.concat_tables(parts), [(0, 0)], out[0].probe, [(0, 0)], unique=True, layout="rank", evidence=ev_rank(1000)))
    assert out[-1].build.column(0).num_chunks == 4

    # ---------------------------------------------------------------- sizes
    u = _i(rng.permutation(3000))
    for n in (0, 1, 63, 64, 65, 2047, 2048, 2049):
        pk = _i(_probe_keys(rng, np.arange(3000), max(n, 6), -30, 3030)[:n])
        add("probe_rows_%d" % n, u, pk, unique=True, layout="rank", evidence=ev_rank(3000))
        add("probe_rows_%d_chained" % n, _i(np.concatenate([[0, 299], rng.integers(0, 300, 900)])), _i(_probe_keys(rng, np.arange(300), max(n, 6), -3, 303)[:n]), layout="direct chained", evidence=ev_direct(300))
    # pairs across the 64-row chunks of the pair count: runs of hits and misses whose chains end on either side of a chunk end
    bk = np.repeat(np.arange(40), rng.integers(1, 9, 40))
    pk = np.concatenate([np.repeat([1, 50, 2, 51, 3], [62, 3, 63, 1, 64]), rng.integers(0, 45, 200), np.full(64, 7), np.full(64, 60), np.full(65, 8)])
    add("pairs_across_chunks", _i(bk), _i(pk), layout="direct chained", evidence=None, residuals=RESID_SET[1:2])
    # every probe row finds its partner (probe_unique keeps the probe's sides as they are), and the same with one miss
    hit_all = rng.integers(0, 3000, 2049)
    one_miss = hit_all.copy()
    one_miss[1500] = 3000
    dim = pa.table({"id": _i(rng.permutation(5000)), "x": _i(rng.integers(0, 9, 5000))})
    for tag, pk in (("all_match", hit_all), ("one_miss", one_miss)):
        fk = rng.integers(0, 5000, len(pk))
        fk[7] = 5000 if tag == "one_miss" else fk[7]
        p = _tab([_i(pk)], rng, True).append_column("fk", _i(fk))
        b = _tab([u], rng, False)
        for lay, opts, ev in (("rank", {}, ev_rank(3000)), ("direct", NO_RANK, ev_direct(3000)), ("hashed", {"join_ordered": (0, 1)}, ev_slots(3000))):
            out.append(Case("%s_%s" % (tag, lay), b, [(0, 0)], p, [(0, 0)], unique=True, options=opts, layout=lay, evidence=ev))
            out.append(Case("%s_%s/rowid" % (tag, lay), b, [(0, 0)], p, [(0, 0)], unique=True, options=opts, layout=lay, evidence=ev, via=("rowid", F_KEY)))
            out.append(Case("%s_%s/joined" % (tag, lay), b, [(0, 0)], p, [(0, 0)], unique=True, options=opts, layout=lay, evidence=ev, via=("joined", dim, 6),
                            residuals=[[((1, 1), LTE, (0, 2))], [((0, 2), NEQ, (0, 2))]]))
    # a unique table whose only key partner fails the residual
    b = _tab([_i(np.arange(100))], rng, False)
    p = _tab([_i(np.arange(-2, 103))], rng, True)
    out.append(Case("only_partner_fails", b, [(0, 0)], p, [(0, 0)], unique=True, layout="rank", evidence=ev_rank(100), residuals=[[((0, 0), NEQ, (0, 0))], [((0, 0), GT, (0, 0)), ((0, 1), EQ, (0, 1))]]))
    return out


def cases():
    """the named cases, the same objects on every call; tables are shared between cases and must not be changed"""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return iter(_CASES)


def nl_cases():
    """(name, build relation table, probe relation table, residual) for ldb_gpu_join_nl: small sides, zero to two conjuncts"""
    rng = np.random.default_rng(20261021)
    b, p = _tab([_i(rng.integers(0, 5, 37))], rng, False), _tab([_i(rng.integers(0, 6, 131))], rng, True)
    b0 = b.slice(0, 0)
    sets = [("cross", []), ("eq_key", [((0, 0), EQ, (0, 0))])] + [("r%d" % i, r) for i, r in enumerate(RESID_SET)]
    out = [("nl_" + tag, b, p, r) for tag, r in sets]
    out += [("nl_empty_build", b0, p, []), ("nl_empty_build_r", b0, p, RESID_SET[0]), ("nl_empty_probe", b, p.slice(0, 0), RESID_SET[1]), ("nl_one_row", b.slice(3, 1), p.slice(5, 1), [])]
    return out
