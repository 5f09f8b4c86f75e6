"""Sort, top-k, partition, window order and the registration dictionary (csrc/ldb_sort.hip and its consumers) at the edges of the key
types and of the three sorting paths — the one-workgroup bitonic sort (<= 4096 rows), the 4-bit LSD radix sort with constant-digit
skipping, the radix select in front of top-k.  Every comparison is bit-exact equality of row-id vectors with the oracle
(oracle/ldb_oracle.c), whose answers for the same inputs tests/test_order_edges.py checks against a plain-Python comparator without a device.
Inputs come from order_ref.cases(); tables are registered once per module."""
import gc

import numpy as np
import pyarrow as pa
import pytest

import order_ref
from lingodb_amd import api, capi
from oracle_bind import HostRel, HostTable

pytestmark = pytest.mark.gpu

CASES = {name: (table, specs) for name, table, specs in order_ref.cases()}
SORT_CASES = [n for n in CASES if not n.startswith("topk_")]
TOPK_CASES = [n for n in CASES if n.startswith("topk_")]
SELECT_CASES = ["topk_a_const_words", "topk_b_shared_lead", "topk_c_4096_candidates", "topk_c_4097_candidates", "topk_d_dec33_desc", "topk_e_prefix40"]
I64_MIN = -(2 ** 63)
NULL_ROW = 0xFFFFFFFF


class World:
    """device tables, host tables and oracle answers, each made once (keyed by the identity of the pyarrow table / the case name)"""

    def __init__(self, ctx, oracle):
        self.ctx, self.oracle = ctx, oracle
        self.dev, self.host, self.want = {}, {}, {}
        self.tables = []

    def register(self, table, form="auto", narrow=False):
        """form 'plain': no dictionaries; 'dict': every utf8 column dictionary-encoded (by registration from 4096 rows, on request below);
        'auto': the library's defaults"""
        key = (id(table), form, narrow)
        if key not in self.dev:
            lib = capi.gpu_lib()
            if form == "plain":
                lib.ldb_gpu_set_option(b"dict_encode", 0)
            try:
                t = self.ctx.register("oe_%d" % len(self.dev), table, narrow_decimals=narrow)
            finally:
                lib.ldb_gpu_set_option(b"dict_encode", 1)
            for c, f in enumerate(table.schema):
                if pa.types.is_string(f.type):
                    if form == "dict":
                        if table.num_rows < 4096:
                            assert t.dict_encode(c) > 0
                        assert t.dict_size(c) > 0
                    elif form == "plain":
                        assert t.dict_size(c) == -1
            self.dev[key] = t
            self.tables.append(table)  # (keeps id() unique)
        return self.dev[key]

    def hrel(self, table):
        if id(table) not in self.host:
            self.host[id(table)] = HostTable(table)
        return self.host[id(table)].rel()

    def order(self, name):
        if name not in self.want:
            table, specs = CASES[name]
            self.want[name] = self.oracle.sort(self.hrel(table), order_ref.sort_specs(specs))
        return self.want[name]

    def close(self):
        for t in self.dev.values():
            t.release()


@pytest.fixture(scope="module")
def world(ctx, oracle):
    w = World(ctx, oracle)
    yield w
    w.close()


def forms_of(name):
    """the registrations a case is run under: strings plain and dictionary-encoded, decimal(12,2) also narrowed to 64 bits"""
    if name.startswith(("utf8", "topk_e")):
        return [("plain", False), ("dict", False)]
    if name.startswith("dec12_2"):
        return [("auto", False), ("auto", True)]
    return [("auto", False)]


def live(ctx):
    gc.collect()  # (handles dropped without release() go now, not in the middle of a measurement)
    return ctx.mem_stats()["live_blocks"]


def refused(ctx, call, status):
    """`call` must fail with `status` and leave as many live device blocks as it found"""
    before = live(ctx)
    with pytest.raises(capi.LdbError) as e:
        call()
    assert e.value.status == status, e.value
    del e
    assert live(ctx) == before


# ---------------------------------------------------------------- key types x row counts x directions, digit skipping, eight keys
@pytest.mark.parametrize("name", SORT_CASES)
def test_sort_matches_oracle(world, name):
    table, specs = CASES[name]
    want = world.order(name)
    for form, narrow in forms_of(name):
        rel = world.register(table, form, narrow).rel()
        out = rel.sort(order_ref.sort_specs(specs))
        assert np.array_equal(out.rowids(0), want), (form, narrow)
        for k in order_ref.topk_ks(name):
            top = rel.topk(order_ref.sort_specs(specs), k)
            assert np.array_equal(top.rowids(0), want[:k]), (form, narrow, k)
            top.release()
        out.release(), rel.release()


@pytest.mark.parametrize("n", [4097, 20000])
def test_all_keys_equal_is_the_identity(world, n):
    table, specs = CASES["all_equal_%d" % n]
    out = world.register(table).rel().sort(order_ref.sort_specs(specs))
    assert np.array_equal(out.rowids(0), np.arange(n, dtype=np.uint32))  # every digit is constant: no pass runs, nothing moves


def test_nine_keys_are_refused(world, ctx):
    table, specs = CASES["eight_keys_4097"]
    rel = world.register(table).rel()
    nine = order_ref.sort_specs(specs + [(8, False)])
    refused(ctx, lambda: rel.sort(nine), capi.LDB_ERR_UNSUPPORTED)
    refused(ctx, lambda: rel.topk(nine, 5), capi.LDB_ERR_UNSUPPORTED)
    refused(ctx, lambda: rel.sort([]), capi.LDB_ERR_UNSUPPORTED)


# ---------------------------------------------------------------- top-k: the radix select
@pytest.mark.parametrize("name", TOPK_CASES)
def test_topk_matches_sorted_prefix(world, name):
    table, specs = CASES[name]
    want = world.order(name)
    for form, narrow in forms_of(name):
        rel = world.register(table, form, narrow).rel()
        for k in order_ref.topk_ks(name):
            top = rel.topk(order_ref.sort_specs(specs), k)
            assert top.rows == min(k, table.num_rows)
            assert np.array_equal(top.rowids(0), want[:k]), (form, k)
            top.release()
        rel.release()


@pytest.mark.parametrize("name", SELECT_CASES)
def test_topk_short_select_changes_nothing(world, name):
    """option topk_short_select: 1 (default) stops the select passes once the candidates fit one workgroup, 0 runs all of them"""
    table, specs = CASES[name]
    want = world.order(name)
    lib = capi.gpu_lib()
    rel = world.register(table, forms_of(name)[0][0]).rel()
    got = {}
    try:
        for short in (0, 1):
            lib.ldb_gpu_set_option(b"topk_short_select", short)
            got[short] = [rel.topk(order_ref.sort_specs(specs), k).rowids(0) for k in order_ref.topk_ks(name)]
    finally:
        lib.ldb_gpu_set_option(b"topk_short_select", 1)
    for k, g0, g1 in zip(order_ref.topk_ks(name), got[0], got[1]):
        assert np.array_equal(g0, g1) and np.array_equal(g0, want[:k]), k
    rel.release()


# ---------------------------------------------------------------- relations that are not the identity
def test_sort_and_topk_of_a_filtered_relation(world, ctx, oracle):
    table, specs = CASES["int64_8193_desc"]
    plist = [api.pred((0, 1), capi.F_GTE, 0)]  # tie >= 0: about three rows in five, > 4096 of them
    rel, hrel = world.register(table).rel(), world.hrel(table)
    idx = oracle.scan_filter(hrel, plist)
    assert 4096 < len(idx) < table.num_rows
    want = idx[oracle.sort(hrel.select(idx), order_ref.sort_specs(specs))]
    frel = rel.scan_filter(plist)
    assert np.array_equal(frel.sort(order_ref.sort_specs(specs)).rowids(0), want)
    for k in (0, 1, 10, 4096, len(idx) - 1, len(idx), len(idx) + 1):
        assert np.array_equal(frel.topk(order_ref.sort_specs(specs), k).rowids(0), want[:k]), k
    few = rel.scan_filter([api.pred((0, 1), capi.F_EQ, 2)])  # <= 4096 rows: the one-workgroup sort over row ids
    idx2 = oracle.scan_filter(hrel, [api.pred((0, 1), capi.F_EQ, 2)])
    assert 1 < len(idx2) <= 4096
    assert np.array_equal(few.sort(order_ref.sort_specs(specs)).rowids(0), idx2[oracle.sort(hrel.select(idx2), order_ref.sort_specs(specs))])


@pytest.fixture(scope="module")
def joined(world, ctx):
    """5000 probe rows against 600 build rows with duplicate keys; some probe keys find no partner"""
    rng = np.random.default_rng(77)
    probe = pa.table({"k": pa.array(rng.integers(0, 500, 5000), pa.int32()), "x": pa.array(rng.choice([0.0, -0.0, 1.5, -1.5], 5000))})
    build = pa.table({"k": pa.array(rng.integers(0, 400, 600), pa.int32()), "d": order_ref.dec_array([int(v) * 2 ** 64 for v in rng.integers(-3, 4, 600)], 38, 0)})
    gp, gb = world.register(probe), world.register(build)
    return probe, build, gp, gb


def test_sort_of_a_join_result_by_keys_of_both_sides(world, ctx, oracle, joined):
    probe, build, gp, gb = joined
    out = gb.rel().join_build([(0, 0)]).probe(gp.rel(), [(0, 0)], capi.JOIN_INNER)
    p, b = out.rowids(0), out.rowids(1)  # side 0 = probe rows, side 1 = build rows; the pairs as the device wrote them are the input order
    assert len(p) > 4096
    specs = [api.sort_spec((1, 1), True), api.sort_spec((0, 1))]
    perm = oracle.sort(HostRel([(HostTable(probe), p), (HostTable(build), b)], len(p)), specs)
    s = out.sort(specs)
    assert np.array_equal(s.rowids(0), p[perm]) and np.array_equal(s.rowids(1), b[perm])
    t = out.topk(specs, 100)
    assert np.array_equal(t.rowids(0), p[perm][:100]) and np.array_equal(t.rowids(1), b[perm][:100])


def test_sort_after_left_outer_join(world, ctx, oracle, joined):
    probe, build, gp, gb = joined
    out = gb.rel().join_build([(0, 0)]).probe(gp.rel(), [(0, 0)], capi.JOIN_LEFT_OUTER)
    p, b = out.rowids(0), out.rowids(1)
    assert (b == NULL_ROW).any() and len(p) > 4096
    refused(ctx, lambda: out.sort([api.sort_spec((1, 1))]), capi.LDB_ERR_UNSUPPORTED)  # a key of the padded side holds NULLs
    refused(ctx, lambda: out.topk([api.sort_spec((0, 1)), api.sort_spec((1, 0))], 10), capi.LDB_ERR_UNSUPPORTED)
    specs = [api.sort_spec((0, 1), True), api.sort_spec((0, 0))]
    perm = oracle.sort(HostRel([(HostTable(probe), p), (HostTable(build), b)], len(p)), specs)
    s = out.sort(specs)
    assert np.array_equal(s.rowids(0), p[perm]) and np.array_equal(s.rowids(1), b[perm])


def test_nullable_keys(world, ctx, oracle):
    n = 5000
    rng = np.random.default_rng(5)
    vals = rng.integers(-100, 100, n).tolist()
    no_null = pa.table({"v": pa.array(vals, pa.int64()), "id": pa.array(np.arange(n, dtype=np.int32))})
    vals[1234] = None
    one_null = pa.table({"v": pa.array(vals, pa.int64()), "id": pa.array(np.arange(n, dtype=np.int32))})
    # a validity bitmap with every bit set
    arr = no_null.column(0).combine_chunks()
    all_set = pa.Array.from_buffers(pa.int64(), n, [pa.py_buffer(np.full((n + 7) // 8, 0xFF, np.uint8).tobytes()), arr.buffers()[1]], null_count=0)
    nullable = pa.table({"v": all_set, "id": no_null.column(1)})
    specs = [api.sort_spec((0, 0), True)]
    want = oracle.sort(HostTable(no_null).rel(), specs)
    assert np.array_equal(world.register(nullable).rel().sort(specs).rowids(0), want)
    g = world.register(one_null).rel()
    refused(ctx, lambda: g.sort(specs), capi.LDB_ERR_UNSUPPORTED)
    refused(ctx, lambda: g.topk(specs, 3), capi.LDB_ERR_UNSUPPORTED)
    # the same column behind a filter that drops the NULL row: nothing NULL is left among the keys
    keep = g.scan_filter([api.pred((0, 1), capi.F_NEQ, 1234)])
    idx = np.array([i for i in range(n) if i != 1234], dtype=np.uint32)
    assert np.array_equal(keep.sort(specs).rowids(0), idx[oracle.sort(HostTable(no_null).rel().select(idx), specs)])


# ---------------------------------------------------------------- partition
@pytest.fixture(scope="module")
def parts(world):
    n = 20000
    rng = np.random.default_rng(31)
    words = [b"", b"a", b"ab", b"twelve bytes", b"thirteen byte", b"\xff", "日本".encode()] + [b"w%d" % i for i in range(300)]
    full = pa.table({"id": pa.array(np.arange(n, dtype=np.int32)), "k32": pa.array(rng.integers(-(2 ** 31), 2 ** 31, n), pa.int32()),
                     "k64": pa.array(rng.integers(-1000, 1000, n), pa.int64()), "s": order_ref.str_array([words[i] for i in rng.integers(0, len(words), n)])})
    return {20000: full, 4097: full.slice(0, 4097), 1: full.slice(0, 1), 0: full.slice(0, 0)}


def check_partition(world, table, keys, nparts, plist=None):
    rel, hrel = world.register(table).rel(), world.hrel(table)
    idx = np.arange(table.num_rows, dtype=np.uint32)
    if plist:
        idx = world.oracle.scan_filter(hrel, plist)
        rel, hrel = rel.scan_filter(plist), hrel.select(idx)
    ids = order_ref.partition_ids(world.oracle, hrel, keys, nparts)
    packed, counts = rel.partition(keys, nparts, [(0, 0)])
    assert counts == np.bincount(ids, minlength=nparts).tolist()
    assert packed.rows == len(idx)
    got = packed.read_fixed(0).view(np.int32) if len(idx) else np.zeros(0, np.int32)
    assert np.array_equal(got, idx[np.argsort(ids, kind="stable")].astype(np.int32))  # partition after partition, input order inside each
    packed.release()


@pytest.mark.parametrize("nparts", [1, 2, 16, 17, 255, 256])
@pytest.mark.parametrize("n", [20000, 4097])
@pytest.mark.parametrize("keys", [[(0, 1)], [(0, 2), (0, 3)]], ids=["int32", "int64_utf8"])
def test_partition_counts_and_order(world, parts, keys, n, nparts):
    check_partition(world, parts[n], keys, nparts)


@pytest.mark.parametrize("nparts", [2, 17, 256])
def test_partition_of_a_filtered_relation(world, parts, nparts):
    check_partition(world, parts[20000], [(0, 1)], nparts, [api.pred((0, 2), capi.F_LT, 300)])


@pytest.mark.parametrize("n", [0, 1])
def test_partition_of_nothing_and_of_one_row(world, parts, n):
    for nparts in (1, 16, 17, 256):
        check_partition(world, parts[n], [(0, 2), (0, 3)], nparts)


def test_partition_count_limits(world, ctx, parts):
    rel = world.register(parts[4097]).rel()
    for nparts in (0, 257):
        refused(ctx, lambda: rel.partition([(0, 1)], nparts, [(0, 0)]), capi.LDB_ERR_INVALID)


# ---------------------------------------------------------------- the dictionary built at registration
def test_registration_with_a_string_the_sort_cannot_order(ctx, oracle):
    """5000 rows, ten distinct strings, one of 300 bytes: over the 256-byte limit of a string sort key, so the dictionary cannot be ordered.
    Registration succeeds all the same and the column answers predicates like any other."""
    rng = np.random.default_rng(8)
    long = b"L" * 299 + b"!"
    words = [b"alpha", b"beta", b"", b"gamma", b"L" * 256, b"delta", b"\xff", b"L" * 299, b"eps", long]
    vals = [words[i] for i in rng.integers(0, len(words), 5000)]
    table = pa.table({"id": pa.array(np.arange(5000, dtype=np.int32)), "s": order_ref.str_array(vals), "short": order_ref.str_array([v[:3] for v in vals])})
    t = ctx.register("oe_long_dict", table)
    assert t.rows == 5000
    # (column 1 itself stays unencoded on an MI355X today — dict_size(1) == -1: building its dictionary sorts the distinct values, and that sort
    # refuses the 300-byte one.  Encoded would be just as good, so nothing is asserted about it.)
    assert t.dict_size(2) > 0  # its neighbour (every value <= 3 bytes) still gets its dictionary
    hrel = HostTable(table).rel()
    for const in (long, b"beta", b"L" * 299, b"absent"):
        plist = [api.pred((0, 1), capi.F_EQ, const)]
        want = oracle.scan_filter(hrel, plist)
        assert want.tolist() == [i for i, v in enumerate(vals) if v == const]
        assert np.array_equal(t.rel().scan_filter(plist).rowids(0), want), const
    t.release()


# ---------------------------------------------------------------- window order
def test_window_orders_zero_signs_like_the_sort(world, oracle):
    """ORDER BY f, tie with f holding zeros of both signs: the window's row order is the sort's"""
    table, specs = CASES["float64_4097_asc"]
    rel, cols = world.register(table).rel().window([], order_ref.sort_specs(specs), [(capi.WIN_COUNT_STAR, None)], frame=(I64_MIN, 0))
    assert np.array_equal(rel.rowids(0), world.order("float64_4097_asc"))
    assert cols.to_arrow().column(0).to_pylist() == list(range(1, table.num_rows + 1))
