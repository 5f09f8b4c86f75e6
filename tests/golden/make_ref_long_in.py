"""Generates tests/golden/ref_long_in.json by running the REFERENCE'S OWN Restrictions (oracle/_ref/libldb_ref.so, ref_scan_filter — as
make_ref_golden.py does) over a seeded table of 3 000 rows with string IN lists of 10 and 300 constants: the hash set of
Restrictions.cpp:481-515, which the string-set scan kernel (csrc/ldb_strset.hip) replaces.  The fixture is data only — the rows, the integer
column, the lists and the passing row ids — and is what tests/test_gpu_strset.py::test_reference_restrictions_fixture compares against on the
GPU box, where neither the reference tree nor oracle/_ref is read.

Run from the repo root where oracle/_ref has been built:  python tests/golden/make_ref_long_in.py"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "lingo-db_amd"), os.path.join(ROOT, "tests"), ROOT]

import test_oracle_vs_ref as tv  # noqa: E402  (binding helpers of the reference library)

N_ROWS = 3000


def title(rng):
    """movie-title-like strings: a shared article, one to four words, sometimes a year — many share their first eight bytes"""
    words = ["The", "A", "Night", "Day", "of", "the", "Living", "Dead", "Return", "Star", "Wars", "Love", "Story", "II", "Überfall", "Café", "東京"]
    k = int(rng.integers(1, 5))
    s = " ".join(words[int(j)] for j in rng.integers(0, len(words), k))
    if rng.integers(0, 3) == 0:
        s += " (%d)" % int(rng.integers(1950, 2020))
    return s


def main():
    lib = C.CDLL(tv.REF_LIB)
    lib.ref_scan_filter.restype = C.c_int64
    lib.ref_scan_filter.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(tv.RefFilter), C.c_int32, C.c_void_p, C.c_int32]
    rng = np.random.default_rng(20261018)
    distinct = sorted({title(rng) for _ in range(1500)})
    rows = [None if i % 17 == 5 else distinct[int(j)] for i, j in enumerate(rng.integers(0, len(distinct), N_ROWS))]
    k = rng.integers(0, 100, N_ROWS).astype(np.int32)
    table = pa.table({"s": pa.array(rows, pa.string()), "k": pa.array(k)})
    ten = [distinct[int(j)] for j in rng.choice(len(distinct), 8, replace=False)] + ["no such title", "The"]
    many = [distinct[int(j)] for j in rng.choice(len(distinct), 280, replace=False)] + ["missing %d" % i for i in range(18)] + [ten[0], ten[0]]
    assert len(ten) == 10 and len(many) == 300
    cases = [{"values": ten}, {"values": many, "k_lt": 60}]
    for c in cases:
        filters = [{"col": "s", "op": "IN", "in": c["values"]}] + ([{"col": "k", "op": "LT", "v": c["k_lt"]}] if "k_lt" in c else [])
        c["passing"] = [int(r) for r in tv.run_ref_filter(lib, table, filters)]
        member = set(c["values"])
        assert c["passing"] == [i for i, v in enumerate(rows) if v in member and ("k_lt" not in c or k[i] < c["k_lt"])], "the reference disagrees with Python's set membership"
        assert len(c["passing"]) > 0
    with open(os.path.join(HERE, "ref_long_in.json"), "w") as f:
        json.dump({"rows": rows, "k": k.tolist(), "cases": cases}, f, ensure_ascii=True)
    print("ref_long_in.json:", [len(c["passing"]) for c in cases], "passing rows")


if __name__ == "__main__":
    main()
