"""Generates tests/golden/ref_strfn.json by calling the REFERENCE'S OWN string runtime — StringRuntime::toUpper, toLower,
concat, len, fromInt and substr, as compiled unmodified into oracle/_ref/libldb_ref.so — on a seeded pool of strings and
integers.  A few lines of glue of our own (below) are compiled against the reference's headers into oracle/_ref/ at
generation time; nothing of it is committed.  The fixture is data only: the inputs and the recorded outputs, bytes as hex.
tests/test_strfn_api.py pins the Python restatement (tests/strfn_eval.py) to it, tests/test_gpu_strfn.py the device kernels.

Run from the repo root where oracle/_ref has been built:  python tests/golden/make_ref_strfn.py"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("LDB_REFERENCE_DIR", "/root/reference")

GLUE = r"""
#include "lingodb/runtime/StringRuntime.h"
#include "lingodb/runtime/helpers.h"
#include <cstdint>
#include <cstring>
using namespace lingodb;
static runtime::VarLen32 in(const char* s, int64_t n) { return runtime::VarLen32::fromDataAndLen(s, (size_t) n, runtime::StorageClass::TRANSIENT); }
static int64_t give(runtime::VarLen32 r, char* out, int64_t cap) {
   const int64_t n = (int64_t) r.getLen();
   if (n <= cap) memcpy(out, r.data(), (size_t) n);
   return n;
}
extern "C" {
int64_t glue_upper(const char* s, int64_t n, char* out, int64_t cap) { return give(runtime::StringRuntime::toUpper(in(s, n)), out, cap); }
int64_t glue_lower(const char* s, int64_t n, char* out, int64_t cap) { return give(runtime::StringRuntime::toLower(in(s, n)), out, cap); }
int64_t glue_concat(const char* a, int64_t na, const char* b, int64_t nb, char* out, int64_t cap) { return give(runtime::StringRuntime::concat(in(a, na), in(b, nb)), out, cap); }
int64_t glue_len(const char* s, int64_t n) { return runtime::StringRuntime::len(in(s, n)); }
int64_t glue_from_int(int64_t v, char* out, int64_t cap) { return give(runtime::StringRuntime::fromInt(v), out, cap); }
int64_t glue_substr(const char* s, int64_t n, int64_t from, int64_t len, char* out, int64_t cap) { return give(runtime::StringRuntime::substr(in(s, n), from, len), out, cap); }
}
"""


def build_glue():
    src = os.path.join(REF_DIR, "strfn_glue.cpp")
    so = os.path.join(REF_DIR, "libstrfn_glue.so")
    with open(src, "w") as f:
        f.write(GLUE)
    ref = os.path.join(REF_DIR, "libldb_ref.so")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-w", "-DENABLE_REFCOUNT=1", "-I" + os.path.join(ROOT, "oracle", "ref_build", "shim"),
                           "-I" + os.path.join(REFERENCE, "include"), "-I" + os.path.join(REFERENCE, "vendored"), "-I" + pa.get_include(), src, "-o", so, ref,
                           "-Wl,-rpath," + REF_DIR, "-Wl,-rpath," + pa.get_library_dirs()[0]])
    return C.CDLL(so)


def pool(rng):
    """a few hundred strings: ASCII of every kind, 2- / 3- / 4-byte UTF-8, every length around the VarLen32 short / long boundary"""
    fixed = ["", "a", "Z", "abc", "ABC", "MiXeD CaSe 123", "hello, world!", "@[`{ ~^_|", "0123456789", "ß", "É", "éÉ", "straße STRASSE", "ÀÁÂÃÄÅÆÇÈÉÊËÌÍÎÏ", "àáâãäåæçèéêëìíîï",
             "ÿþýüûúùø÷öõôóòñð", "Ωμέγα ΑΛΦΑ", "Привет МИР", "東京都", "日本語 Text mixed", "€uro ₤ ‰", "😀 emoji 😀", "a😀b𝄞c", "\U0010FFFF\U00010000", "\u0080¿߿ࠀ￿",
             "tab\there", "line\nbreak", "nul\x00inside", "x" * 11, "y" * 12, "z" * 13, "é" * 5 + "a", "é" * 6, "é" * 6 + "a", "Ab" * 40, "q" * 100, "Éa" * 30]
    alphabets = ["abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ", "0123456789", " !\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~", "ßÉéüÖñçÅøÆ", "ΑαΩωЖжЯя", "東京日本語한국", "😀𝄞🚀"]
    out = list(fixed)
    for k in range(200):
        n = int(rng.integers(0, 32)) if k % 9 else int(rng.choice([11, 12, 13]))
        mix = [alphabets[int(j)] for j in rng.choice(len(alphabets), int(rng.integers(1, 4)), replace=False)]
        chars = "".join(mix)
        out.append("".join(chars[int(j)] for j in rng.integers(0, len(chars), n)))
    # byte lengths 11 / 12 / 13 exactly, with and without multi-byte characters
    for n in (11, 12, 13):
        out.append("Q" * n)
        out.append("é" * ((n - 1) // 2) + "q" * (n - 2 * ((n - 1) // 2)))
    return out


def integers():
    v = [0, 1, -1, 7, -7, 2 ** 31 - 1, -(2 ** 31), 2 ** 31, 2 ** 63 - 1, -(2 ** 63), -(2 ** 63) + 1]
    for k in range(1, 19):
        v += [10 ** k - 1, 10 ** k, -(10 ** k) + 1, -(10 ** k)]
    return v


def main():
    lib = build_glue()
    cp, i64 = C.c_char_p, C.c_int64
    for name, args in (("glue_upper", [cp, i64, cp, i64]), ("glue_lower", [cp, i64, cp, i64]), ("glue_concat", [cp, i64, cp, i64, cp, i64]), ("glue_len", [cp, i64]),
                       ("glue_from_int", [i64, cp, i64]), ("glue_substr", [cp, i64, i64, i64, cp, i64])):
        getattr(lib, name).restype = i64
        getattr(lib, name).argtypes = args
    buf = C.create_string_buffer(1 << 12)

    def took(n):
        assert 0 <= n <= len(buf)
        return buf.raw[:n]

    rng = np.random.default_rng(20261019)
    strings = [s.encode() for s in pool(rng)]
    seen = set().union(*[set(b) for b in strings])
    assert {0x80, 0xBF, 0xC2, 0xC3, 0xDF, 0xE0, 0xEF, 0xF0, 0xF4} <= seen and {len(b) for b in strings} >= {0, 11, 12, 13}
    ints = integers()
    doc = {"strings": [b.hex() for b in strings], "ints": ints}
    doc["upper"] = [took(lib.glue_upper(b, len(b), buf, len(buf))).hex() for b in strings]
    doc["lower"] = [took(lib.glue_lower(b, len(b), buf, len(buf))).hex() for b in strings]
    doc["length"] = [int(lib.glue_len(b, len(b))) for b in strings]
    doc["concat_next"] = [took(lib.glue_concat(a, len(a), b, len(b), buf, len(buf))).hex() for a, b in zip(strings, strings[1:])]
    doc["from_int"] = [took(lib.glue_from_int(v, buf, len(buf))).decode("ascii") for v in ints]
    doc["substr"] = []
    for i in range(0, len(strings), 7):
        for frm, ln in ((1, 3), (2, 2), (0, 2), (-2, 5), (3, 0), (4, -1), (1, 1 << 30), (30, 4), (6, 7)):
            b = strings[i]
            doc["substr"].append({"i": i, "from": frm, "for": ln, "out": took(lib.glue_substr(b, len(b), frm, ln, buf, len(buf))).hex()})
    path = os.path.join(HERE, "ref_strfn.json")
    with open(path, "w") as f:
        json.dump(doc, f, ensure_ascii=True, separators=(",", ":"))
    print("ref_strfn.json: %d strings, %d integers, %d substr cases, %d bytes" % (len(strings), len(ints), len(doc["substr"]), os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
