"""The string runtime functions of the reference (src/runtime/StringRuntime.cpp: toUpper, toLower, concat, len, fromInt,
substr) restated on Python `bytes` — what the device kernels of csrc/ldb_strfn.hip are compared against.  The restatement
itself is pinned to the reference's recorded outputs (tests/golden/ref_strfn.json) by tests/test_strfn_api.py."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_strfn.json")
STR_WHOLE = 2 ** 63 - 1


def upper(b):
    """std::toupper byte by byte in the C locale: a-z only, every byte >= 0x80 passes through"""
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in b)


def lower(b):
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in b)


def length(b):
    """UTF-8 characters = bytes that are not continuation bytes (10xxxxxx)"""
    return sum(1 for c in b if (c >> 6) != 2)


def from_int(v):
    return str(int(v)).encode()


def _char_to_byte(b, char_index, known_byte=0, known_char=0):
    while known_byte < len(b):
        if (b[known_byte] >> 6) != 2:
            if known_char == char_index:
                return known_byte
            known_char += 1
        known_byte += 1
    return len(b)


def substr(b, frm, for_len):
    """StringRuntime::substr: character positions from 1; positions before the string count towards the length"""
    leg_len = max(0, for_len)
    leg_from = max(frm, 1)
    leg_to = max(frm + leg_len, leg_from)
    b0 = _char_to_byte(b, leg_from - 1)
    b1 = _char_to_byte(b, leg_to - 1, b0, leg_from - 1)
    return b[b0:b1]


def strcat_row(parts, row):
    """one row of ldb_gpu_map_strcat: parts = bytes (a constant) | {"col": values, "case": …, "from": …, "for": …} |
    {"int": values}; values are per-row lists with None for NULL.  → bytes, or None when a part is NULL"""
    out = b""
    for p in parts:
        if isinstance(p, (bytes, str)):
            out += p.encode() if isinstance(p, str) else p
            continue
        if "int" in p:
            v = p["int"][row]
            if v is None:
                return None
            out += from_int(v)
            continue
        v = p["col"][row]
        if v is None:
            return None
        v = v.encode() if isinstance(v, str) else v
        if p.get("from", 1) != 1 or p.get("for", STR_WHOLE) != STR_WHOLE:
            v = substr(v, p.get("from", 1), p.get("for", STR_WHOLE))
        c = p.get("case")
        out += upper(v) if c == "upper" else lower(v) if c == "lower" else v
    return out


def strcat(parts, n):
    return [strcat_row(parts, i) for i in range(n)]


def load_fixture():
    with open(FIXTURE) as f:
        d = json.load(f)
    for k in ("strings", "upper", "lower", "concat_next"):
        d[k] = [bytes.fromhex(h) for h in d[k]]
    d["from_int"] = [s.encode() for s in d["from_int"]]
    for c in d["substr"]:
        c["out"] = bytes.fromhex(c["out"])
    return d
