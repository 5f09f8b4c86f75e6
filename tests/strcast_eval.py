"""The casts between text and int / decimal / date of the reference's string runtime (src/runtime/StringRuntime.cpp: toInt
:174-185, toDecimal :187-200, toDate :439-444, fromDecimal :217-222, fromDate :452-456) restated on Python `bytes` and
`int` — what the device code of csrc/ldb_strcast.h is compared against.  No pyarrow in here: tests/test_strcast_api.py
pins this restatement to pyarrow (whose Decimal128::FromString / ToString and date parser the reference calls).

A parse returns the value, or None where the string is BAD: the reference throws or leaves its result undefined.  Decimals
are unscaled integers (the value times 10^scale), dates days since 1970-01-01."""

INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
DATE_MIN, DATE_MAX = -719162, 2932896  # 0001-01-01, 9999-12-31
_SPACE = b" \t\n\v\f\r"  # isspace in the C locale
_DIGITS = b"0123456789"


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


# ---------------------------------------------------------------- text → value
def stoll_grammar(s):
    """→ (sign, digits) when s is blanks, an optional sign, at least one digit and nothing else; None otherwise"""
    s = _b(s)
    k = 0
    while k < len(s) and s[k] in _SPACE:
        k += 1
    sign = 1
    if k < len(s) and s[k] in b"+-":
        sign = -1 if s[k] == 0x2D else 1
        k += 1
    digits = s[k:]
    if not digits or any(c not in _DIGITS for c in digits):
        return None
    return sign, digits


def to_int(s):
    """std::stoll that must consume the whole string; a value outside int64 throws"""
    g = stoll_grammar(s)
    if g is None:
        return None
    v = 0
    for c in g[1]:
        v = v * 10 + (c - 0x30)
    v *= g[0]
    return v if INT64_MIN <= v <= INT64_MAX else None


def decimal_parts(s):
    """Decimal128::FromString's grammar → (negative, whole digits, fraction digits, exponent) or None.  The exponent is
    what arrow reads behind e / E: a '+' that is skipped, then an int32 ('-'? digits+)"""
    s = _b(s)
    k = 0
    neg = False
    if k < len(s) and s[k] in b"+-":
        neg = s[k] == 0x2D
        k += 1
    j = k
    while j < len(s) and s[j] in _DIGITS:
        j += 1
    whole, frac = s[k:j], b""
    if j < len(s) and s[j] == 0x2E:
        k = j = j + 1
        while j < len(s) and s[j] in _DIGITS:
            j += 1
        frac = s[k:j]
    if not whole and not frac:
        return None
    exp = 0
    if j < len(s):
        if s[j] not in b"eE":
            return None
        j += 1
        if j < len(s) and s[j] == 0x2B:
            j += 1
        eneg = j < len(s) and s[j] == 0x2D
        if eneg:
            j += 1
        ed = s[j:]
        if not ed or any(c not in _DIGITS for c in ed):
            return None
        exp = int(ed) * (-1 if eneg else 1)
        if not -(2 ** 31) <= exp <= 2 ** 31 - 1:
            return None
    return neg, whole, frac, exp


def to_decimal(s, precision, scale):
    """FromString, Rescale to `scale`, then |v| < 10^precision (stricter than the reference, as arrow's own cast)"""
    p = decimal_parts(s)
    if p is None:
        return None
    neg, whole, frac, exp = p
    digits = (whole + frac).lstrip(b"0")
    if len(digits) > 38:  # more significant digits than a decimal128 has
        return None
    parsed_scale = len(frac) - exp
    if -parsed_scale > 38:  # FromString: "cannot be represented"
        return None
    if parsed_scale - scale > 38:  # Rescale has no multiplier: undefined in the reference
        return None
    d = int(digits) if digits else 0
    shift = scale - parsed_scale
    if shift >= 0:
        v = d * 10 ** shift
    else:
        v, r = divmod(d, 10 ** -shift)
        if r:  # a non-zero digit would be dropped
            return None
    if v >= 10 ** precision:
        return None
    return -v if neg else v


def _leap(y):
    return (y % 4 == 0 and y % 100 != 0) or y % 400 == 0


def _days_from_civil(y, m, d):
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def to_date(s):
    """exactly DDDD-DD-DD, a day of the proleptic Gregorian calendar, year 0001 … 9999"""
    s = _b(s)
    if len(s) != 10 or s[4] != 0x2D or s[7] != 0x2D or any(s[k] not in _DIGITS for k in (0, 1, 2, 3, 5, 6, 8, 9)):
        return None
    y, m, d = int(s[0:4]), int(s[5:7]), int(s[8:10])
    if y < 1 or not 1 <= m <= 12:
        return None
    dim = 29 if m == 2 and _leap(y) else 28 if m == 2 else 30 if m in (4, 6, 9, 11) else 31
    if not 1 <= d <= dim:
        return None
    return _days_from_civil(y, m, d)


def parse_column(kind, strings, precision=0, scale=0):
    """one ldb_gpu_map_strparse call: → (values with None for NULL, number of bad rows)"""
    fn = {"int": to_int, "decimal": lambda s: to_decimal(s, precision, scale), "date": to_date}[kind]
    out, bad = [], 0
    for s in strings:
        v = None if s is None else fn(s)
        bad += s is not None and v is None
        out.append(v)
    return out, bad


# ---------------------------------------------------------------- value → text
def from_int(v):
    return str(int(v)).encode()


def from_decimal(v, scale):
    """Decimal128::ToString(scale) of the unscaled integer v"""
    d = str(abs(int(v)))
    nd = len(d)
    adj = nd - 1 - scale
    sign = "-" if v < 0 else ""
    if scale == 0:
        t = d
    elif adj < -6:
        t = d[0] + ("." + d[1:] if nd > 1 else "") + "E-" + str(-adj)
    elif nd > scale:
        t = d[:nd - scale] + "." + d[nd - scale:]
    else:
        t = "0." + "0" * (scale - nd) + d
    return (sign + t).encode()


def from_date(days):
    """%F inside 0001-01-01 … 9999-12-31; None (the row is NULL) outside"""
    if not DATE_MIN <= days <= DATE_MAX:
        return None
    z = days + 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = mp + 3 if mp < 10 else mp - 9
    y = yoe + era * 400 + (m <= 2)
    return b"%04d-%02d-%02d" % (y, m, d)


def strcat_row(parts, row):
    """one row of ldb_gpu_map_strcat with the number and date parts: parts = bytes (a constant) | {"col": strings} |
    {"int": ints} | {"dec": unscaled ints, "scale": s} | {"date": days}; per-row lists with None for NULL"""
    out = b""
    for p in parts:
        if isinstance(p, (bytes, str)):
            out += _b(p)
            continue
        key = next(k for k in ("col", "int", "dec", "date") if k in p)
        v = p[key][row]
        if v is None:
            return None
        t = _b(v) if key == "col" else from_int(v) if key == "int" else from_decimal(v, p["scale"]) if key == "dec" else from_date(v)
        if t is None:
            return None
        out += t
    return out


def strcat(parts, n):
    return [strcat_row(parts, i) for i in range(n)]
