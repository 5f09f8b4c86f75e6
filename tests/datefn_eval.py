"""Plain-Python restatement of the date functions (ldb_gpu_map_datefn, the `datediff` expression) on Python integers.

A DATE32 value is a day number since 1970-01-01, a timestamp an int64 of ns since the epoch; both go through floor
division into days and the proleptic Gregorian calendar in UTC (Hinnant's civil_from_days / days_from_civil, the algorithm
of the date.h the reference's DateRuntime uses).  `None` is NULL.  tests/test_datefn_api.py pins this file to the reference
(tests/golden/ref_datefn.json) and to datetime; tests/test_gpu_datefn.py compares the device with it bit for bit."""

NS_PER_DAY = 86_400_000_000_000
PARTS = ("year", "month", "day", "hour", "minute", "second")
DATE32_MIN, DATE32_MAX = -719162, 2932896  # 0001-01-01 … 9999-12-31
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
MAX_MONTHS = 240000


def civil_from_days(z):
    z += 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (1 if m <= 2 else 0), m, d


def days_from_civil(y, m, d):
    """plain arithmetic: a day past the end of its month runs over into the next one (2023-02-31 is 2023-03-03)"""
    y -= 1 if m <= 2 else 0
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _split(x, is_date):
    """(day, ns of the day)"""
    return (x, 0) if is_date else (x // NS_PER_DAY, x % NS_PER_DAY)


def extract(part, x, is_date):
    if x is None:
        return None
    day, ns = _split(x, is_date)
    y, m, d = civil_from_days(day)
    s = ns // 1_000_000_000
    return {"year": y, "month": m, "day": d, "hour": s // 3600, "minute": s // 60 % 60, "second": s % 60}[part]


def trunc(part, x, is_date):
    """the input's type; an int64 instant before 1678-01-01 (and a day whose year starts before INT32_MIN) wraps"""
    if x is None:
        return None
    day, ns = _split(x, is_date)
    k = PARTS.index(part)
    if k < 2:
        y, m, _ = civil_from_days(day)
        day = days_from_civil(y, 1 if k == 0 else m, 1)
    if is_date:
        return _wrap(day, 32)
    s = ns // 1_000_000_000
    unit = {3: 3600, 4: 60, 5: 1}.get(k)
    keep = (s - s % unit) * 1_000_000_000 if unit else 0
    return _wrap(day * NS_PER_DAY + keep, 64)


def add_months(x, months, is_date):
    """None when an input is NULL or the result leaves the type's range; no clamping at the end of a month"""
    if x is None or months is None or abs(months) > MAX_MONTHS:
        return None
    day, ns = _split(x, is_date)
    y, m, d = civil_from_days(day)
    mi = m - 1 + months
    dy = mi // 12
    r = days_from_civil(y + dy, mi - dy * 12 + 1, d)
    if is_date:
        return r if DATE32_MIN <= r <= DATE32_MAX else None
    v = r * NS_PER_DAY + ns
    return v if INT64_MIN <= v <= INT64_MAX else None


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def datediff(unit, end, start, is_date):
    """truncating divisions, as the reference's: -1.5 s → -1, -90 s → -1 minute; a date32 difference is whole days"""
    if end is None or start is None:
        return None
    per_day = {"day": 1, "hour": 24, "minute": 1440, "second": 86400}[unit]
    if is_date:
        return (end - start) * per_day
    s = _tdiv(end - start, 1_000_000_000)
    return s if unit == "second" else _tdiv(s, 86400 // per_day)
