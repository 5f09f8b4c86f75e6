// ldb_datefn.h — the calendar arithmetic of the date functions (ldb_datefn.hip): device helpers only.
// Replaces (reference): DateHelper and toEpochNs (src/runtime/DateRuntime.cpp:11-75), which go through arrow's vendored
// date.h: floor<days>, year_month_day{sys_days} (civil from days) and sys_days{year_month_day} (days from civil) of the
// proleptic Gregorian calendar in UTC.
// A timestamp is split ONCE in 64 bits (one floor division by the constant 86 400 000 000 000); after that the day number of
// any int64 instant is within ±106 752 and the calendar runs in 32-bit integers — 64-bit division by a constant costs
// several times the instructions on this chip (d_extract_year in ldb_hash.hip divides in 64 bits throughout; it stays as
// it is, it is not the model).  A date32 column may hold ANY int32 day: the day shifted to the 0000-03-01 origin needs 33
// bits there, which d_civil handles by cases instead of widening.
#pragma once
#include "ldb_device.h"

#define LDB_NS_PER_DAY 86400000000000LL
#define LDB_DATE32_MIN (-719162) /* 0001-01-01 */
#define LDB_DATE32_MAX 2932896 /* 9999-12-31 */
#define LDB_MAX_MONTHS 240000 /* |m| above this leaves either range from anywhere inside it (20 000 years) */

struct DCivil {
   int32_t y;
   uint32_t m, d; // 1 … 12, 1 … 31
};
// an instant as (day, ns of that day), floor semantics: -1 ns is the last ns of 1969-12-31
__device__ __forceinline__ int32_t d_split_ns(int64_t ns, int64_t* ns_of_day) {
   int64_t q = ns / LDB_NS_PER_DAY;
   int64_t r = ns - q * LDB_NS_PER_DAY;
   if (r < 0) {
      r += LDB_NS_PER_DAY;
      q -= 1;
   }
   *ns_of_day = r;
   return (int32_t) q;
}
// whole seconds of a day from its ns (< 86 400 * 10^9 < 2^47)
__device__ __forceinline__ uint32_t d_sec_of_day(int64_t ns_of_day) { return (uint32_t) ((uint64_t) ns_of_day / 1000000000ull); }

// civil from days (date.h year_month_day::from_days) for every int32 day
__device__ __forceinline__ DCivil d_civil(int32_t day) {
   int32_t era;
   uint32_t doe;
   if (day >= 0) { // day + 719468 < 2^32: unsigned
      const uint32_t z = (uint32_t) day + 719468u;
      const uint32_t e = z / 146097u;
      era = (int32_t) e;
      doe = z - e * 146097u;
   } else { // no overflow on this side: signed floor division
      const int32_t z = day + 719468;
      era = (z >= 0 ? z : z - 146096) / 146097;
      doe = (uint32_t) (z - era * 146097);
   }
   const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
   const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
   const uint32_t mp = (5u * doy + 2u) / 153u;
   DCivil c;
   c.d = doy - (153u * mp + 2u) / 5u + 1u;
   c.m = mp < 10u ? mp + 3u : mp - 9u;
   c.y = (int32_t) yoe + era * 400 + (c.m <= 2u ? 1 : 0);
   return c;
}
// days from civil (date.h year_month_day::to_days): plain arithmetic, so a day past the end of its month runs over into the
// next one (2023-02-31 is 2023-03-03) exactly as sys_days{ymd} does.  Wrapping 32-bit arithmetic: the caller bounds y.
__device__ __forceinline__ int32_t d_days_from_civil(int32_t y, uint32_t m, uint32_t d) {
   y -= m <= 2u ? 1 : 0;
   const int32_t era = (y >= 0 ? y : y - 399) / 400;
   const uint32_t yoe = (uint32_t) (y - era * 400);
   const uint32_t doy = (153u * (m > 2u ? m - 3u : m + 9u) + 2u) / 5u + d - 1u;
   const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
   return (int32_t) ((uint32_t) era * 146097u + doe - 719468u);
}

// ---- EXTRACT(part): DateRuntime::extractYear … extractSecond (DateRuntime.cpp:99-116)
template <int PART>
__device__ __forceinline__ int64_t d_extract_day(int32_t day) { // of a date32 value
   if (PART >= LDB_DP_HOUR) return 0;
   const DCivil c = d_civil(day);
   return PART == LDB_DP_YEAR ? (int64_t) c.y : PART == LDB_DP_MONTH ? (int64_t) c.m : (int64_t) c.d;
}
template <int PART>
__device__ __forceinline__ int64_t d_extract_ns(int64_t ns) {
   int64_t nsod;
   const int32_t day = d_split_ns(ns, &nsod);
   if (PART <= LDB_DP_DAY) return d_extract_day<PART>(day);
   const uint32_t s = d_sec_of_day(nsod);
   return PART == LDB_DP_HOUR ? s / 3600u : PART == LDB_DP_MINUTE ? (s / 60u) % 60u : s % 60u;
}
// ---- TRUNC(part): DateRuntime::dateTrunc (DateRuntime.cpp:117-164) — the parts up to `part` kept, the finer ones at their
// first value.  The result of an instant before 1678-01-01 does not fit int64 (signed overflow in the reference): wrapped.
template <int PART>
__device__ __forceinline__ int32_t d_trunc_day(int32_t day) {
   if (PART >= LDB_DP_DAY) return day;
   const DCivil c = d_civil(day);
   return d_days_from_civil(c.y, PART == LDB_DP_YEAR ? 1u : c.m, 1u);
}
template <int PART>
__device__ __forceinline__ int64_t d_trunc_ns(int64_t ns) {
   int64_t nsod;
   const int32_t day = d_split_ns(ns, &nsod);
   uint64_t keep = 0; // ns of the day that stay
   if (PART >= LDB_DP_HOUR) {
      const uint32_t s = d_sec_of_day(nsod);
      const uint32_t unit = PART == LDB_DP_HOUR ? 3600u : PART == LDB_DP_MINUTE ? 60u : 1u;
      keep = (uint64_t) (s - s % unit) * 1000000000ull;
   }
   return (int64_t) ((uint64_t) (int64_t) d_trunc_day<PART>(day) * (uint64_t) LDB_NS_PER_DAY + keep);
}
// ---- ADD_MONTHS(m): DateHelper::addMonths (DateRuntime.cpp:35-40, :77-82) — year and month normalised by floor division,
// day of the month and time of day kept, NO clamping to the end of the target month (see d_days_from_civil).
// false = the result leaves the type's range (NULL).  |m| is tested first so that nothing below can overflow.
__device__ __forceinline__ bool d_add_months_civil(int32_t day, int64_t months, int32_t* out) {
   if (months > LDB_MAX_MONTHS || months < -LDB_MAX_MONTHS) return false;
   const DCivil c = d_civil(day);
   const int32_t mi = (int32_t) c.m - 1 + (int32_t) months;
   const int32_t dy = (mi >= 0 ? mi : mi - 11) / 12;
   *out = d_days_from_civil(c.y + dy, (uint32_t) (mi - dy * 12) + 1u, c.d);
   return true;
}
__device__ __forceinline__ bool d_add_months_day(int32_t day, int64_t months, int32_t* out) {
   // a day this far outside 0001 … 9999 cannot come back in 240 000 months (< 7 500 000 days), and inside the bound the
   // 32-bit calendar is far from wrapping
   if (day < LDB_DATE32_MIN - 7500000 || day > LDB_DATE32_MAX + 7500000) return false;
   int32_t r;
   if (!d_add_months_civil(day, months, &r)) return false;
   *out = r;
   return r >= LDB_DATE32_MIN && r <= LDB_DATE32_MAX;
}
__device__ __forceinline__ bool d_add_months_ns(int64_t ns, int64_t months, int64_t* out) {
   int64_t nsod;
   const int32_t day = d_split_ns(ns, &nsod);
   int32_t r;
   if (!d_add_months_civil(day, months, &r)) return false;
   const i128 v = (i128) r * (i128) LDB_NS_PER_DAY + (i128) nsod;
   *out = (int64_t) v;
   return v >= (i128) INT64_MIN && v <= (i128) INT64_MAX;
}
