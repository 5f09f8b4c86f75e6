// ldb_strcast.h — device helpers of the casts between text and int / decimal / date (ldb_strfn.hip: the INT / DECIMAL /
// DATE parts of a concatenation; ldb_strcast.hip: a utf8 column parsed as INT64 / DECIMAL128 / DATE32).  Ahead-of-time
// kernels only: not one of the sources hiprtc compiles.  Everything here works on values and byte addresses alone.
//
// Text of a number (reference src/runtime/StringRuntime.cpp: fromInt :201-212, fromDecimal :217-222 = arrow's
// Decimal128::ToString(scale), fromDate :452-456 = "%F"): the digits are produced ONCE per number, as 40 ASCII bytes in five
// registers — the value is cut into groups of eight digits with 64-bit arithmetic (divisions by the constant 10^8 only), and
// a group becomes eight bytes with three packed multiply / shift / subtract steps — and any window of the text is then cut
// out of those registers with shifts.  No division per output byte.
// Parsing (toInt :174-185 = std::stoll that must consume the string, toDecimal :187-200 = Decimal128::FromString then
// Rescale, toDate :439-444 = arrow's ParseValue<Date32Type>): the bytes come eight at a time, a parser stops at the first byte
// that makes its string bad, no load goes past the value buffer.
#pragma once
#include "ldb_device.h"

typedef uint64_t __attribute__((aligned(1))) sc_u64_unaligned;

// ---------------------------------------------------------------- powers of ten
struct DPow10Tab {
   uint64_t lo[39], hi[39];
};
constexpr DPow10Tab d_make_pow10_tab() {
   DPow10Tab t{};
   u128 r = 1;
   for (int k = 0; k < 39; k++) {
      t.lo[k] = (uint64_t) r;
      t.hi[k] = (uint64_t) (r >> 64);
      r *= 10;
   }
   return t;
}
static __device__ const DPow10Tab D_POW10 = d_make_pow10_tab();
__device__ __forceinline__ u128 d_pow10_u128(uint32_t k) { return ((u128) D_POW10.hi[k] << 64) | D_POW10.lo[k]; } // k <= 38
// decimal digits of a < 10^38 (1 for 0): binary search in the table
__device__ __forceinline__ uint32_t d_dec_digits_u128(u128 a) {
   uint32_t lo = 1, hi = 38; // the smallest nd in [1, 38] with a < 10^nd
   while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a < d_pow10_u128(mid)) hi = mid;
      else lo = mid + 1;
   }
   return lo;
}

// ---------------------------------------------------------------- digits
#define SC_ZEROS 0x3030303030303030ull
// x < 10^8 as eight ASCII digits, the first digit in the lowest byte
__device__ __forceinline__ uint64_t d_ascii8(uint32_t x) {
   const uint32_t top = x / 10000u, bot = x - top * 10000u;
   const uint64_t m = (uint64_t) top | ((uint64_t) bot << 32); // two numbers < 10^4, one per 32 bits
   const uint64_t h = ((m * 10486ull) >> 20) & 0x0000007F0000007Full; // each / 100 (exact below 43 699)
   const uint64_t p = h | ((m - 100ull * h) << 16); // four numbers < 100, one per 16 bits
   const uint64_t t = ((p * 103ull) >> 10) & 0x000F000F000F000Full; // each / 10 (exact below 179)
   return (t | ((p - 10ull * t) << 8)) + SC_ZEROS;
}
struct DDigits {
   uint64_t g[5]; // 40 ASCII digits, right-aligned: byte 0 of g[0] is the leftmost, byte 7 of g[4] the ones
   uint32_t nd; // significant digits (1 for 0): digit j from the left is byte 40 - nd + j
};
__device__ __forceinline__ void d_digits_count(DDigits& d) {
   uint32_t lz = 39; // (zero keeps its last '0')
#pragma unroll
   for (int w = 4; w >= 0; w--) {
      const uint64_t z = d.g[w] ^ SC_ZEROS;
      if (z) lz = 8u * (uint32_t) w + ((uint32_t) __builtin_ctzll(z) >> 3);
   }
   d.nd = 40u - lz;
}
__device__ __forceinline__ DDigits d_digits_u64(uint64_t a) {
   DDigits d;
   const uint64_t q1 = a / 100000000ull;
   const uint32_t r1 = (uint32_t) (a - q1 * 100000000ull);
   const uint32_t q2 = (uint32_t) (q1 / 100000000ull), r2 = (uint32_t) (q1 - (uint64_t) q2 * 100000000ull);
   d.g[0] = d.g[1] = SC_ZEROS;
   d.g[2] = q1 ? d_ascii8(q2) : SC_ZEROS; // (q2 < 1845)
   d.g[3] = q1 ? d_ascii8(r2) : SC_ZEROS;
   d.g[4] = d_ascii8(r1);
   d_digits_count(d);
   return d;
}
// a < 10^40 (every |decimal128| is): short division of four 32-bit limbs by 10^8, four times; a numerator is below
// 10^8 * 2^32 < 2^59
__device__ __forceinline__ DDigits d_digits_u128(u128 a) {
   if ((uint64_t) (a >> 64) == 0) return d_digits_u64((uint64_t) a);
   uint32_t l[4] = {(uint32_t) a, (uint32_t) (a >> 32), (uint32_t) (a >> 64), (uint32_t) (a >> 96)};
   DDigits d;
#pragma unroll
   for (int p = 4; p >= 1; p--) {
      uint64_t rem = 0;
#pragma unroll
      for (int k = 3; k >= 0; k--) {
         const uint64_t cur = (rem << 32) | l[k];
         const uint64_t q = cur / 100000000ull;
         rem = cur - q * 100000000ull;
         l[k] = (uint32_t) q;
      }
      d.g[p] = d_ascii8((uint32_t) rem);
   }
   d.g[0] = d_ascii8(l[0]); // what is left is below 10^8
   d_digits_count(d);
   return d;
}
__device__ __forceinline__ u128 d_mask_bytes(uint32_t cnt) { return cnt >= 16 ? ~(u128) 0 : (((u128) 1) << (8 * cnt)) - 1; }
// bytes s … s + cnt - 1 of the 40 (cnt <= 16, s + cnt <= 40), the first in the lowest byte
__device__ __forceinline__ u128 d_digits_bytes(const DDigits& d, uint32_t s, uint32_t cnt) {
   const uint32_t w = s >> 3, sh = 8 * (s & 7);
   const uint64_t a = w == 0 ? d.g[0] : w == 1 ? d.g[1] : w == 2 ? d.g[2] : w == 3 ? d.g[3] : d.g[4];
   const uint64_t b = w == 0 ? d.g[1] : w == 1 ? d.g[2] : w == 2 ? d.g[3] : w == 3 ? d.g[4] : 0;
   const uint64_t c = w == 0 ? d.g[2] : w == 1 ? d.g[3] : w == 2 ? d.g[4] : 0;
   const uint64_t lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
   const uint64_t hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
   return ((((u128) hi) << 64) | lo) & d_mask_bytes(cnt);
}

// ---------------------------------------------------------------- the text of a number
// [-]["0." zeros][na digits][.][the other digits][E-x]: every form of fromInt and of Decimal128::ToString(scale)
struct DNumText {
   DDigits d;
   uint32_t neg; // 1: a leading '-'
   uint32_t lead; // bytes of "0." and the zeros behind it (0: none)
   uint32_t na; // digits in front of the point (all of them when there is none)
   uint32_t dot; // 1: a '.' behind those
   uint32_t exp; // x of a trailing "E-x" (0: none; otherwise 7 … 38)
};
__device__ __forceinline__ uint32_t d_num_text_len(const DNumText& t) { return t.neg + t.lead + t.d.nd + t.dot + (t.exp ? (t.exp >= 10 ? 4u : 3u) : 0u); }
// the form alone, from the number of digits: adj = nd - 1 - scale; scale 0: the digits; adj < -6: d[.ddd]E-x; nd > scale:
// a point before the last `scale` digits; otherwise "0.", scale - nd zeros, the digits
__device__ __forceinline__ void d_dec_form(DNumText& t, int32_t scale) {
   const int32_t nd = (int32_t) t.d.nd, adj = nd - 1 - scale;
   t.lead = 0;
   t.na = (uint32_t) nd;
   t.dot = 0;
   t.exp = 0;
   if (scale <= 0) return;
   if (adj < -6) {
      t.na = 1;
      t.dot = nd > 1 ? 1u : 0u;
      t.exp = (uint32_t) -adj;
   } else if (nd > scale) {
      t.na = (uint32_t) (nd - scale);
      t.dot = 1;
   } else {
      t.lead = (uint32_t) (2 + scale - nd);
   }
}
__device__ __forceinline__ DNumText d_int_text(int64_t v) {
   DNumText t;
   t.neg = v < 0 ? 1u : 0u;
   t.d = d_digits_u64(v < 0 ? 0 - (uint64_t) v : (uint64_t) v);
   d_dec_form(t, 0);
   return t;
}
__device__ __forceinline__ DNumText d_dec_text(i128 v, int32_t scale) {
   DNumText t;
   t.neg = v < 0 ? 1u : 0u;
   t.d = d_digits_u128(v < 0 ? (u128) 0 - (u128) v : (u128) v);
   d_dec_form(t, scale);
   return t;
}
// bytes of the text of v at `scale` without its digits (the length kernel)
__device__ __forceinline__ uint32_t d_dec_text_len(i128 v, int32_t scale) {
   DNumText t;
   t.neg = v < 0 ? 1u : 0u;
   t.d.nd = d_dec_digits_u128(v < 0 ? (u128) 0 - (u128) v : (u128) v);
   d_dec_form(t, scale);
   return d_num_text_len(t);
}
// `seg` (1 … 16) bytes of the text from byte q, the first in the lowest byte
__device__ __forceinline__ u128 d_num_text_bytes(const DNumText& t, uint32_t q, uint32_t seg) {
   const uint32_t end = q + seg, s0 = 40u - t.d.nd;
   u128 r = 0;
   uint32_t P = 0; // first byte of the piece at hand
   if (t.neg && q == 0) r = '-';
   P += t.neg;
   if (t.lead) { // '0' bytes with a '.' at byte 1
      const uint32_t b = P > q ? P : q, e = P + t.lead < end ? P + t.lead : end;
      if (b < e) {
         const uint32_t off = b - P, cnt = e - b;
         u128 z = ((((u128) SC_ZEROS) << 64) | SC_ZEROS) & d_mask_bytes(cnt);
         if (off <= 1 && 1 < off + cnt) z ^= (u128) ('0' ^ '.') << (8 * (1 - off));
         r |= z << (8 * (b - q));
      }
      P += t.lead;
   }
   { // the digits in front of the point
      const uint32_t b = P > q ? P : q, e = P + t.na < end ? P + t.na : end;
      if (b < e) r |= d_digits_bytes(t.d, s0 + (b - P), e - b) << (8 * (b - q));
      P += t.na;
   }
   if (t.dot) {
      if (P >= q && P < end) r |= (u128) '.' << (8 * (P - q));
      P += 1;
   }
   const uint32_t nb = t.d.nd - t.na;
   if (nb) {
      const uint32_t b = P > q ? P : q, e = P + nb < end ? P + nb : end;
      if (b < e) r |= d_digits_bytes(t.d, s0 + t.na + (b - P), e - b) << (8 * (b - q));
      P += nb;
   }
   if (t.exp && end > P) {
      const uint32_t x = t.exp >= 10 ? ('E' | ('-' << 8) | (('0' + t.exp / 10) << 16) | (('0' + t.exp % 10) << 24)) : ('E' | ('-' << 8) | (('0' + t.exp) << 16));
      const uint32_t len = t.exp >= 10 ? 4u : 3u;
      const uint32_t b = P > q ? P : q, e = P + len < end ? P + len : end;
      if (b < e) r |= ((u128) (x >> (8 * (b - P))) & d_mask_bytes(e - b)) << (8 * (b - q));
   }
   return r;
}

// ---------------------------------------------------------------- dates (proleptic Gregorian, days since 1970-01-01)
#define SC_DATE_MIN (-719162) // 0001-01-01
#define SC_DATE_MAX 2932896 // 9999-12-31
#define SC_DATE_TEXT_LEN 10
// YYYY-MM-DD of a day in [SC_DATE_MIN, SC_DATE_MAX]: `seg` bytes from byte q
__device__ __forceinline__ u128 d_date_text_bytes(int32_t days, uint32_t q, uint32_t seg) {
   const uint32_t z = (uint32_t) (days + 719468); // days since 0000-03-01 (positive in the range)
   const uint32_t era = z / 146097u, doe = z - era * 146097u;
   const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
   const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
   const uint32_t mp = (5u * doy + 2u) / 153u;
   const uint32_t d = doy - (153u * mp + 2u) / 5u + 1u;
   const uint32_t m = mp < 10 ? mp + 3 : mp - 9;
   const uint32_t y = yoe + era * 400u + (m <= 2 ? 1u : 0u);
   const uint64_t x = d_ascii8(y * 10000u + m * 100u + d); // "YYYYMMDD"
   const uint64_t lo = (x & 0xFFFFFFFFull) | ((uint64_t) '-' << 32) | (((x >> 32) & 0xFFFFull) << 40) | ((uint64_t) '-' << 56);
   const u128 text = (((u128) (x >> 48)) << 64) | lo;
   return (text >> (8 * q)) & d_mask_bytes(seg);
}

// ---------------------------------------------------------------- parsing
// eight bytes from byte `at` of the value buffer, of which the caller looks at the first min(8, left) — the rest of its
// string; no load goes past `avail`, the bytes of the buffer: its last bytes take byte loads
__device__ __forceinline__ uint64_t d_str_load8(const uint8_t* base, uint64_t at, uint32_t left, uint64_t avail) {
   if (at + 8 <= avail) return *(const LDB_GLOBAL sc_u64_unaligned*) (base + at);
   uint64_t x = 0;
   for (uint32_t k = 0; k < left && k < 8; k++) x |= (uint64_t) base[at + k] << (8 * k);
   return x;
}
// std::stoll(s, &pos) with pos == len: blanks (C-locale isspace), one sign, digits to the end, a value inside int64
__device__ __forceinline__ bool d_parse_int64(const uint8_t* base, uint64_t at, uint32_t len, uint64_t avail, int64_t* out) {
   uint32_t st = 0; // 0: blanks, 1: behind the sign, 2: digits
   bool neg = false;
   uint64_t acc = 0;
   for (uint32_t k = 0; k < len; k += 8) {
      uint64_t x = d_str_load8(base, at + k, len - k, avail);
      const uint32_t m = len - k < 8 ? len - k : 8;
      for (uint32_t j = 0; j < m; j++, x >>= 8) {
         const uint32_t c = (uint32_t) (x & 0xFF), dgt = c - '0';
         if (dgt <= 9) {
            // acc * 10 + dgt must stay <= 2^63 - 1 (2^63 behind a '-'); 2^63 = 922337203685477580 * 10 + 8
            if (acc > 922337203685477580ull || (acc == 922337203685477580ull && dgt > (neg ? 8u : 7u))) return false;
            acc = acc * 10 + dgt;
            st = 2;
         } else if (st == 0 && (c == ' ' || c - 9u <= 4u)) {
         } else if (st == 0 && (c == '+' || c == '-')) {
            neg = c == '-';
            st = 1;
         } else {
            return false;
         }
      }
   }
   if (st != 2) return false;
   *out = neg ? (int64_t) (0 - acc) : (int64_t) acc;
   return true;
}
// Decimal128::FromString, then Rescale to `scale`, then |v| < 10^precision.  FromString: sign? digits* (. digits*)?
// ([eE] +? -? digits+)? with a digit in front of the exponent, which is an int32; it refuses a scale below -38.  The digits
// are collected without their trailing zeros (D, and z zeros pending), so that no step divides: the value is
// D * 10^(z + scale - parsed scale), bad when that power is negative (a non-zero digit would be dropped).  More than 38
// significant digits are bad, and so is a parsed scale more than 38 above `scale` (the reference's Rescale has no
// multiplier for it), zero digits or not.
__device__ __forceinline__ bool d_parse_decimal(const uint8_t* base, uint64_t at, uint32_t len, uint64_t avail, int32_t precision, int32_t scale, i128* out) {
   enum { S_START, S_SIGNED, S_WHOLE, S_FRAC, S_E, S_EPLUS, S_EMINUS, S_EDIG };
   uint32_t st = S_START;
   bool neg = false, eneg = false, any = false;
   uint64_t d64 = 0; // D while it has at most 19 digits (10^19 < 2^64): 64-bit arithmetic for all but the longest numbers
   u128 D = 0;
   uint32_t nD = 0; // digits in D
   uint32_t nsig = 0, z = 0; // digits from the first non-zero one on; the zeros at their end, not yet in D
   int64_t F = 0, E = 0; // digits behind the point; |exponent|
   for (uint32_t k = 0; k < len; k += 8) {
      uint64_t x = d_str_load8(base, at + k, len - k, avail);
      const uint32_t m = len - k < 8 ? len - k : 8;
      for (uint32_t j = 0; j < m; j++, x >>= 8) {
         const uint32_t c = (uint32_t) (x & 0xFF), dgt = c - '0';
         if (dgt <= 9) {
            if (st <= S_FRAC) {
               if (st != S_FRAC) st = S_WHOLE;
               else F++;
               any = true;
               if (dgt == 0) {
                  if (nsig) nsig++, z++;
               } else {
                  nsig++;
                  for (uint32_t a = z + 1; a; a--) { // the pending zeros, then this digit
                     const uint32_t add = a == 1 ? dgt : 0;
                     if (nD < 19) {
                        d64 = d64 * 10 + add;
                     } else {
                        if (nD == 19) D = d64;
                        D = D * 10 + add;
                     }
                     nD++;
                  }
                  z = 0;
               }
               if (nsig > 38) return false;
            } else {
               st = S_EDIG;
               E = E * 10 + dgt;
               if (E > ((int64_t) 1 << 31) - (eneg ? 0 : 1)) return false; // not an int32
            }
         } else if (c == '.') {
            if (st > S_WHOLE) return false;
            st = S_FRAC;
         } else if (c == 'e' || c == 'E') {
            if ((st != S_WHOLE && st != S_FRAC) || !any) return false;
            st = S_E;
         } else if (c == '+' || c == '-') {
            if (st == S_START) {
               neg = c == '-';
               st = S_SIGNED;
            } else if (st == S_E) {
               eneg = c == '-';
               st = eneg ? S_EMINUS : S_EPLUS;
            } else if (st == S_EPLUS && c == '-') { // ("e+-5": the '+' is skipped, then an int32 is read)
               eneg = true;
               st = S_EMINUS;
            } else {
               return false;
            }
         } else {
            return false;
         }
      }
   }
   if (!(st == S_EDIG || ((st == S_WHOLE || st == S_FRAC) && any))) return false;
   const int64_t ps = F - (eneg ? -E : E); // the parsed scale
   if (-ps > 38 || ps - scale > 38) return false;
   if (nD <= 19) D = d64;
   if (D == 0) {
      *out = 0;
      return true;
   }
   const int64_t e10 = (int64_t) z + scale - ps;
   if (e10 < 0 || e10 > precision) return false;
   if (D >= d_pow10_u128((uint32_t) (precision - e10))) return false;
   const u128 v = D * d_pow10_u128((uint32_t) e10);
   *out = neg ? (i128) ((u128) 0 - v) : (i128) v;
   return true;
}
// exactly DDDD-DD-DD, a day of the proleptic Gregorian calendar in the years 0001 … 9999
__device__ __forceinline__ bool d_parse_date(const uint8_t* base, uint64_t at, uint32_t len, uint64_t avail, int32_t* out) {
   if (len != SC_DATE_TEXT_LEN) return false;
   const uint64_t lo = d_str_load8(base, at, 10, avail), hi = d_str_load8(base, at + 8, 2, avail);
   uint32_t dg[10];
   bool ok = true;
#pragma unroll
   for (int k = 0; k < 10; k++) {
      const uint32_t c = (uint32_t) ((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFF);
      dg[k] = c - '0';
      ok = ok && (k == 4 || k == 7 ? c == '-' : dg[k] <= 9);
   }
   if (!ok) return false;
   const uint32_t y = dg[0] * 1000 + dg[1] * 100 + dg[2] * 10 + dg[3], m = dg[5] * 10 + dg[6], d = dg[8] * 10 + dg[9];
   if (y < 1 || m < 1 || m > 12 || d < 1) return false;
   const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
   const uint32_t dim = m == 2 ? (leap ? 29u : 28u) : ((0x0A50u >> m) & 1u) ? 30u : 31u; // bits 4, 6, 9, 11: the 30-day months
   if (d > dim) return false;
   const uint32_t yy = m <= 2 ? y - 1 : y; // (days_from_civil; yy >= 0)
   const uint32_t era = yy / 400u, yoe = yy - era * 400u;
   const uint32_t doy = (153u * (m > 2 ? m - 3 : m + 9) + 2u) / 5u + d - 1u;
   const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
   *out = (int32_t) (era * 146097u + doe) - 719468;
   return true;
}
