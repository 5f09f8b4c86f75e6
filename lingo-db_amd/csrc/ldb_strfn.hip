// ldb_strfn.hip — string expressions as computed columns: upper / lower / || / cast(int | decimal | date as varchar) / length.
// Replaces (reference): the runtime calls the SQL frontend emits for these (sql_mlir_translator.cpp:910-936, registered in
// Dialect/DB/RuntimeFunctions/RuntimeFunctions.cpp:276-285) and src/runtime/StringRuntime.cpp executes per tuple:
// toUpper / toLower (:355-364, :396-418: std::toupper / std::tolower byte by byte in the C locale — only a-z / A-Z change,
// bytes >= 0x80 pass through), concat (:419-432: bytes of a, then bytes of b), fromInt (:201-212: arrow's StringFormatter —
// plain decimal with a leading '-'), fromDecimal (:217-222) and fromDate (:452-456; both in ldb_strcast.h), substr (:292-319,
// see ldb_strfn.h) and len (:276-290: bytes that are not 10xxxxxx).
//
// One result row = the PARTS of that row left to right (ldb_strpart: a utf8 column — whole or a character window, as it is
// or case-mapped —, a constant, or an integer / decimal / date column as text).  Three steps:
//   k_strcat_lens   one output length per row + the validity bitmap (written as 64-bit words from a wave ballot).  A whole
//                   column part costs two offset loads, an INT / DECIMAL part a digit count, a DATE part a range check; only
//                   a windowed part reads its string,
//                   and leaves (first byte, byte length) of the window per row for the fill.
//   ldb_exclusive_scan_i64   lengths → 64-bit offsets.
//   k_strcat_fill   parallel over OUTPUT BYTES: see there.
#include "ldb_internal.h"
#include "ldb_strfn.h"
#include "ldb_strcast.h"
#include <climits>

struct DSPart {
   DCol col;
   int32_t kind; // ldb_strpart_kind
   int32_t strcase; // ldb_strcase
   int32_t windowed; // COL: (from, for_len) is not the whole string
   int32_t widx; // windowed parts numbered 0, 1, …: aux[(2 * widx) * n + i] = first byte, aux[(2 * widx + 1) * n + i] = bytes
   int64_t from, for_len;
   uint64_t const_off; // CONST: first byte in the constants buffer
   uint32_t const_len;
   uint32_t pad;
   uint64_t src_bytes; // COL: bytes in the column's value buffer, CONST: bytes in the constants buffer (reads never go past it)
};
struct DStrcat {
   int32_t n_parts;
   int32_t nullable;
   uint64_t consts; // device address of the constants' bytes, back to back
   DSPart p[LDB_MAX_STRPARTS];
};

#define SF_WORD 16 // W: bytes of output one lane produces per tile (one 16-byte vector store)
#define SF_BLOCK 256
#define SF_TILE (SF_WORD * SF_BLOCK) // T: bytes of output per tile
#define SF_TILES_PER_GROUP 16 // consecutive tiles one workgroup walks after ONE binary search in the offsets
#define SF_LDS_ROWS 1024 // offsets staged in LDS at a time (+ 1)
extern "C" int32_t ldb_strcat_tile_bytes() { return SF_TILE; }
extern "C" int32_t ldb_strcat_lds_rows() { return SF_LDS_ROWS; }

typedef uint64_t __attribute__((aligned(1))) sf_u64_unaligned;

__device__ __forceinline__ uint32_t d_dec_digits(uint64_t a) { // decimal digits of a (1 for 0)
   uint32_t d = 1;
   while (a >= 10) {
      a /= 10;
      d++;
   }
   return d;
}
// StringRuntime::fromInt: bytes of the decimal text of v
__device__ __forceinline__ uint32_t d_int_text_len(int64_t v) { return d_dec_digits(v < 0 ? 0 - (uint64_t) v : (uint64_t) v) + (v < 0 ? 1u : 0u); }

// length in bytes of part p on logical row i; *ok = false when the part is NULL there.  `aux` as written by k_strcat_lens
// (the fill) or NULL (the length kernel itself: a windowed part is measured here and its window returned in *w0 / *wl).
__device__ __forceinline__ uint32_t d_part_len(const DSPart& p, uint64_t i, uint64_t n, const uint32_t* __restrict__ aux, bool* ok, uint32_t* w0, uint32_t* wl) {
   if (p.kind == LDB_SP_CONST) return p.const_len;
   const uint32_t row = d_phys_row(p.col, i);
   if (!d_valid(p.col, row)) {
      *ok = false;
      return 0;
   }
   if (p.kind == LDB_SP_INT) return d_int_text_len(d_load_i64(p.col, row));
   if (p.kind == LDB_SP_DECIMAL) return d_dec_text_len(d_load_i128(p.col, row), p.col.scale);
   if (p.kind == LDB_SP_DATE) { // fromDate is ten bytes inside 0001-01-01 … 9999-12-31 only: a day outside makes the row NULL
      const int64_t day = d_load_i64(p.col, row);
      if (day < SC_DATE_MIN || day > SC_DATE_MAX) *ok = false;
      return SC_DATE_TEXT_LEN;
   }
   if (!p.windowed) {
      uint32_t len;
      (void) d_load_str(p.col, row, &len);
      return len;
   }
   if (aux) return aux[(2 * (uint64_t) p.widx + 1) * n + i];
   uint32_t len, b0, b1;
   const uint8_t* s = d_load_str(p.col, row, &len);
   d_substr_range(s, len, p.from, p.for_len, &b0, &b1);
   *w0 = b0;
   *wl = b1 - b0;
   return b1 - b0;
}

// Thread t of the grid takes rows t, t + T, … (T a multiple of 64): a wave holds 64 consecutive rows from a multiple of 64 =
// one word of the Arrow validity bitmap, written from one ballot (the scheme of map_fexpr_body).
__global__ __launch_bounds__(256) void k_strcat_lens(DStrcat d, uint64_t n, int64_t* __restrict__ lens, uint32_t* __restrict__ aux, uint64_t* __restrict__ valid_words) {
   const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
   const uint32_t lane = d_lane_id();
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i - lane < n; i += stride) {
      const bool in = i < n;
      bool ok = in;
      int64_t total = 0;
      if (in) {
         for (int k = 0; k < d.n_parts; k++) {
            uint32_t w0 = 0, wl = 0;
            const uint32_t l = d_part_len(d.p[k], i, n, nullptr, &ok, &w0, &wl);
            total += l;
            if (d.p[k].kind == LDB_SP_COL && d.p[k].windowed) {
               aux[(2 * (uint64_t) d.p[k].widx) * n + i] = w0;
               aux[(2 * (uint64_t) d.p[k].widx + 1) * n + i] = wl;
            }
         }
         lens[i] = ok ? total : 0; // a NULL row has no bytes
      }
      if (valid_words) { // (wave-uniform)
         const uint64_t word = __ballot(ok);
         if (lane == 0 && in) valid_words[i >> 6] = word;
      }
   }
}

// std::toupper / std::tolower in the C locale on eight packed bytes: a byte changes iff it is in a-z (A-Z); no per-byte
// branch.  y = the low seven bits of every byte; y + (0x80 - lo) sets bit 7 iff y >= lo (no carry leaves a byte: y <= 0x7F).
__device__ __forceinline__ uint64_t d_swar_case(uint64_t x, int strcase) {
   const uint64_t ones = 0x0101010101010101ull, high = 0x8080808080808080ull;
   const uint64_t y = x & ~high;
   if (strcase == LDB_SC_UPPER) {
      const uint64_t m = (y + (0x80 - 'a') * ones) & ~(y + (0x80 - ('z' + 1)) * ones) & ~x & high;
      return x - (m >> 2); // 0x80 >> 2 = 0x20
   }
   const uint64_t m = (y + (0x80 - 'A') * ones) & ~(y + (0x80 - ('Z' + 1)) * ones) & ~x & high;
   return x + (m >> 2);
}
// `seg` (1 … 16) bytes of part p on logical row i, from byte `q` of the part's text, as a little-endian 128-bit value
__device__ __forceinline__ u128 d_part_bytes(const DStrcat& d, const DSPart& p, uint64_t i, uint64_t n, const uint32_t* __restrict__ aux, uint32_t q, uint32_t seg) {
   // the text of a number is produced once, in registers (ldb_strcast.h), and the bytes asked for are cut out of it
   if (p.kind == LDB_SP_INT) return d_num_text_bytes(d_int_text(d_load_i64(p.col, d_phys_row(p.col, i))), q, seg);
   if (p.kind == LDB_SP_DECIMAL) return d_num_text_bytes(d_dec_text(d_load_i128(p.col, d_phys_row(p.col, i)), p.col.scale), q, seg);
   if (p.kind == LDB_SP_DATE) return d_date_text_bytes((int32_t) d_load_i64(p.col, d_phys_row(p.col, i)), q, seg);
   uint64_t at, avail; // first source byte in its buffer, bytes of the buffer
   const uint8_t* base;
   if (p.kind == LDB_SP_CONST) {
      base = gptr<uint8_t>(d.consts);
      at = p.const_off + q;
   } else {
      const uint32_t row = d_phys_row(p.col, i);
      base = gptr<uint8_t>(p.col.values);
      at = (uint64_t) gptr<int64_t>(p.col.offsets)[row] + q;
      if (p.windowed) at += aux[(2 * (uint64_t) p.widx) * n + i];
   }
   avail = p.src_bytes;
   uint64_t lo = 0, hi = 0;
   if (at + 16 <= avail) { // two unaligned 8-byte loads, inside the buffer
      lo = *(const LDB_GLOBAL sf_u64_unaligned*) (base + at);
      if (seg > 8) hi = *(const LDB_GLOBAL sf_u64_unaligned*) (base + at + 8);
   } else { // the last bytes of the buffer: byte loads
      for (uint32_t k = 0; k < seg; k++) {
         const uint64_t c = base[at + k];
         if (k < 8) lo |= c << (8 * k);
         else hi |= c << (8 * (k - 8));
      }
   }
   if (p.strcase != LDB_SC_NONE) {
      lo = d_swar_case(lo, p.strcase);
      hi = d_swar_case(hi, p.strcase);
   }
   u128 r = ((u128) hi << 64) | lo;
   if (seg < 16) r &= (((u128) 1) << (8 * seg)) - 1;
   return r;
}

// The fill, parallel over OUTPUT BYTES.  The value buffer is cut into tiles of T = SF_TILE bytes; a workgroup walks
// SF_TILES_PER_GROUP consecutive tiles.  It finds the row that holds the first byte of its first tile by binary search in
// the offsets (once; every further tile starts where the previous one ended), stages the offsets of the rows that
// intersect the tile in LDS — SF_LDS_ROWS at a time, in a loop when a tile holds more rows than that (runs of empty or
// 1-byte rows) — and every lane assembles ONE aligned 16-byte word of the tile in registers: for the bytes of its word it
// resolves (row, part, byte of the part) from the staged offsets and the parts' lengths, fetches the source bytes of each
// (row, part) segment with two unaligned 8-byte loads, case-maps them as packed words, shifts them into place, and issues
// one 16-byte store.  Only the last word of the buffer is partial (byte stores).  The work of a lane is bounded by the word
// and the rows of its tile, whatever the length of any single row; no atomics.
__global__ __launch_bounds__(SF_BLOCK) void k_strcat_fill(DStrcat d, uint64_t n, const int64_t* __restrict__ offs, const uint32_t* __restrict__ aux, uint8_t* __restrict__ out, uint64_t total) {
   __shared__ int64_t s_off[SF_LDS_ROWS + 1];
   const uint32_t tid = threadIdx.x;
   const uint64_t n_tiles = (total + SF_TILE - 1) / SF_TILE;
   const uint64_t n_groups = (n_tiles + SF_TILES_PER_GROUP - 1) / SF_TILES_PER_GROUP;
   for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
      const uint64_t tile0 = g * SF_TILES_PER_GROUP;
      const uint64_t tile1 = tile0 + SF_TILES_PER_GROUP < n_tiles ? tile0 + SF_TILES_PER_GROUP : n_tiles;
      // the row r with offs[r] <= first byte < offs[r + 1]: offs[0] = 0 and offs[n] = total > first byte, so 0 <= r < n
      uint64_t r;
      {
         const int64_t first = (int64_t) (tile0 * SF_TILE);
         uint64_t lo = 0, hi = n; // the first index in [0, n] whose offset is > first
         while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (offs[mid] > first) hi = mid;
            else lo = mid + 1;
         }
         r = lo - 1;
      }
      for (uint64_t tile = tile0; tile < tile1; tile++) {
         const int64_t tb = (int64_t) (tile * SF_TILE);
         const int64_t te = tb + SF_TILE < (int64_t) total ? tb + SF_TILE : (int64_t) total;
         const int64_t w0 = tb + (int64_t) tid * SF_WORD;
         const int64_t w1 = w0 + SF_WORD < te ? w0 + SF_WORD : te;
         u128 acc = 0;
         uint64_t rc = r; // first row of the staged chunk: offs[rc] <= tb
         uint32_t cnt;
         for (;;) {
            cnt = (uint32_t) (n - rc < SF_LDS_ROWS ? n - rc : SF_LDS_ROWS); // rows rc … rc + cnt - 1, offsets rc … rc + cnt; cnt >= 1
            __syncthreads(); // the readers of the previous chunk are done
            for (uint32_t k = tid; k <= cnt; k += SF_BLOCK) s_off[k] = offs[rc + k];
            __syncthreads();
            const int64_t c_lo = s_off[0], c_hi = s_off[cnt];
            int64_t b = w0 > c_lo ? w0 : c_lo;
            const int64_t e = w1 < c_hi ? w1 : c_hi;
            if (b < e) {
               uint32_t lo = 0, hi = cnt; // the first staged index whose offset is > b (s_off[0] <= b < s_off[cnt])
               while (lo < hi) {
                  const uint32_t mid = (lo + hi) >> 1;
                  if (s_off[mid] > b) hi = mid;
                  else lo = mid + 1;
               }
               uint32_t j = lo - 1;
               while (b < e) {
                  while (s_off[j + 1] <= b) j++; // rows that ended before b (empty and NULL rows among them); stops: b < s_off[cnt]
                  const uint64_t i = rc + j;
                  uint32_t q = (uint32_t) (b - s_off[j]); // byte of the row
                  uint32_t pend = 0;
                  const int64_t b_was = b;
                  for (int k = 0; k < d.n_parts && b < e; k++) {
                     bool ok = true;
                     uint32_t u0, u1;
                     const uint32_t pbeg = pend;
                     pend += d_part_len(d.p[k], i, n, aux, &ok, &u0, &u1);
                     if (q >= pend) continue;
                     const uint32_t left = pend - q;
                     const uint32_t seg = (int64_t) left < e - b ? left : (uint32_t) (e - b);
                     acc |= d_part_bytes(d, d.p[k], i, n, aux, q - pbeg, seg) << (8 * (uint32_t) (b - w0));
                     b += seg;
                     q += seg;
                  }
                  if (b == b_was) break; // (cannot happen: the offsets are the sums of these lengths; never spin)
               }
            }
            if (c_hi >= te || rc + cnt >= n) break; // (uniform)
            rc += cnt;
         }
         if (w0 < te) {
            if (w0 + SF_WORD <= te) {
               *(u128*) (out + w0) = acc;
            } else {
               for (int64_t k = w0; k < te; k++) out[k] = (uint8_t) (acc >> (8 * (uint32_t) (k - w0)));
            }
         }
         // the next tile starts in the last staged row whose offset is <= te (the row that holds byte te, or an empty one at te)
         {
            uint32_t lo = 0, hi = cnt + 1; // the first staged index in [0, cnt] whose offset is > te, cnt + 1 if none
            while (lo < hi) {
               const uint32_t mid = (lo + hi) >> 1;
               if (s_off[mid] > te) hi = mid;
               else lo = mid + 1;
            }
            r = rc + lo - 1; // lo >= 1: s_off[0] <= tb < te
            if (r >= n) r = n - 1; // (te == total: the group ends here)
         }
      }
   }
}

// StringRuntime::len: bytes that are not continuation bytes, eight at a time (bit 7 set and bit 6 clear → popcount)
__global__ __launch_bounds__(256) void k_strlen(DCol col, uint64_t n, int64_t* __restrict__ out, uint64_t* __restrict__ valid_words) {
   const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
   const uint32_t lane = d_lane_id();
   const uint64_t high = 0x8080808080808080ull;
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i - lane < n; i += stride) {
      const bool in = i < n;
      bool ok = false;
      if (in) {
         const uint32_t row = d_phys_row(col, i);
         ok = d_valid(col, row);
         int64_t chars = 0;
         if (ok) {
            uint32_t len;
            const uint8_t* s = d_load_str(col, row, &len);
            uint32_t cont = 0, k = 0;
            for (; k + 8 <= len; k += 8) {
               const uint64_t x = *(const LDB_GLOBAL sf_u64_unaligned*) (s + k);
               cont += (uint32_t) __builtin_popcountll(x & ~(x << 1) & high);
            }
            for (; k < len; k++) cont += (s[k] >> 6) == 2 ? 1u : 0u;
            chars = (int64_t) (len - cont);
         }
         out[i] = chars;
      }
      if (valid_words) {
         const uint64_t word = __ballot(ok);
         if (lane == 0 && in) valid_words[i >> 6] = word;
      }
   }
}

static const ldb_column* strfn_column(const ldb_rel* r, ldb_colref ref) { // (after ldb_make_dcol has accepted ref)
   return &r->sides[(size_t) ref.side].table->cols[(size_t) ref.col];
}

extern "C" int32_t ldb_gpu_map_strcat(ldb_ctx* ctx, ldb_rel* in, const ldb_strpart* parts, int32_t n_parts, const char* name, ldb_table** out) {
   if (!ctx || !in || !parts || !out) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: NULL argument");
   if (n_parts < 1 || n_parts > LDB_MAX_STRPARTS) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_strcat: %d parts (1 to LDB_MAX_STRPARTS = %d)", n_parts, LDB_MAX_STRPARTS);
   // the arguments alone first: a refused call does no work (no lazy column is written out for it)
   for (int32_t k = 0; k < n_parts; k++) {
      const ldb_strpart& p = parts[k];
      if (p.kind < LDB_SP_COL || p.kind > LDB_SP_DATE) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: unknown kind %d", k, p.kind);
      if (p.strcase != LDB_SC_NONE && p.strcase != LDB_SC_UPPER && p.strcase != LDB_SC_LOWER) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: unknown strcase %d", k, p.strcase);
      if (p.kind != LDB_SP_COL) {
         const char* what = p.kind == LDB_SP_CONST ? "constant" : p.kind == LDB_SP_INT ? "integer" : p.kind == LDB_SP_DECIMAL ? "decimal" : "date";
         if (p.strcase != LDB_SC_NONE) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: a case mapping on a %s part (column parts only)", k, what);
         const bool no_window = (p.from == 0 && p.for_len == 0) || (p.from == 1 && p.for_len == LDB_STR_WHOLE);
         if (!no_window) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: a window on a %s part (column parts only)", k, what);
      }
      if (p.kind == LDB_SP_CONST && (p.str_len < 0 || p.str_len > (int64_t) UINT32_MAX || (p.str_len > 0 && !p.str))) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: bad constant (%lld bytes)", k, (long long) p.str_len);
   }
   LDB_TRY(ldb_rel_force(ctx, in));
   const int64_t n = in->n_rows;
   if (n > (int64_t) UINT32_MAX) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_strcat: %lld rows (at most 2^32 - 1)", (long long) n);
   DStrcat d;
   memset(&d, 0, sizeof(d));
   d.n_parts = n_parts;
   std::string consts;
   int n_windowed = 0;
   bool nullable = false;
   for (int32_t k = 0; k < n_parts; k++) {
      const ldb_strpart& p = parts[k];
      DSPart& q = d.p[k];
      q.kind = p.kind;
      q.strcase = p.strcase;
      if (p.kind == LDB_SP_CONST) {
         q.const_off = consts.size();
         q.const_len = (uint32_t) p.str_len;
         consts.append(p.str ? p.str : "", (size_t) p.str_len);
         continue;
      }
      // (the type is looked at before ldb_make_dcol: a refused part does not get a lazy column's strings written)
      if (p.col.side >= 0 && (size_t) p.col.side < in->sides.size() && p.col.col >= 0 && (size_t) p.col.col < in->sides[(size_t) p.col.side].table->cols.size()) {
         const int t = strfn_column(in, p.col)->type.type;
         if (p.kind == LDB_SP_COL && t != LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: a utf8 column expected (type %d)", k, t);
         if (p.kind == LDB_SP_INT && t != LDB_T_INT32 && t != LDB_T_INT64) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: an int32 / int64 column expected (type %d)", k, t);
         if (p.kind == LDB_SP_DECIMAL && t != LDB_T_DECIMAL128) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: a decimal128 column expected (type %d)", k, t);
         if (p.kind == LDB_SP_DATE && t != LDB_T_DATE32) LDB_FAIL(LDB_ERR_INVALID, "map_strcat: part %d: a date32 column expected (type %d)", k, t);
      }
      LDB_TRY(ldb_make_dcol(in, p.col, &q.col));
      nullable = nullable || q.col.validity || q.col.rowids || p.kind == LDB_SP_DATE; // (a day outside 0001 … 9999 is NULL)
      if (p.kind == LDB_SP_COL) {
         q.src_bytes = (uint64_t) std::max<int64_t>(0, strfn_column(in, p.col)->value_bytes);
         q.windowed = !(p.from == 1 && p.for_len == LDB_STR_WHOLE);
         if (q.windowed) {
            q.widx = n_windowed++;
            // (no string has 2^62 characters: clamped so that from + for_len cannot overflow in d_substr_range)
            const int64_t lim = (int64_t) 1 << 61;
            q.from = std::min(std::max(p.from, -lim), lim);
            q.for_len = std::min(p.for_len, lim);
         }
      }
   }
   d.nullable = nullable ? 1 : 0;
   LdbBufs tmp(ctx);
   uint8_t* d_consts = nullptr;
   if (!consts.empty()) { // the constants' bytes in one device buffer
      LDB_TRY(ldb_dev_upload(ctx, consts.data(), consts.size(), (void**) &d_consts, false));
      tmp.adopt(d_consts);
      d.consts = (uint64_t) d_consts;
      for (int32_t k = 0; k < n_parts; k++)
         if (d.p[k].kind == LDB_SP_CONST) d.p[k].src_bytes = consts.size();
   }
   const int grid = ldb_grid_for(ctx, n, 256, 8);
   int64_t* lens;
   uint32_t* aux = nullptr;
   LDB_TRY(tmp.alloc(&lens, 8 * (size_t) (n + 1)));
   if (n_windowed) LDB_TRY(tmp.alloc(&aux, 4 * (size_t) 2 * n_windowed * (size_t) (n ? n : 1)));
   ldb_coltype t = {LDB_T_UTF8, 0, 0, nullable ? 1 : 0};
   const char* nm = name ? name : "strcat";
   uint64_t* valid_words = nullptr;
   if (nullable) LDB_TRY(tmp.alloc(&valid_words, 8 * (size_t) ((n + 63) / 64 + 1)));
   if (n) {
      LdbProf prof_(ctx, "k_strcat_lens");
      hipLaunchKernelGGL(k_strcat_lens, dim3(grid), dim3(256), 0, ctx->stream, d, (uint64_t) n, lens, aux, valid_words);
   }
   int64_t* offs;
   LDB_TRY(tmp.alloc(&offs, 8 * (size_t) (n + 1)));
   LDB_TRY(ldb_exclusive_scan_i64(ctx, lens, offs, n, offs + n));
   uint64_t total = 0;
   LDB_TRY(ldb_read_u64(ctx, offs + n, &total));
   tmp.free(lens);
   const int64_t cap = (int64_t) total;
   LdbTableHold res(ctx);
   LDB_TRY(ldb_gpu_table_alloc(ctx, "mapped", 1, &t, &nm, n, &cap, 0, &res.t));
   LDB_HIP(hipMemcpyAsync(res->cols[0].offsets, offs, 8 * (size_t) (n + 1), hipMemcpyDeviceToDevice, ctx->stream));
   res->cols[0].value_bytes = cap;
   if (n && total) {
      const uint64_t n_tiles = (total + SF_TILE - 1) / SF_TILE;
      const int fgrid = ldb_grid_for(ctx, (int64_t) ((n_tiles + SF_TILES_PER_GROUP - 1) / SF_TILES_PER_GROUP), 1, 8);
      LdbProf prof_(ctx, "k_strcat_fill");
      hipLaunchKernelGGL(k_strcat_fill, dim3(fgrid), dim3(SF_BLOCK), 0, ctx->stream, d, (uint64_t) n, (const int64_t*) offs, (const uint32_t*) aux, (uint8_t*) res->cols[0].values, total);
   }
   if (nullable) { // the bitmap the length kernel wrote becomes the column's
      if (res->cols[0].validity) LdbBufs::drop(ctx, &res->cols[0].validity);
      tmp.keep(valid_words);
      res->cols[0].validity = (uint8_t*) valid_words;
      res->cols[0].null_count = -1;
   }
   LDB_HIP(hipGetLastError());
   *out = res.release();
   return LDB_OK;
}

extern "C" int32_t ldb_gpu_map_strlen(ldb_ctx* ctx, ldb_rel* in, ldb_colref col, const char* name, ldb_table** out) {
   if (!ctx || !in || !out) LDB_FAIL(LDB_ERR_INVALID, "map_strlen: NULL argument");
   LDB_TRY(ldb_rel_force(ctx, in));
   if (col.side >= 0 && (size_t) col.side < in->sides.size() && col.col >= 0 && (size_t) col.col < in->sides[(size_t) col.side].table->cols.size() &&
       strfn_column(in, col)->type.type != LDB_T_UTF8)
      LDB_FAIL(LDB_ERR_INVALID, "map_strlen: utf8 column expected (type %d)", strfn_column(in, col)->type.type);
   DCol dc;
   LDB_TRY(ldb_make_dcol(in, col, &dc));
   if (dc.type != LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "map_strlen: utf8 column expected");
   const int64_t n = in->n_rows;
   if (n > (int64_t) UINT32_MAX) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_strlen: %lld rows (at most 2^32 - 1)", (long long) n);
   const bool nullable = dc.validity || dc.rowids;
   ldb_coltype t = {LDB_T_INT64, 0, 0, nullable ? 1 : 0};
   const char* nm = name ? name : "length";
   LdbTableHold res(ctx);
   LDB_TRY(ldb_gpu_table_alloc(ctx, "mapped", 1, &t, &nm, n, nullptr, 0, &res.t));
   uint64_t* valid_words = nullptr;
   if (nullable) {
      if (res->cols[0].validity) LdbBufs::drop(ctx, &res->cols[0].validity);
      LDB_TRY(LdbBufs::alloc_into(ctx, &res->cols[0].validity, 8 * (size_t) ((n + 63) / 64 + 1)));
      valid_words = (uint64_t*) res->cols[0].validity;
      res->cols[0].null_count = -1;
   }
   if (n) {
      const int grid = ldb_grid_for(ctx, n, 256, 8);
      LdbProf prof_(ctx, "k_strlen");
      hipLaunchKernelGGL(k_strlen, dim3(grid), dim3(256), 0, ctx->stream, dc, (uint64_t) n, (int64_t*) res->cols[0].values, valid_words);
   }
   LDB_HIP(hipGetLastError());
   *out = res.release();
   return LDB_OK;
}
