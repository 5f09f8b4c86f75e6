// ldb_strcast.hip — a utf8 column parsed as INT64 / DECIMAL128(p, s) / DATE32: cast(col as int | decimal | date).
// Replaces (reference): StringRuntime::toInt (src/runtime/StringRuntime.cpp:174-185: std::stoll that must consume the whole
// string), toDecimal (:187-200: arrow's Decimal128::FromString, then Rescale) and toDate (:439-444: arrow's
// ParseValue<Date32Type>), which the generated code calls per tuple.  Where the reference throws or leaves its result
// undefined the row is BAD here: NULL, and counted.  The parsers themselves are in ldb_strcast.h; the other direction
// (numbers and dates as text) is the INT / DECIMAL / DATE part of ldb_gpu_map_strcat (ldb_strfn.hip).
#include "ldb_internal.h"
#include "ldb_strcast.h"

// One row per lane on the scheme of k_strlen: thread t of the grid takes rows t, t + T, … (T a multiple of 64), so a wave
// holds 64 consecutive rows from a multiple of 64 = one word of the validity bitmap, written from one ballot; the bad rows
// of a wave are counted from a second ballot and added by one lane.  A lane reads its string eight bytes at a time and stops
// at the first byte that makes it bad; a string of another length than 10 is no date without a load.  Known limit, shared
// with k_strlen: a pathologically long VALID text (megabytes of leading zeros or blanks) serialises its wave.
__global__ __launch_bounds__(256) void k_strparse(DCol col, uint64_t n, uint64_t value_bytes, int32_t kind, int32_t precision, int32_t scale, int32_t out_width, uint8_t* __restrict__ out,
                                                  uint64_t* __restrict__ valid_words, unsigned long long* __restrict__ n_bad) {
   const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
   const uint32_t lane = d_lane_id();
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i - lane < n; i += stride) {
      const bool in = i < n;
      bool ok = false, bad = false;
      if (in) {
         const uint32_t row = d_phys_row(col, i);
         i128 v = 0;
         if (d_valid(col, row)) {
            const int64_t* o = gptr<int64_t>(col.offsets);
            const uint64_t at = (uint64_t) o[row];
            const uint32_t len = (uint32_t) ((uint64_t) o[row + 1] - at);
            const uint8_t* base = gptr<uint8_t>(col.values);
            if (kind == LDB_PARSE_INT64) {
               int64_t x = 0;
               ok = d_parse_int64(base, at, len, value_bytes, &x);
               v = x;
            } else if (kind == LDB_PARSE_DECIMAL) {
               ok = d_parse_decimal(base, at, len, value_bytes, precision, scale, &v);
            } else {
               int32_t x = 0;
               ok = d_parse_date(base, at, len, value_bytes, &x);
               v = x;
            }
            bad = !ok;
            if (!ok) v = 0;
         }
         if (out_width == 16) {
            uint64_t* p = (uint64_t*) out + 2 * i;
            p[0] = (uint64_t) v;
            p[1] = (uint64_t) ((u128) v >> 64);
         } else if (out_width == 8) {
            ((int64_t*) out)[i] = (int64_t) v;
         } else {
            ((int32_t*) out)[i] = (int32_t) v;
         }
      }
      const uint64_t word = __ballot(ok), bad_word = __ballot(bad);
      if (lane == 0) { // (i < n in lane 0 of every wave that is here)
         valid_words[i >> 6] = word;
         if (bad_word) atomicAdd(n_bad, (unsigned long long) __builtin_popcountll(bad_word));
      }
   }
}

extern "C" int32_t ldb_gpu_map_strparse(ldb_ctx* ctx, ldb_rel* in, ldb_colref col, int32_t kind, int32_t precision, int32_t scale, const char* name, ldb_table** out, int64_t* n_bad) {
   if (!ctx || !in || !out) LDB_FAIL(LDB_ERR_INVALID, "map_strparse: NULL argument");
   // the arguments alone first: a refused call does no work
   if (kind != LDB_PARSE_INT64 && kind != LDB_PARSE_DECIMAL && kind != LDB_PARSE_DATE) LDB_FAIL(LDB_ERR_INVALID, "map_strparse: unknown kind %d", kind);
   if (kind == LDB_PARSE_DECIMAL) {
      if (precision < 1 || precision > 38) LDB_FAIL(LDB_ERR_INVALID, "map_strparse: precision %d (1 to 38)", precision);
      if (scale < 0 || scale > precision) LDB_FAIL(LDB_ERR_INVALID, "map_strparse: scale %d (0 to the precision, %d)", scale, precision);
   }
   LDB_TRY(ldb_rel_force(ctx, in));
   const bool ref_ok = col.side >= 0 && (size_t) col.side < in->sides.size() && col.col >= 0 && (size_t) col.col < in->sides[(size_t) col.side].table->cols.size();
   if (ref_ok && in->sides[(size_t) col.side].table->cols[(size_t) col.col].type.type != LDB_T_UTF8)
      LDB_FAIL(LDB_ERR_INVALID, "map_strparse: utf8 column expected (type %d)", in->sides[(size_t) col.side].table->cols[(size_t) col.col].type.type);
   DCol dc;
   LDB_TRY(ldb_make_dcol(in, col, &dc));
   if (dc.type != LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "map_strparse: utf8 column expected");
   const uint64_t value_bytes = (uint64_t) std::max<int64_t>(0, in->sides[(size_t) col.side].table->cols[(size_t) col.col].value_bytes);
   const int64_t n = in->n_rows;
   if (n > (int64_t) UINT32_MAX) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_strparse: %lld rows (at most 2^32 - 1)", (long long) n);
   ldb_coltype t = {LDB_T_INT64, 0, 0, 1};
   if (kind == LDB_PARSE_DECIMAL) t = {LDB_T_DECIMAL128, precision, scale, 1};
   if (kind == LDB_PARSE_DATE) t = {LDB_T_DATE32, 0, 0, 1};
   const char* nm = name ? name : "parsed";
   LdbTableHold res(ctx);
   LDB_TRY(ldb_gpu_table_alloc(ctx, "mapped", 1, &t, &nm, n, nullptr, 0, &res.t));
   const int32_t width = res->cols[0].width;
   if (width != 4 && width != 8 && width != 16) LDB_FAIL(LDB_ERR_INVALID, "map_strparse: result column of %d bytes per value", width);
   if (res->cols[0].validity) LdbBufs::drop(ctx, &res->cols[0].validity);
   LDB_TRY(LdbBufs::alloc_into(ctx, &res->cols[0].validity, 8 * (size_t) ((n + 63) / 64 + 1)));
   res->cols[0].null_count = -1;
   LdbBufs tmp(ctx);
   unsigned long long* d_bad;
   LDB_TRY(tmp.alloc(&d_bad, 8));
   LDB_HIP(hipMemsetAsync(d_bad, 0, 8, ctx->stream));
   if (n) {
      const int grid = ldb_grid_for(ctx, n, 256, 8);
      LdbProf prof_(ctx, "k_strparse");
      hipLaunchKernelGGL(k_strparse, dim3(grid), dim3(256), 0, ctx->stream, dc, (uint64_t) n, value_bytes, kind, precision, scale, width, (uint8_t*) res->cols[0].values, (uint64_t*) res->cols[0].validity, d_bad);
   }
   LDB_HIP(hipGetLastError());
   if (n_bad) {
      uint64_t bad = 0;
      LDB_TRY(ldb_read_u64(ctx, d_bad, &bad));
      *n_bad = (int64_t) bad;
   }
   *out = res.release();
   return LDB_OK;
}
