// ldb_datefn.hip — date and time functions as computed columns: extract(part), date_trunc(part), date ± interval month.
// Replaces (reference): DateRuntime::extractYear … extractSecond (src/runtime/DateRuntime.cpp:99-116), dateTrunc (:117-164)
// and addMonths / subtractMonths (:77-82 over DateHelper::addMonths :35-40), which the generated code calls per tuple
// (RuntimeFunctions.cpp:316-330).  The calendar arithmetic is in ldb_datefn.h; the semantics are stated at
// ldb_gpu_map_datefn in lingodb_gpu.h.  date_diff is SUB / SDIV of the expression programs (ldb_plan_expr.cpp).
#include "ldb_internal.h"
#include "ldb_datefn.h"

// IW = bytes of the column's TYPE (4: date32 days, 8: int64 ns), FN / PART compile-time: no per-row switch
template <int IW, int FN, int PART>
__device__ __forceinline__ int64_t d_datefn(int64_t x) { // EXTRACT and TRUNC: defined for every input
   if (FN == LDB_DF_EXTRACT) return IW == 4 ? d_extract_day<PART>((int32_t) x) : d_extract_ns<PART>(x);
   return IW == 4 ? (int64_t) d_trunc_day<PART>((int32_t) x) : d_trunc_ns<PART>(x);
}

// 16 bytes of a column whose base is only known to be aligned to its values: the compiler still emits one dwordx4 access
// (global memory takes it at any dword address), so a base that is not 16-byte aligned needs no scalar head — only the
// n mod 4 rows of the tail are left over
struct __attribute__((packed, aligned(4))) DVec4i {
   int32_t v[4];
};
struct __attribute__((packed, aligned(8))) DVec2l {
   int64_t v[2];
};

// Dense path (no row ids, device width = the type's): a lane takes 4 consecutive rows per step with 16-byte loads and
// stores; validity is not looked at — NULL slots are computed like any other (every input is defined) and the result's
// bitmap is the input's, copied by the host on the stream.  The last n mod 4 rows go to the first lanes of the grid.
template <int IW, int FN, int PART>
__global__ __launch_bounds__(256) void k_datefn_dense(uint64_t in, uint64_t out, uint64_t n) {
   constexpr int OW = FN == LDB_DF_EXTRACT ? 8 : IW;
   const uint64_t n4 = n >> 2, stride = (uint64_t) gridDim.x * blockDim.x, gid = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x;
   for (uint64_t g = gid; g < n4; g += stride) {
      int64_t x[4], r[4];
      if (IW == 4) {
         const DVec4i v = gptr<DVec4i>(in)[g];
#pragma unroll
         for (int k = 0; k < 4; k++) x[k] = v.v[k];
      } else {
         const DVec2l a = gptr<DVec2l>(in)[2 * g], b = gptr<DVec2l>(in)[2 * g + 1];
         x[0] = a.v[0], x[1] = a.v[1], x[2] = b.v[0], x[3] = b.v[1];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] = d_datefn<IW, FN, PART>(x[k]);
      if (OW == 4) {
         DVec4i o;
#pragma unroll
         for (int k = 0; k < 4; k++) o.v[k] = (int32_t) r[k];
         gptr_mut<DVec4i>(out)[g] = o;
      } else {
         DVec2l a, b;
         a.v[0] = r[0], a.v[1] = r[1], b.v[0] = r[2], b.v[1] = r[3];
         gptr_mut<DVec2l>(out)[2 * g] = a;
         gptr_mut<DVec2l>(out)[2 * g + 1] = b;
      }
   }
   if (gid < (n & 3)) {
      const uint64_t i = 4 * n4 + gid;
      const int64_t x = IW == 4 ? (int64_t) gptr<int32_t>(in)[i] : gptr<int64_t>(in)[i];
      const int64_t r = d_datefn<IW, FN, PART>(x);
      if (OW == 4) gptr_mut<int32_t>(out)[i] = (int32_t) r;
      else gptr_mut<int64_t>(out)[i] = r;
   }
}

// General path (row ids, another device width, ADD_MONTHS): one row per lane on the scheme of k_strparse — thread t of the
// grid takes rows t, t + T, … (T a multiple of 64), so a wave holds 64 consecutive rows from a multiple of 64 = one word of
// the result's validity bitmap, written from one ballot with an ordinary vector store by lane 0.  valid_words == NULL: the
// result cannot hold a NULL and no bitmap is written.
template <int IW, int FN, int PART>
__global__ __launch_bounds__(256) void k_datefn_rows(DCol col, DCol mcol, int32_t has_mcol, int64_t months, uint64_t n, uint64_t out, uint64_t* __restrict__ valid_words) {
   constexpr int OW = FN == LDB_DF_EXTRACT ? 8 : IW;
   const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
   const uint32_t lane = d_lane_id();
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i - lane < n; i += stride) {
      bool ok = false;
      if (i < n) {
         const uint32_t row = d_phys_row(col, i);
         ok = d_valid(col, row);
         int64_t r = 0;
         if (FN == LDB_DF_ADD_MONTHS) {
            int64_t m = months;
            if (ok && has_mcol) {
               const uint32_t mrow = d_phys_row(mcol, i);
               ok = d_valid(mcol, mrow);
               if (ok) m = d_load_i64(mcol, mrow);
            }
            if (ok) {
               const int64_t x = d_load_i64(col, row);
               if (IW == 4) {
                  int32_t d = 0;
                  ok = d_add_months_day((int32_t) x, m, &d);
                  r = d;
               } else {
                  ok = d_add_months_ns(x, m, &r);
               }
               if (!ok) r = 0;
            }
         } else if (ok) {
            r = d_datefn<IW, FN, PART>(d_load_i64(col, row));
         }
         if (OW == 4) gptr_mut<int32_t>(out)[i] = (int32_t) r;
         else gptr_mut<int64_t>(out)[i] = r;
      }
      if (valid_words) { // (uniform over the grid)
         const uint64_t word = __ballot(ok);
         if (lane == 0) valid_words[i >> 6] = word; // (i < n in lane 0 of every wave that is here)
      }
   }
}

namespace {
struct DatefnLaunch {
   ldb_ctx* ctx;
   bool dense;
   int grid;
   DCol col, mcol;
   int32_t has_mcol;
   int64_t months;
   uint64_t n, out;
   uint64_t* valid_words;
   template <int IW, int FN, int PART>
   void go() const {
      if (dense) {
         LdbProf prof_(ctx, "k_datefn_dense");
         hipLaunchKernelGGL((k_datefn_dense<IW, FN, PART>), dim3(grid), dim3(256), 0, ctx->stream, col.values, out, n);
      } else {
         LdbProf prof_(ctx, "k_datefn_rows");
         hipLaunchKernelGGL((k_datefn_rows<IW, FN, PART>), dim3(grid), dim3(256), 0, ctx->stream, col, mcol, has_mcol, months, n, out, valid_words);
      }
   }
   template <int IW, int FN>
   void by_part(int32_t part) const {
      switch (part) {
         case LDB_DP_YEAR: return go<IW, FN, LDB_DP_YEAR>();
         case LDB_DP_MONTH: return go<IW, FN, LDB_DP_MONTH>();
         case LDB_DP_DAY: return go<IW, FN, LDB_DP_DAY>();
         case LDB_DP_HOUR: return go<IW, FN, LDB_DP_HOUR>();
         case LDB_DP_MINUTE: return go<IW, FN, LDB_DP_MINUTE>();
         default: return go<IW, FN, LDB_DP_SECOND>();
      }
   }
   template <int IW>
   void by_fn(int32_t fn, int32_t part) const {
      if (fn == LDB_DF_EXTRACT) return by_part<IW, LDB_DF_EXTRACT>(part);
      if (fn == LDB_DF_TRUNC) return by_part<IW, LDB_DF_TRUNC>(part);
      go<IW, LDB_DF_ADD_MONTHS, LDB_DP_YEAR>(); // (never dense)
   }
};
} // namespace

extern "C" int32_t ldb_gpu_map_datefn(ldb_ctx* ctx, ldb_rel* in, ldb_colref col, int32_t fn, int32_t part, int64_t months, const ldb_colref* months_col, const char* name, ldb_table** out) {
   if (!ctx || !in || !out) LDB_FAIL(LDB_ERR_INVALID, "map_datefn: NULL argument");
   // the arguments alone first: a refused call does no work
   if (fn != LDB_DF_EXTRACT && fn != LDB_DF_TRUNC && fn != LDB_DF_ADD_MONTHS) LDB_FAIL(LDB_ERR_INVALID, "map_datefn: unknown function %d", fn);
   const bool add = fn == LDB_DF_ADD_MONTHS;
   if (!add && (part < LDB_DP_YEAR || part > LDB_DP_SECOND)) LDB_FAIL(LDB_ERR_INVALID, "map_datefn: unknown part %d", part);
   LDB_TRY(ldb_rel_force(ctx, in));
   DatefnLaunch L{};
   LDB_TRY(ldb_make_dcol(in, col, &L.col));
   if (L.col.type != LDB_T_DATE32 && L.col.type != LDB_T_INT64) LDB_FAIL(LDB_ERR_INVALID, "map_datefn: date32 or int64 (ns since the epoch) column expected (type %d)", L.col.type);
   L.has_mcol = add && months_col ? 1 : 0;
   if (L.has_mcol) {
      LDB_TRY(ldb_make_dcol(in, *months_col, &L.mcol));
      if (L.mcol.type != LDB_T_INT32 && L.mcol.type != LDB_T_INT64) LDB_FAIL(LDB_ERR_INVALID, "map_datefn: int32 or int64 months column expected (type %d)", L.mcol.type);
   }
   const int64_t n = in->n_rows;
   if (n > (int64_t) UINT32_MAX) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_datefn: %lld rows (at most 2^32 - 1)", (long long) n);
   const bool is_date = L.col.type == LDB_T_DATE32;
   ldb_coltype t = {fn == LDB_DF_EXTRACT ? LDB_T_INT64 : (ldb_type) L.col.type, 0, 0, add ? 1 : 0};
   const char* nm = name ? name : "datefn";
   LdbTableHold res(ctx);
   LDB_TRY(ldb_gpu_table_alloc(ctx, "mapped", 1, &t, &nm, n, nullptr, 0, &res.t));
   ldb_column& rc = res->cols[0];
   if (rc.width != (fn == LDB_DF_EXTRACT || !is_date ? 8 : 4)) LDB_FAIL(LDB_ERR_INVALID, "map_datefn: result column of %d bytes per value", rc.width);
   const uintptr_t base = (uintptr_t) L.col.values;
   L.dense = !add && !L.col.rowids && L.col.width == (is_date ? 4 : 8) && base % (uintptr_t) L.col.width == 0;
   const bool nullable = add || L.col.validity || L.col.rowids;
   if (nullable) {
      LDB_TRY(LdbBufs::alloc_into(ctx, &rc.validity, 8 * (size_t) ((n + 63) / 64 + 1)));
      rc.null_count = -1; // unknown (Arrow convention)
   }
   L.ctx = ctx;
   L.months = months;
   L.n = (uint64_t) n;
   L.out = (uint64_t) rc.values;
   if (n) {
      if (L.dense) {
         L.grid = ldb_grid_for(ctx, (n + 3) / 4, 256, 8);
         if (nullable) { // NULL in → NULL out: the same bitmap
            LDB_HIP(hipMemcpyAsync(rc.validity, (const void*) L.col.validity, (size_t) ((n + 7) / 8), hipMemcpyDeviceToDevice, ctx->stream));
            rc.null_count = in->sides[(size_t) col.side].table->cols[(size_t) col.col].null_count;
         }
      } else {
         L.grid = ldb_grid_for(ctx, n, 256, 8);
         L.valid_words = (uint64_t*) rc.validity;
      }
      if (is_date) L.by_fn<4>(fn, part);
      else L.by_fn<8>(fn, part);
   }
   LDB_HIP(hipGetLastError());
   *out = res.release();
   return LDB_OK;
}
