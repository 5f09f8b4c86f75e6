// ldb_colstats.hip — per-column statistics, computed on first use and cached in the column: value range, zone map, sortedness.
#include "ldb_internal.h"
#include "ldb_device.h"
#include <algorithm>

// ---------------------------------------------------------------- column statistics
__global__ void k_column_range(DCol col, uint64_t n, long long* __restrict__ out) {
   long long lo = 0x7FFFFFFFFFFFFFFFll, hi = -0x7FFFFFFFFFFFFFFFll - 1;
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
      long long k = d_load_i64(col, (uint32_t) i);
      lo = k < lo ? k : lo;
      hi = k > hi ? k : hi;
   }
   for (int off = 32; off > 0; off >>= 1) {
      long long l2 = __shfl_down(lo, off), h2 = __shfl_down(hi, off);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
   }
   if ((threadIdx.x & 63) == 0) {
      atomicMin(&out[0], lo);
      atomicMax(&out[1], hi);
   }
}
int32_t ldb_column_range(ldb_ctx* ctx, const ldb_table* t, int32_t col, int64_t* lo, int64_t* hi) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "column_range: bad column %d", col);
   const ldb_column& c = t->cols[(size_t) col];
   const int ty = c.type.type;
   const bool ok = ty == LDB_T_INT8 || ty == LDB_T_INT16 || ty == LDB_T_INT32 || ty == LDB_T_INT64 || ty == LDB_T_DATE32 ||
                   (ty == LDB_T_DECIMAL128 && c.type.precision < 19);
   if (!ok) return LDB_ERR_UNSUPPORTED;
   if (!c.has_range) {
      long long* d_out = (long long*) (ctx->d_scratch + LDB_SCRATCH_COLUMN_RANGE);
      const long long init[2] = {INT64_MAX, INT64_MIN};
      long long got[2] = {0, -1};
      if (t->n_rows > 0) {
         DCol dc;
         memset(&dc, 0, sizeof(dc));
         dc.values = (uint64_t) c.values;
         dc.type = ty;
         dc.width = c.width;
         dc.precision = c.type.precision;
         dc.scale = c.type.scale;
         LDB_TRY(ldb_h2d_small(ctx, d_out, init, 16)); // (pinned staging: a pageable source makes the copy wait for the stream)
         hipLaunchKernelGGL(k_column_range, dim3(ldb_grid_for(ctx, t->n_rows, 256, 8)), dim3(256), 0, ctx->stream, dc, (uint64_t) t->n_rows, d_out);
         LDB_TRY(LDB_READBACK(ctx, got, d_out, 16));
      }
      c.vmin = got[0];
      c.vmax = got[1];
      c.has_range = true;
   }
   *lo = c.vmin;
   *hi = c.vmax;
   return LDB_OK;
}

// one workgroup per zone of LDB_ZONE_ROWS rows
__global__ __launch_bounds__(256) void k_column_zones(DCol col, uint64_t n, int64_t* __restrict__ zmin, int64_t* __restrict__ zmax) {
   __shared__ int64_t s_lo[4], s_hi[4];
   const uint64_t b = (uint64_t) blockIdx.x << LDB_ZONE_SHIFT, e = b + LDB_ZONE_ROWS < n ? b + LDB_ZONE_ROWS : n;
   int64_t lo = INT64_MAX, hi = INT64_MIN;
   for (uint64_t i = b + threadIdx.x; i < e; i += 256) {
      const int64_t v = d_load_i64(col, (uint32_t) i);
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
   }
   for (int o = 32; o > 0; o >>= 1) {
      const int64_t l2 = __shfl_xor((long long) lo, o), h2 = __shfl_xor((long long) hi, o);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
   }
   if ((threadIdx.x & 63) == 0) {
      s_lo[threadIdx.x >> 6] = lo;
      s_hi[threadIdx.x >> 6] = hi;
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int k = 1; k < 4; k++) {
         lo = s_lo[k] < lo ? s_lo[k] : lo;
         hi = s_hi[k] > hi ? s_hi[k] : hi;
      }
      zmin[blockIdx.x] = lo;
      zmax[blockIdx.x] = hi;
   }
}
int32_t ldb_column_zones(ldb_ctx* ctx, const ldb_table* t, int32_t col, uint64_t* zmin, uint64_t* zmax) {
   *zmin = *zmax = 0;
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "column_zones: bad column %d", col);
   const ldb_column& c = t->cols[(size_t) col];
   const int ty = c.type.type;
   const bool ok = ty == LDB_T_INT8 || ty == LDB_T_INT16 || ty == LDB_T_INT32 || ty == LDB_T_INT64 || ty == LDB_T_DATE32 || (ty == LDB_T_DECIMAL128 && c.type.precision < 19 && c.width == 8);
   if (!ok || !c.owned || c.validity || t->n_rows < 2 * (int64_t) LDB_ZONE_ROWS) return LDB_OK; // (views share their owner's values: no statistics of their own)
   if (c.zone_state < 0) {
      const int64_t nz = (t->n_rows + LDB_ZONE_ROWS - 1) >> LDB_ZONE_SHIFT;
      int64_t *zl, *zh;
      LdbBufs tmp(ctx); // (freed on the error returns below)
      LDB_TRY(tmp.alloc(&zl, 8 * (size_t) nz));
      LDB_TRY(tmp.alloc(&zh, 8 * (size_t) nz));
      DCol dc;
      memset(&dc, 0, sizeof(dc));
      dc.values = (uint64_t) c.values;
      dc.type = ty;
      dc.width = c.width;
      dc.precision = c.type.precision;
      dc.scale = c.type.scale;
      hipLaunchKernelGGL(k_column_zones, dim3((unsigned) nz), dim3(256), 0, ctx->stream, dc, (uint64_t) t->n_rows, zl, zh);
      std::vector<int64_t> hl((size_t) nz), hh((size_t) nz);
      LDB_HIP(hipMemcpyAsync(hl.data(), zl, 8 * (size_t) nz, hipMemcpyDeviceToHost, ctx->stream));
      LDB_HIP(hipMemcpyAsync(hh.data(), zh, 8 * (size_t) nz, hipMemcpyDeviceToHost, ctx->stream));
      LDB_HIP(hipStreamSynchronize(ctx->stream));
      // selective? the zones together must cover well under the whole value range (sorted / clustered columns do; a
      // uniformly scattered column has every zone span the full range and a zone test could never exclude anything)
      int64_t gl = INT64_MAX, gh = INT64_MIN;
      long double span = 0;
      for (int64_t z = 0; z < nz; z++) {
         gl = std::min(gl, hl[(size_t) z]);
         gh = std::max(gh, hh[(size_t) z]);
         span += (long double) hh[(size_t) z] - (long double) hl[(size_t) z];
      }
      const long double full = ((long double) gh - (long double) gl) * (long double) nz;
      const bool useful = full > 0 && span < 0.5L * full;
      if (useful) {
         c.zone_min = zl;
         c.zone_max = zh;
         tmp.keep(zl);
         tmp.keep(zh);
      }
      c.zone_state = useful ? 1 : 0;
   }
   if (c.zone_state == 1) {
      *zmin = (uint64_t) c.zone_min;
      *zmax = (uint64_t) c.zone_max;
   }
   return LDB_OK;
}

extern "C" int64_t ldb_gpu_table_zones(ldb_ctx* ctx, const ldb_table* t, int32_t col) {
   uint64_t a = 0, b = 0;
   if (!ctx || ldb_column_zones(ctx, t, col, &a, &b) != LDB_OK) return -1;
   return a ? (t->n_rows + LDB_ZONE_ROWS - 1) >> LDB_ZONE_SHIFT : 0;
}
__global__ void k_column_sorted(DCol col, uint64_t n, unsigned int* __restrict__ unsorted) {
   bool bad = false;
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x + 1; i < n; i += (uint64_t) gridDim.x * blockDim.x)
      bad = bad || d_load_i64(col, (uint32_t) i) < d_load_i64(col, (uint32_t) (i - 1));
   if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(unsorted, 1u);
}
int32_t ldb_column_sorted(ldb_ctx* ctx, const ldb_table* t, int32_t col, bool* sorted) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "column_sorted: bad column %d", col);
   const ldb_column& c = t->cols[(size_t) col];
   const int ty = c.type.type;
   const bool ok = ty == LDB_T_INT8 || ty == LDB_T_INT16 || ty == LDB_T_INT32 || ty == LDB_T_INT64 || ty == LDB_T_DATE32 ||
                   (ty == LDB_T_DECIMAL128 && c.type.precision < 19);
   if (c.sorted_state < 0) {
      if (!ok || c.validity) {
         c.sorted_state = 0;
      } else if (t->n_rows < 2) {
         c.sorted_state = 1;
      } else {
         DCol dc;
         memset(&dc, 0, sizeof(dc));
         dc.values = (uint64_t) c.values;
         dc.type = ty;
         dc.width = c.width;
         dc.precision = c.type.precision;
         dc.scale = c.type.scale;
         unsigned int* d_flag = (unsigned int*) (ctx->d_scratch + LDB_SCRATCH_COLUMN_SORTED);
         LDB_HIP(hipMemsetAsync(d_flag, 0, 8, ctx->stream));
         hipLaunchKernelGGL(k_column_sorted, dim3(ldb_grid_for(ctx, t->n_rows, 256, 8)), dim3(256), 0, ctx->stream, dc, (uint64_t) t->n_rows, d_flag);
         uint64_t f = 0;
         LDB_TRY(ldb_read_u64(ctx, d_flag, &f));
         c.sorted_state = (f & 1) ? 0 : 1;
      }
   }
   *sorted = c.sorted_state == 1;
   return LDB_OK;
}
