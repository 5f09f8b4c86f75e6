// ldb_strminmax.hip — key-less MIN / MAX over utf8 columns: the last operator of every Join Order Benchmark plan
// (SELECT MIN(n.name), MIN(t.title) … with no GROUP BY).
// Replaces (reference): the generated reduce over a SimpleState (src/runtime/SimpleState.cpp:8-30) whose combine function
// calls StringRuntime::compareLt / compareGt (src/runtime/StringRuntime.cpp:240-248): std::string_view order — unsigned
// bytes first, then length.
//
// A string has no fixed-width accumulator, so the extreme is found in two launches that serve ALL string aggregates of a call:
//   1. prefix pass: every row gives an order-preserving 64-bit key — its first 8 bytes, big-endian, zero padded — reduced
//      with shuffles inside the wave, through LDS inside the workgroup and with ONE 64-bit atomicMax per workgroup on a
//      global word (MIN reduces the complemented key, so one zero-initialised word and one reduction serve both).  The
//      key is monotone but not strict (s < t ⇒ key(s) ≤ key(t); "ab" and "ab\0" share a key), so
//   2. resolve pass: only rows whose key equals the winning key are candidates.  A lane keeps the best of its own
//      candidates, the wave reduces its lanes' candidates against each other by full comparison (shuffle the row,
//      compare the bytes behind the shared prefix, then the lengths), and ONE lane per wave runs a compare-and-swap loop
//      on a global `best row + 1` word that replaces the stored row only by a STRICTLY better string.  Equal strings
//      never swap, so once the true extreme is stored every later candidate leaves after one comparison.  There is no
//      lock: a lane never waits for another lane of its wave (see d_sink_minmax128 in ldb_gb_kernel.h for why that
//      matters), a failed swap only re-compares against the row that won.
//   The last workgroup to finish turns `best row + 1` into a one-row selection per aggregate (LDB_NULL_ROW when no row
//   was non-NULL); the caller gathers the string through it, so no count returns to the host here.
// A column that carries an order-preserving dictionary (ldb_dict.hip) is compared on its 4-byte codes instead: the key
// is the code, it IS strict, and every candidate of the resolve pass is the same string.
#include "ldb_internal.h"
#include "ldb_device.h"
#include <memory>

#define SMM_MAX_AGGS 16 // = GB_MAX_OUT: a call cannot carry more aggregates
struct DStrAgg {
   DCol col; // the strings, or (codes != 0) the int32 dictionary codes of the column
   int32_t is_max;
   int32_t codes;
};
// global words per aggregate (zeroed arena words): reduced key, non-NULL rows, best row + 1; one arrival counter behind them
#define SMM_WORDS 3
#define SMM_W_KEY 0
#define SMM_W_COUNT 1
#define SMM_W_BEST 2
struct DStrMinMax {
   uint64_t n_rows;
   uint64_t words; // unsigned long long[SMM_WORDS * n_aggs + 1]
   int32_t n_aggs;
   int32_t pad;
   uint64_t sel_out[SMM_MAX_AGGS]; // uint32_t[1] each: the winning logical row, or LDB_NULL_ROW
   DStrAgg a[SMM_MAX_AGGS];
};

#define SMM_BLOCK 256
#define SMM_WAVES (SMM_BLOCK / LDB_WAVE)
#define SMM_U 2 // rows in flight per lane: row ids, then offsets, then bytes — three dependent loads per row

struct SmmRow {
   const uint8_t* p;
   uint32_t len;
   bool ok;
};

// the string of logical row i (codes: the code in `len`, p unused); ok = false for NULL
__device__ __forceinline__ SmmRow smm_row(const DStrAgg& a, uint64_t i) {
   SmmRow r{nullptr, 0, false};
   const uint32_t row = a.col.rowids ? gptr<uint32_t>(a.col.rowids)[i] : (uint32_t) i;
   if (a.col.rowids && row == LDB_NULL_ROW) return r;
   if (a.col.validity && !((gptr<uint8_t>(a.col.validity)[row >> 3] >> (row & 7)) & 1)) return r;
   if (a.codes) {
      r.len = gptr<uint32_t>(a.col.values)[row];
      r.ok = r.len != 0xFFFFFFFFu;
      return r;
   }
   const int64_t* o = gptr<int64_t>(a.col.offsets);
   const int64_t b = o[row], e = o[row + 1];
   r.p = gptr<uint8_t>(a.col.values) + b;
   r.len = (uint32_t) (e - b);
   r.ok = true;
   return r;
}
// first 8 bytes, big-endian, zero padded (codes: the code); MIN complements, so that larger is better for both
__device__ __forceinline__ uint64_t smm_key(const DStrAgg& a, const SmmRow& r) {
   uint64_t k = 0;
   if (a.codes) {
      k = r.len;
   } else {
      const uint32_t m = r.len < 8 ? r.len : 8;
#pragma unroll
      for (uint32_t j = 0; j < 8; j++) k = (k << 8) | (j < m ? (uint64_t) r.p[j] : 0ull);
   }
   return a.is_max ? k : ~k;
}
// is the string of logical row x STRICTLY better than that of row y?  Both rows are non-NULL and share the key: their first
// min(8, lengths) bytes are equal already.
__device__ __forceinline__ bool smm_better(const DStrAgg& a, uint64_t x, uint64_t y) {
   if (a.codes || x == y) return false; // one code = one string
   const SmmRow s = smm_row(a, x), t = smm_row(a, y);
   const uint32_t m = s.len < t.len ? s.len : t.len;
   for (uint32_t j = m < 8 ? m : 8; j < m; j++) {
      const uint8_t cs = s.p[j], ct = t.p[j];
      if (cs != ct) return a.is_max ? cs > ct : cs < ct;
   }
   return a.is_max ? s.len > t.len : s.len < t.len;
}

__global__ __launch_bounds__(SMM_BLOCK) void k_str_minmax_prefix(const DStrMinMax* __restrict__ d) {
   __shared__ unsigned long long s_key[SMM_WAVES];
   __shared__ unsigned long long s_cnt[SMM_WAVES];
   const uint64_t n = d->n_rows, stride = (uint64_t) gridDim.x * SMM_BLOCK;
   const uint32_t lane = threadIdx.x & (LDB_WAVE - 1), wave = threadIdx.x / LDB_WAVE;
   unsigned long long* words = gptr_mut<unsigned long long>(d->words);
   for (int ai = 0; ai < d->n_aggs; ai++) {
      const DStrAgg& a = d->a[ai];
      unsigned long long best = 0, cnt = 0;
      for (uint64_t i0 = blockIdx.x * (uint64_t) SMM_BLOCK + threadIdx.x; i0 < n; i0 += SMM_U * stride) {
         SmmRow r[SMM_U];
#pragma unroll
         for (int u = 0; u < SMM_U; u++) {
            const uint64_t i = i0 + (uint64_t) u * stride;
            r[u] = i < n ? smm_row(a, i) : SmmRow{nullptr, 0, false};
         }
#pragma unroll
         for (int u = 0; u < SMM_U; u++) {
            if (!r[u].ok) continue;
            const unsigned long long k = smm_key(a, r[u]);
            best = k > best ? k : best;
            cnt++;
         }
      }
      for (int off = LDB_WAVE / 2; off > 0; off >>= 1) {
         const unsigned long long ok = __shfl_down(best, off), oc = __shfl_down(cnt, off);
         best = ok > best ? ok : best;
         cnt += oc;
      }
      if (lane == 0) {
         s_key[wave] = best;
         s_cnt[wave] = cnt;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
         for (int w = 1; w < SMM_WAVES; w++) {
            best = s_key[w] > best ? s_key[w] : best;
            cnt += s_cnt[w];
         }
         if (cnt) { // (no non-NULL row here: nothing to say — the zeroed words are the identity of both)
            atomicMax(words + SMM_WORDS * ai + SMM_W_KEY, best);
            atomicAdd(words + SMM_WORDS * ai + SMM_W_COUNT, cnt);
         }
      }
      __syncthreads();
   }
}

__global__ __launch_bounds__(SMM_BLOCK) void k_str_minmax_resolve(const DStrMinMax* __restrict__ d) {
   const uint64_t n = d->n_rows, stride = (uint64_t) gridDim.x * SMM_BLOCK;
   const uint32_t lane = threadIdx.x & (LDB_WAVE - 1);
   unsigned long long* words = gptr_mut<unsigned long long>(d->words);
   for (int ai = 0; ai < d->n_aggs; ai++) {
      const DStrAgg& a = d->a[ai];
      if (words[SMM_WORDS * ai + SMM_W_COUNT] == 0) continue; // (uniform: written by the launch before this one)
      const unsigned long long win = words[SMM_WORDS * ai + SMM_W_KEY];
      unsigned long long mine = 0; // best candidate of this lane: logical row + 1
      for (uint64_t i0 = blockIdx.x * (uint64_t) SMM_BLOCK + threadIdx.x; i0 < n; i0 += SMM_U * stride) {
         SmmRow r[SMM_U];
#pragma unroll
         for (int u = 0; u < SMM_U; u++) {
            const uint64_t i = i0 + (uint64_t) u * stride;
            r[u] = i < n ? smm_row(a, i) : SmmRow{nullptr, 0, false};
         }
#pragma unroll
         for (int u = 0; u < SMM_U; u++) {
            const uint64_t i = i0 + (uint64_t) u * stride;
            if (!r[u].ok || smm_key(a, r[u]) != win) continue;
            if (!mine || smm_better(a, i, mine - 1)) mine = i + 1;
         }
      }
      // every lane of the wave is here (the loop bounds differ per lane, the code after the loop is reached by all)
      for (int off = LDB_WAVE / 2; off > 0; off >>= 1) {
         const unsigned long long other = __shfl_down(mine, off);
         if (other && (!mine || smm_better(a, other - 1, mine - 1))) mine = other;
      }
      if (lane == 0 && mine) {
         unsigned long long* slot = words + SMM_WORDS * ai + SMM_W_BEST;
         unsigned long long cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
         while (cur == 0 || smm_better(a, mine - 1, cur - 1)) {
            const unsigned long long prev = atomicCAS(slot, cur, mine);
            if (prev == cur) break;
            cur = prev; // somebody else got in: compare against THEIR row (the input columns are read-only, no fence needed for them)
         }
      }
   }
   // the last workgroup to arrive writes the selections
   __shared__ bool s_last;
   __threadfence();
   __syncthreads();
   if (threadIdx.x == 0) s_last = atomicAdd(words + SMM_WORDS * d->n_aggs, 1ull) == (unsigned long long) gridDim.x - 1ull;
   __syncthreads();
   if (!s_last) return;
   __threadfence();
   for (int ai = threadIdx.x; ai < d->n_aggs; ai += SMM_BLOCK) {
      const unsigned long long b = __hip_atomic_load(words + SMM_WORDS * ai + SMM_W_BEST, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *gptr_mut<uint32_t>(d->sel_out[ai]) = b ? (uint32_t) (b - 1) : LDB_NULL_ROW;
   }
}

int32_t ldb_str_minmax(ldb_ctx* ctx, const ldb_rel* in, const ldb_colref* cols, const int32_t* is_max, int32_t n, uint32_t** sel_out) {
   if (n < 1 || n > SMM_MAX_AGGS) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: %d string aggregates (max %d)", n, SMM_MAX_AGGS);
   if (!in->pending.empty()) LDB_FAIL(LDB_ERR_INVALID, "groupby: string MIN / MAX over a lazy relation");
   auto hp = std::make_unique<DStrMinMax>();
   DStrMinMax* h = hp.get();
   memset(h, 0, sizeof(*h));
   h->n_rows = (uint64_t) in->n_rows;
   h->n_aggs = n;
   bool all_codes = true;
   for (int32_t a = 0; a < n; a++) {
      // (the codes first: a lazy column has no bytes, and must not be written out for a consumer that reads codes)
      LDB_TRY(ldb_make_dcol_dict(in, cols[a], &h->a[a].col));
      const ldb_column& c = in->sides[(size_t) cols[a].side].table->cols[(size_t) cols[a].col];
      if (c.type.type != LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "groupby: string MIN / MAX over a column of type %d", c.type.type);
      h->a[a].codes = c.dict_codes != nullptr;
      h->a[a].is_max = is_max[a] ? 1 : 0;
      all_codes = all_codes && h->a[a].codes;
      h->sel_out[a] = (uint64_t) sel_out[a];
   }
   uint64_t* words;
   LDB_TRY(ldb_counters(ctx, SMM_WORDS * n + 1, &words)); // zeroed: key, count, best row + 1 per aggregate, then the arrival counter
   h->words = (uint64_t) words;
   LdbDesc<DStrMinMax> desc(ctx);
   LDB_TRY(desc.upload(h, sizeof(*h)));
   const DStrMinMax* d = desc.p;
   // a row of strings is two dependent misses (offsets, bytes): many waves per CU; codes stream
   const int grid = ldb_grid_for(ctx, (in->n_rows + SMM_U - 1) / SMM_U, SMM_BLOCK, all_codes ? 4 : 8);
   {
      LdbProf prof_(ctx, "k_str_minmax_prefix");
      hipLaunchKernelGGL(k_str_minmax_prefix, dim3(grid), dim3(SMM_BLOCK), 0, ctx->stream, d);
   }
   {
      LdbProf prof_(ctx, "k_str_minmax_resolve");
      hipLaunchKernelGGL(k_str_minmax_resolve, dim3(grid), dim3(SMM_BLOCK), 0, ctx->stream, d);
   }
   LDB_HIP(hipGetLastError());
   return LDB_OK;
}
