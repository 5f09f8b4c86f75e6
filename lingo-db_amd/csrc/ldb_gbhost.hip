// ldb_gbhost.hip — fused scan + predicate + hash group-by aggregation: host side, AOT kernels,
// and the hook into the run-time specialiser.  Device code: ldb_gb_kernel.h.
// Replaces (reference): the generated pipeline body around PreAggregationHashtableFragment
// (LookupPreAggrHtFragment, src/compiler/Conversion/SubOpToControlFlow/SubOpToControlFlow.cpp:3065-3157;
// ReduceOpLowering :3719-3768; PreAggregationHashtableFragment::insert,
// src/runtime/PreAggregationHashtable.cpp:46-60), PreAggregationHashtable::merge (:76-158),
// Hashtable (src/runtime/Hashtable.cpp) and SimpleState for key-less aggregates
// (src/runtime/SimpleState.cpp:8-30).
//
// MI355X design (not a port of the pointer-chained CPU tables):
//   * the reference's per-worker 1024-slot pre-aggregation cache becomes a per-workgroup table in
//     LDS (160 KB/CU): open addressing, slot word = {hash tag : 32 | representative row+1 : 32}
//     claimed by one 64-bit LDS CAS; accumulators are 64-bit words updated with LDS atomics.
//   * low-cardinality group-bys (TPC-H Q1: 4 groups) would serialise 64 lanes on a handful of
//     LDS addresses, so the table is REPLICATED R times and lane l works on replica l % R.
//   * 128-bit decimal SUMs are two 64-bit words: atomic add on the low word returns the old value,
//     the carry (old + v < old) is added to the high word — exact because additions commute and
//     every wrap of the low word is observed by exactly one lane.
//   * at the end each workgroup flushes its LDS groups into one global open-addressing table
//     (global 64-bit CAS + atomics); rows whose group does not fit LDS go to the global table
//     directly.  A final kernel compacts occupied slots into dense result columns.
//   * keys are never copied into the table: a slot names a representative input row; equality
//     is checked against that row's key columns (any key type, incl. strings), and the output key
//     columns are a gather of the representative rows (late materialisation).
//   * like the reference (which JIT-compiles each pipeline with LLVM), large inputs run a kernel
//     specialised at run time on the descriptor (hiprtc, ldb_jit.hip); small inputs and any
//     specialisation failure use the generic ahead-of-time kernel below — both are this source.
#include "ldb_internal.h"
#include "ldb_chain.h"
#include "ldb_gb_kernel.h"
#include "ldb_jit.h"
#include "ldb_strset.h"
#include <cmath>
#include <algorithm>
#include <memory>

extern __shared__ __attribute__((aligned(16))) unsigned long long gb_lds_dyn[];

// generic ahead-of-time kernel: metadata and addresses both come from the descriptor in memory
__global__ __launch_bounds__(GB_BLOCK) void k_groupby(const DGroupBy* __restrict__ d) { gb_body<1>(*d, d, gb_lds_dyn); }

__global__ void k_gb_sorted_heads(const DGroupBy* __restrict__ d, uint32_t* __restrict__ chunk_cnt) { gb_sorted_heads_body(*d, d, chunk_cnt); }

__global__ void k_gb_init(uint64_t* keys, uint64_t* acc, const DGroupBy* __restrict__ d) {
   const uint64_t cap = d->g_cap;
   const int nw = d->n_words;
   for (uint64_t p = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; p < cap; p += (uint64_t) gridDim.x * blockDim.x) {
      if (keys) keys[p] = (d->keyless && p == 0) ? 1ull : 0ull; // (dense_out: no slot words at all)
      for (int w = 0; w < nw; w++) acc[(uint64_t) w * cap + p] = d->word_init[w];
   }
}

// ---------------------------------------------------------------- partitioned counting (direct slots, COUNT(*) only)
// Q13's shape: 148 M rows → a row count per customer, 10 M random keys.  The direct path pays one global atomic per
// row into a 128 MB table (23 G atomics/s: 6.3 ms).  Here the rows' slots are first radix-partitioned by slot range —
// a histogram pass and a scatter pass with workgroup-private LDS cursors, 4 bytes per row each way — and then every
// partition (16 K consecutive slots) is counted by ONE workgroup in 64 KB of LDS and written to the table with plain,
// coalesced stores: no global atomics, ~2.5 GB of sequential traffic instead of 148 M random read-modify-writes.
// Semantics of the reference unchanged (PreAggregationHashtable.cpp:46-158 reduces thread-local fragments per
// partition; this is the same idea with LDS as the fragment).
#define GBP_BLOCK 256
#define GBP_SBLOCK 1024 // histogram / scatter: few, large workgroups → long per-(workgroup, partition) runs, full cache lines
#define GBP_SHIFT 14
#define GBP_MAX_PARTS 4096
__global__ __launch_bounds__(GBP_SBLOCK) void k_gbp_hist(const DGroupBy* __restrict__ d, uint32_t nparts, uint64_t rows_per_wg, uint32_t* __restrict__ hist) {
   __shared__ uint32_t h[GBP_MAX_PARTS];
   for (uint32_t p = threadIdx.x; p < nparts; p += GBP_SBLOCK) h[p] = 0;
   __syncthreads();
   const uint64_t n = d->n_rows, b = blockIdx.x * rows_per_wg, e = b + rows_per_wg < n ? b + rows_per_wg : n;
   for (uint64_t i = b + threadIdx.x; i < e; i += GBP_SBLOCK) atomicAdd(&h[(uint32_t) (d_direct_slot(*d, d, i) >> GBP_SHIFT)], 1u);
   __syncthreads();
   for (uint32_t p = threadIdx.x; p < nparts; p += GBP_SBLOCK) hist[(uint64_t) p * gridDim.x + blockIdx.x] = h[p];
}
__global__ __launch_bounds__(GBP_SBLOCK) void k_gbp_scatter(const DGroupBy* __restrict__ d, uint32_t nparts, uint64_t rows_per_wg, const uint32_t* __restrict__ offs, uint32_t* __restrict__ slots_out) {
   __shared__ uint32_t cur[GBP_MAX_PARTS];
   for (uint32_t p = threadIdx.x; p < nparts; p += GBP_SBLOCK) cur[p] = offs[(uint64_t) p * gridDim.x + blockIdx.x];
   __syncthreads();
   const uint64_t n = d->n_rows, b = blockIdx.x * rows_per_wg, e = b + rows_per_wg < n ? b + rows_per_wg : n;
   for (uint64_t i = b + threadIdx.x; i < e; i += GBP_SBLOCK) {
      const uint32_t slot = (uint32_t) d_direct_slot(*d, d, i);
      slots_out[atomicAdd(&cur[slot >> GBP_SHIFT], 1u)] = slot;
   }
}
// the rows' direct slots as a dense 32-bit array: the input of the write-combining partition (ldb_wc.hip)
__global__ void k_gbp_slots(const DGroupBy* __restrict__ d, uint32_t* __restrict__ slots) {
   const uint64_t n = d->n_rows;
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) slots[i] = (uint32_t) d_direct_slot(*d, d, i);
}
__global__ __launch_bounds__(GBP_BLOCK) void k_gbp_count(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ offs, uint32_t grid0, uint32_t nparts, uint64_t n_total,
                                                         uint64_t* __restrict__ counters) {
   __shared__ uint32_t c[1u << GBP_SHIFT];
   const uint32_t p = blockIdx.x;
   for (uint32_t j = threadIdx.x; j < (1u << GBP_SHIFT); j += GBP_BLOCK) c[j] = 0;
   __syncthreads();
   const uint64_t b = offs[(uint64_t) p * grid0], e = p + 1 < nparts ? (uint64_t) offs[(uint64_t) (p + 1) * grid0] : n_total;
   for (uint64_t i = b + threadIdx.x; i < e; i += GBP_BLOCK) atomicAdd(&c[slots[i] & ((1u << GBP_SHIFT) - 1)], 1u);
   __syncthreads();
   uint64_t* out = counters + ((uint64_t) p << GBP_SHIFT);
   for (uint32_t j = threadIdx.x; j < (1u << GBP_SHIFT); j += GBP_BLOCK) out[j] = c[j];
}

// the general case of the partitioned path: ANY aggregates over direct slots (Q15: SUM of a 128-bit product per supplier over 23 M random
// keys — 13 G global atomics / s = 4.6 ms).  The (slot, row) pairs are partitioned by slot range like the counts above; ONE workgroup then owns
// 2^shift consecutive slots, keeps their accumulator words in LDS (word w of local slot j at lds[w << shift | j]), folds its rows in with LDS
// atomics — the row's columns are gathered by row number — and writes the finished words to the table with plain coalesced stores.  The
// reference's merge works the same way: one task per partition of the pre-aggregation fragments (PreAggregationHashtable.cpp:76-158).
extern __shared__ __attribute__((aligned(16))) unsigned long long gbp_lds[];
__global__ __launch_bounds__(GBP_BLOCK) void k_gbp_agg(const DGroupBy* __restrict__ d, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ offs,
                                                       uint32_t grid0, uint32_t nparts, uint64_t n_total, uint32_t shift) {
   const uint32_t P = 1u << shift;
   const int nw = d->n_words;
   for (int w = 0; w < nw; w++) {
      const unsigned long long init = d->word_init[w];
      for (uint32_t j = threadIdx.x; j < P; j += GBP_BLOCK) gbp_lds[((uint32_t) w << shift) + j] = init;
   }
   __syncthreads();
   const uint32_t p = blockIdx.x;
   const uint64_t b = offs[(uint64_t) p * grid0], e = p + 1 < nparts ? (uint64_t) offs[(uint64_t) (p + 1) * grid0] : n_total;
   for (uint64_t i = b + threadIdx.x; i < e; i += GBP_BLOCK) {
      const uint32_t slot = slots[i] & (P - 1);
      const uint64_t row = rows[i];
      RowVals rv;
      uint32_t rvalid;
      d_load_vals(*d, d, row, rv, rvalid);
      const Sink s{gbp_lds + slot, P};
      d_accumulate(*d, d, rv, rvalid, row, s);
   }
   __syncthreads();
   unsigned long long* acc = (unsigned long long*) d->g_acc;
   const uint64_t cap = d->g_cap;
   for (int w = 0; w < nw; w++)
      for (uint32_t j = threadIdx.x; j < P; j += GBP_BLOCK) acc[(uint64_t) w * cap + ((uint64_t) p << shift) + j] = gbp_lds[((uint32_t) w << shift) + j];
}

// compact occupied slots → dense outputs
// occupied slots per 64-slot chunk (→ exclusive scan → output position of every group).  A cursor
// atomic per wave instead is one contended address: ~10 ns each in the L2 — 84 ms for the 8.4 M
// chunks of Q18's 150 M-group table.
__global__ void k_gb_occupancy(const uint64_t* __restrict__ g_keys, uint64_t cap, uint32_t* __restrict__ pop) {
   for (uint64_t p = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; p < ((cap + 63) & ~63ull); p += (uint64_t) gridDim.x * blockDim.x) {
      const uint64_t occ = __ballot(p < cap && g_keys[p] != 0);
      if ((threadIdx.x & 63) == 0) pop[p >> 6] = (uint32_t) __popcll(occ);
   }
}
// the same + the exclusive scan of the chunk counts in ONE chained launch (ldb_chain.h): a tile is 256 chunks (16 384 slots), a
// wave takes 64 of them with independent loads; off[c] = occupied slots before chunk c, *total = number of groups
#define GBO_TILE_CHUNKS 256
__global__ __launch_bounds__(256) void k_gb_occupancy_scan(const uint64_t* __restrict__ occ_words, uint64_t cap, uint64_t n_chunks, uint64_t n_tiles, uint32_t* __restrict__ off,
                                                           unsigned long long* __restrict__ total, unsigned long long* __restrict__ status, unsigned long long* __restrict__ ticket,
                                                           unsigned long long ticket_base, unsigned long long epoch) {
   __shared__ unsigned long long s_tile;
   __shared__ uint32_t s_wave[4];
   __shared__ uint32_t s_prefix;
   __shared__ uint32_t s_cnt[GBO_TILE_CHUNKS];
   if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1ull) - ticket_base;
   __syncthreads();
   const uint64_t tile = s_tile;
   const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const uint64_t chunk0 = tile * GBO_TILE_CHUNKS + (uint64_t) wave * 64;
#pragma unroll 8
   for (uint32_t k = 0; k < 64; k++) {
      const uint64_t p = (chunk0 + k) * 64 + lane;
      const uint64_t m = __ballot(p < cap && occ_words[p] != 0);
      if (lane == 0) s_cnt[wave * 64 + k] = (uint32_t) __popcll(m);
   }
   __syncthreads();
   const uint32_t own = s_cnt[threadIdx.x];
   uint32_t agg;
   uint32_t excl = d_block_scan256<uint32_t>(own, s_wave, &agg);
   if (threadIdx.x < 64) {
      const uint32_t prefix = d_chain_prefix<uint32_t, 32>(status, tile, epoch, agg, threadIdx.x);
      if (threadIdx.x == 0) s_prefix = prefix;
   }
   __syncthreads();
   const uint64_t c = tile * GBO_TILE_CHUNKS + threadIdx.x;
   if (c < n_chunks) off[c] = s_prefix + excl;
   if (total && tile == n_tiles - 1 && threadIdx.x == 0) *total = (unsigned long long) s_prefix + agg;
}
__global__ void k_gb_finalize(const DGroupBy* __restrict__ d, uint32_t* __restrict__ rep_rows, const uint32_t* __restrict__ chunk_off) {
   const uint64_t cap = d->g_cap;
   // occupancy: the slot word, or in direct-address mode the group's row counter
   const uint64_t* occ = d->direct ? (const uint64_t*) d->g_acc + (uint64_t) d->direct_word * cap : (const uint64_t*) d->g_keys;
   for (uint64_t p = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; p < ((cap + 63) & ~63ull); p += (uint64_t) gridDim.x * blockDim.x) {
      // the grid stride is a multiple of the wave size: a wave covers one aligned 64-slot chunk
      uint64_t w = p < cap ? occ[p] : 0;
      const uint64_t occ = __ballot(w != 0);
      if (w == 0) continue;
      const uint32_t lane = threadIdx.x & 63;
      uint64_t g = (uint64_t) chunk_off[p >> 6] + (uint64_t) __popcll(occ & ((1ull << lane) - 1ull));
      uint32_t rep = (uint32_t) w - 1u; // (meaningless in direct mode: no aggregate reads the representative row there)
      if (d->direct) { // the key IS the slot number
         const long long key = (long long) d->kmin + (long long) p;
         switch (d->direct_key_width) {
            case 4: ((int32_t*) d->direct_keys_out)[g] = (int32_t) key; break;
            case 8: ((int64_t*) d->direct_keys_out)[g] = (int64_t) key; break;
            default:
               ((int64_t*) d->direct_keys_out)[2 * g] = (int64_t) key;
               ((int64_t*) d->direct_keys_out)[2 * g + 1] = key < 0 ? -1 : 0;
         }
      } else {
         rep_rows[g] = rep;
      }
      d_finalize_group(*d, d, (const unsigned long long*) d->g_acc + p, cap, g, rep);
   }
}
// dense_out: the groups that cross a chunk boundary.  One lane per chunk: a flagged chunk holds the first row of a group that continues
// into the next chunk; its accumulators are the chunk's slot (word w at g_acc[w * n_chunks + chunk]), its number is the last group that
// begins in the chunk, its representative row was written by its first row.
__global__ void k_gb_finalize_cross(const DGroupBy* __restrict__ d, uint64_t n_chunks, const unsigned long long* __restrict__ d_groups) {
   const uint8_t* flags = (const uint8_t*) d->cross_flags;
   const uint32_t* chunk_off = (const uint32_t*) d->chunk_off;
   for (uint64_t c = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; c + 1 < n_chunks; c += (uint64_t) gridDim.x * blockDim.x) {
      if (!flags[c]) continue;
      const uint64_t g = (uint64_t) chunk_off[c + 1] - 1ull;
      if (g >= d->dense_groups) continue; // (mis-speculated replay)
      d_finalize_group(*d, d, (const unsigned long long*) d->g_acc + c, n_chunks, g, d->dense_keys == 2 ? 0u : ((const uint32_t*) d->rep_rows_out)[g]);
   }
   // the output arrays were sized from a count that may have been REPLAYED: should the real one be smaller (the execution is void and will be
   // repeated, but its consumers are queued already), the representative rows behind it must still be row numbers and the keys behind it keys
   // of the column's range (a table built over them indexes by key - min): row 0 / the first group's key.  Normally an empty range.
   for (uint64_t g = (uint64_t) *d_groups + blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; g < d->dense_groups; g += (uint64_t) gridDim.x * blockDim.x) {
      if (d->dense_keys != 2) ((uint32_t*) d->rep_rows_out)[g] = 0;
      if (d->dense_keys) {
         switch (d->direct_key_width) {
            case 4: ((int32_t*) d->direct_keys_out)[g] = ((const int32_t*) d->direct_keys_out)[0]; break;
            case 8: ((int64_t*) d->direct_keys_out)[g] = ((const int64_t*) d->direct_keys_out)[0]; break;
            default:
               ((int64_t*) d->direct_keys_out)[2 * g] = ((const int64_t*) d->direct_keys_out)[0];
               ((int64_t*) d->direct_keys_out)[2 * g + 1] = ((const int64_t*) d->direct_keys_out)[1];
         }
      }
   }
}

// per-group validity bytes → Arrow bitmap; *nulls += number of zero bytes (one atomic per wave of a
// bounded grid)
// (the row count is read on the device: the launch is queued before the host knows the number of groups; `cap` = the rows `bytes` and `bitmap` were
// allocated for — under a replay that is the RECORDED group count, and a mis-speculated execution may really have more groups: it is repeated
// after the end-of-trace comparison, but until then nothing may be read or written past the allocations)
__global__ void k_pack_valid_bytes(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ bitmap, const unsigned long long* __restrict__ d_n, uint64_t cap, unsigned long long* __restrict__ nulls) {
   const uint64_t n = min((uint64_t) *d_n, cap);
   uint64_t nb = (n + 7) / 8;
   unsigned int zeros = 0;
   for (uint64_t b = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; b < nb; b += (uint64_t) gridDim.x * blockDim.x) {
      uint8_t m = 0;
      for (int k = 0; k < 8; k++)
         if (b * 8 + k < n) {
            if (bytes[b * 8 + k])
               m |= (uint8_t) (1u << k);
            else
               zeros++;
         }
      bitmap[b] = m;
   }
   for (int off = 32; off > 0; off >>= 1) zeros += __shfl_down(zeros, off);
   if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(nulls, (unsigned long long) zeros);
}

// ---------------------------------------------------------------- host side
static bool same_acc(const DAcc& a, const DAcc& b) {
   if (a.kind != b.kind || a.n_cpreds != b.n_cpreds || a.count_rows != b.count_rows) return false;
   for (int p = 0; p < a.n_cpreds; p++)
      if (a.cpred[p] != b.cpred[p]) return false;
   if (a.kind == ACC_COUNT && a.count_rows) return true;
   return memcmp(&a.e, &b.e, sizeof(DExprG)) == 0;
}
struct GbBuilder {
   ldb_rel* in;
   DGroupBy* h;
   std::vector<ldb_colref> col_refs;
   bool str_codes = false; // the expression being converted is a string MIN / MAX argument (gb_str_arg): read the column's dictionary codes
   int32_t add_col(ldb_colref ref, int32_t* idx) {
      for (size_t k = 0; k < col_refs.size(); k++)
         if (col_refs[k].side == ref.side && col_refs[k].col == ref.col) {
            *idx = (int32_t) k;
            return LDB_OK;
         }
      if (col_refs.size() >= GB_MAX_COLS) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: more than %d distinct aggregate input columns", GB_MAX_COLS);
      DCol dc;
      if (str_codes) // grouped MIN / MAX over a dictionary-encoded string: the int32 codes stand in (order-preserving, ldb_dict.hip)
         LDB_TRY(ldb_make_dcol_dict(in, ref, &dc));
      else
         LDB_TRY(ldb_make_dcol(in, ref, &dc));
      if (dc.type == LDB_T_UTF8) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: string column in an aggregate expression");
      h->cols[col_refs.size()] = dc;
      *idx = (int32_t) col_refs.size();
      col_refs.push_back(ref);
      h->n_cols = (int32_t) col_refs.size();
      return LDB_OK;
   }
   int32_t conv_expr(const ldb_expr* e, DExprG* out, bool* nullable) {
      memset(out, 0, sizeof(*out));
      if (e->n_terms < 0 || e->n_terms > LDB_MAX_TERMS) LDB_FAIL(LDB_ERR_INVALID, "expression: %d terms (max %d)", e->n_terms, LDB_MAX_TERMS);
      out->n_terms = e->n_terms;
      out->is_float = e->is_float;
      for (int t = 0; t < e->n_terms; t++) {
         const ldb_term& tm = e->t[t];
         if (tm.n_factors < 0 || tm.n_factors > LDB_MAX_FACTORS) LDB_FAIL(LDB_ERR_INVALID, "expression: %d factors (max %d)", tm.n_factors, LDB_MAX_FACTORS);
         if (tm.div_pow10 < 0 || tm.div_pow10 > 38) LDB_FAIL(LDB_ERR_INVALID, "expression: div_pow10 %d", tm.div_pow10);
         out->t[t].n_factors = tm.n_factors;
         out->t[t].negate = tm.negate;
         out->t[t].div_pow10 = tm.div_pow10;
         // fits64: a bound on |Π (a + b * col)| from the bytes each column is stored in and its decimal precision (no statistics needed)
         long double bound = 1.0L;
         bool provable = !e->is_float && tm.n_factors > 0 && ldb_option("gb_fits64", 1) != 0;
         for (int f = 0; f < tm.n_factors; f++) {
            out->t[t].f[f].has_col = tm.f[f].has_col;
            out->t[t].f[f].a = tm.f[f].a;
            out->t[t].f[f].b = tm.f[f].b;
            if (tm.f[f].has_col) {
               int32_t idx;
               LDB_TRY(add_col(tm.f[f].col, &idx));
               out->t[t].f[f].col_idx = idx;
               const ldb_column& c = in->sides[(size_t) tm.f[f].col.side].table->cols[(size_t) tm.f[f].col.col];
               const ldb_rel_side& sd = in->sides[(size_t) tm.f[f].col.side];
               // NULL-able: the column has a validity bitmap, or its side can carry outer-join padding (LDB_NULL_ROW row ids)
               *nullable = *nullable || c.validity != nullptr || (sd.rowids && sd.may_null);
               bool colf = c.type.type == LDB_T_FLOAT64 || c.type.type == LDB_T_FLOAT32;
               if (colf && !e->is_float) LDB_FAIL(LDB_ERR_INVALID, "expression: float column in an integer expression (set is_float)");
               const int cw = c.type.type == LDB_T_UTF8 ? 4 : c.width; // (a string column is read as its int32 dictionary codes)
               long double cb = cw >= 8 ? 9.3e18L : (long double) (1ull << (8 * cw - 1)); // |v| <= 2^(8w-1)
               if (c.type.type == LDB_T_DECIMAL128) {
                  long double pb = 1.0L;
                  for (int k = 0; k < c.type.precision; k++) pb *= 10.0L;
                  cb = std::min(cb, pb);
                  if (c.type.precision >= 19) provable = false; // (a wide column is read as 128 bits)
               }
               if (colf) provable = false;
               bound *= std::max(1.0L, fabsl((long double) tm.f[f].a) + fabsl((long double) tm.f[f].b) * cb);
            } else {
               bound *= std::max(1.0L, fabsl((long double) tm.f[f].a));
            }
         }
         out->t[t].fits64 = provable && bound < 4.0e18L ? 1 : 0; // < 2^62; every factor's bound is >= 1, so every partial product is bounded by it too
      }
      return LDB_OK;
   }
   // accumulator `a` of `words` 64-bit words, the first initialised to `init`; an equal one that exists already is reused
   int32_t add_acc(DAcc& a, int words, uint64_t init, int32_t* idx) {
      for (int k = 0; k < h->n_accs; k++)
         if (same_acc(h->accs[k], a)) {
            *idx = k;
            return LDB_OK;
         }
      if (h->n_accs >= GB_MAX_ACCS || h->n_words + words > GB_MAX_WORDS) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: too many distinct accumulators");
      a.word = h->n_words;
      h->word_init[h->n_words] = init;
      for (int k = 1; k < words; k++) h->word_init[h->n_words + k] = 0;
      h->n_words += words;
      h->accs[h->n_accs] = a;
      *idx = h->n_accs++;
      return LDB_OK;
   }
   // the group's row counter: COUNT(*) without predicates
   int32_t add_rows_counter(int32_t* idx) {
      DAcc rows;
      memset(&rows, 0, sizeof(rows));
      rows.kind = ACC_COUNT;
      rows.count_rows = 1;
      return add_acc(rows, 1, 0, idx);
   }
   // counter of the rows contributing to aggregate `sp` (accumulator `acc`): AVG divisor, and NULL-ness of SUM / MIN / MAX results
   int32_t need_counter(const ldb_agg_spec& sp, const DAcc& acc, bool nullable, int32_t* idx) {
      DAcc c = acc;
      if (sp.fn == LDB_AGG_AVG && sp.has_count_expr) {
         // merging partial (sum, count) states: the divisor is SUM(count_expr)
         bool cn = false;
         c.kind = ACC_SUM64;
         c.count_rows = 0;
         LDB_TRY(conv_expr(&sp.count_expr, &c.e, &cn));
         if (c.e.is_float) LDB_FAIL(LDB_ERR_INVALID, "groupby: AVG count_expr must be an integer expression");
         return add_acc(c, 1, 0, idx);
      }
      c.kind = ACC_COUNT;
      c.count_rows = (!nullable && sp.fn != LDB_AGG_COUNT) ? 1 : 0;
      if (c.count_rows) memset(&c.e, 0, sizeof(c.e));
      return add_acc(c, 1, 0, idx);
   }
   // the predicates of a conditional aggregate, shared between the aggregates that name the same ones
   int32_t add_cpreds(const ldb_agg_spec& sp, DAcc& acc) {
      acc.n_cpreds = sp.n_preds;
      for (int p = 0; p < sp.n_preds; p++) {
         DPred dp;
         LDB_TRY(ldb_make_dpred(in, &sp.preds[p], &dp));
         int found = -1;
         for (int k = 0; k < h->n_cpreds; k++)
            if (!memcmp(&h->cpreds[k], &dp, sizeof(DPred))) found = k;
         if (found < 0) {
            if (h->n_cpreds >= GB_MAX_CPREDS) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: too many conditional-aggregate predicates");
            h->cpreds[h->n_cpreds] = dp;
            found = h->n_cpreds++;
         }
         acc.cpred[p] = found;
      }
      return LDB_OK;
   }
};

// ---------------------------------------------------------------- MIN / MAX over utf8 columns (ldb_str_minmax, ldb_strminmax.hip)
// Does the aggregate read a utf8 column?  The only such shape is MIN / MAX of the bare column (one term, one factor, a = 0, b = 1) with
// a utf8 result and no predicates of its own; *ref = that column.
static int32_t gb_str_arg(const ldb_rel* in, const ldb_agg_spec& sp, int32_t a, bool* is_str, ldb_colref* ref) {
   *is_str = false;
   if (sp.fn == LDB_AGG_COUNT_STAR) return LDB_OK;
   bool any = false;
   for (int t = 0; t < sp.arg.n_terms && t < LDB_MAX_TERMS; t++)
      for (int f = 0; f < sp.arg.t[t].n_factors && f < LDB_MAX_FACTORS; f++) {
         const ldb_factor& fa = sp.arg.t[t].f[f];
         if (!fa.has_col || fa.col.side < 0 || (size_t) fa.col.side >= in->sides.size()) continue; // (a bad reference is reported where it is resolved)
         const ldb_table* tb = in->sides[(size_t) fa.col.side].table;
         if (fa.col.col >= 0 && (size_t) fa.col.col < tb->cols.size() && tb->cols[(size_t) fa.col.col].type.type == LDB_T_UTF8) any = true;
      }
   if (!any) {
      if (sp.out_type == LDB_T_UTF8 && sp.fn != LDB_AGG_COUNT) LDB_FAIL(LDB_ERR_INVALID, "groupby: aggregate %d has a utf8 result type but no string argument", a);
      return LDB_OK;
   }
   const ldb_term& tm = sp.arg.t[0];
   if ((sp.fn != LDB_AGG_MIN && sp.fn != LDB_AGG_MAX) || sp.arg.n_terms != 1 || sp.arg.is_float || tm.n_factors != 1 || tm.negate || tm.div_pow10 || !tm.f[0].has_col || tm.f[0].a != 0 ||
       tm.f[0].b != 1)
      LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: string column in an aggregate expression (only MIN / MAX of the bare column)");
   if (sp.out_type != LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "groupby: aggregate %d is a MIN / MAX over a string column, its result type must be utf8 (got %d)", a, sp.out_type);
   if (sp.n_preds != 0) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: conditional MIN / MAX over a string column");
   *is_str = true;
   *ref = tm.f[0].col;
   return LDB_OK;
}

// The Join Order Benchmark's aggregate: no keys, MIN / MAX over strings (possibly beside other aggregates).  The filter runs first, the other
// aggregates go through the key-less path below on the filtered relation, all string aggregates through ldb_str_minmax together; each
// winning row is a one-row selection whose string the ordinary gather writes (a lazy dictionary column stays codes + dictionary until
// somebody needs the bytes).  One result row.
static int32_t gb_keyless_strings(ldb_ctx* ctx, ldb_rel* in, const ldb_filter_desc* preds, int32_t n_preds, const ldb_agg_spec* aggs, int32_t n_aggs, const std::vector<bool>& is_str,
                                  const std::vector<ldb_colref>& refs, ldb_table** out) {
   LDB_TRY(ldb_rel_force(ctx, in));
   LdbRelHold filtered(ctx);
   ldb_rel* cur = in;
   if (n_preds > 0) {
      LDB_TRY(ldb_gpu_scan_filter(ctx, in, preds, n_preds, &filtered.r));
      LDB_TRY(ldb_rel_force(ctx, filtered.r));
      cur = filtered.r;
   }
   if (cur->n_rows >= (int64_t) LDB_NULL_ROW) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: too many rows");
   std::vector<ldb_agg_spec> rest;
   std::vector<ldb_colref> scols;
   std::vector<int32_t> smax;
   for (int32_t a = 0; a < n_aggs; a++) {
      if (!is_str[(size_t) a]) {
         rest.push_back(aggs[a]);
         continue;
      }
      const ldb_colref ref = refs[(size_t) a];
      if (ref.side < 0 || (size_t) ref.side >= cur->sides.size() || ref.col < 0 || (size_t) ref.col >= cur->sides[(size_t) ref.side].table->cols.size())
         LDB_FAIL(LDB_ERR_INVALID, "groupby: aggregate %d: column %d:%d out of range", a, ref.side, ref.col);
      scols.push_back(ref);
      smax.push_back(aggs[a].fn == LDB_AGG_MAX ? 1 : 0);
   }
   LdbTableHold part(ctx), res(ctx);
   if (!rest.empty()) LDB_TRY(ldb_gpu_groupby(ctx, cur, nullptr, 0, nullptr, 0, rest.data(), (int32_t) rest.size(), 1, &part.t));
   LdbBufs bufs(ctx);
   std::vector<uint32_t*> sels(scols.size(), nullptr);
   for (auto& s : sels) LDB_TRY(bufs.alloc(&s, sizeof(uint32_t)));
   LDB_TRY(ldb_str_minmax(ctx, cur, scols.data(), smax.data(), (int32_t) scols.size(), sels.data()));
   res.t = new ldb_table();
   res.t->ctx = ctx;
   res.t->name = "groupby";
   res.t->n_rows = 1;
   res.t->cols.resize((size_t) n_aggs);
   size_t at_rest = 0, at_str = 0;
   for (int32_t a = 0; a < n_aggs; a++) {
      ldb_column& c = res.t->cols[(size_t) a];
      if (is_str[(size_t) a]) {
         LdbRelHold one(ctx);
         bufs.keep(sels[at_str]); // (ldb_rel_select takes the selection over)
         LDB_TRY(ldb_rel_select(ctx, cur, sels[at_str], 1, &one.r));
         for (auto& s : one.r->sides) s.may_null = true; // no non-NULL argument: the selection holds LDB_NULL_ROW and the result is NULL
         LDB_TRY(ldb_gather_columns(ctx, one.r, &scols[at_str], 1, &c));
         c.type.nullable = 1;
         at_str++;
      } else {
         c = part.t->cols[at_rest]; // the buffers move over with the column
         part.t->cols[at_rest].owned = false;
         part.t->cols[at_rest].dict = nullptr;
         part.t->cols[at_rest].dict_codes = nullptr;
         at_rest++;
      }
      char nm[32];
      snprintf(nm, sizeof(nm), "agg%d", a);
      c.name = nm;
   }
   *out = res.release();
   return LDB_OK;
}

// ---------------------------------------------------------------- ldb_gpu_groupby: the phases (DESIGN.md §2 names them)
// LDS table (S slots x R replicas inside a 60 KB budget, or none) and the global table's capacity: first guess (enlarged by a retry) and maximum
struct GbGeometry {
   size_t lds_bytes;
   uint64_t est, cap, cap_max;
};
static GbGeometry gb_geometry(DGroupBy* h, int64_t est_groups, int64_t n_rows) {
   GbGeometry g;
   const size_t slot_bytes = 8 * (size_t) (1 + h->n_words);
   const size_t lds_budget = 60 * 1024;
   g.est = h->keyless ? 1 : est_groups > 0 ? (uint64_t) est_groups : 0;
   uint32_t S = 1, R = 1;
   h->use_lds = 1;
   if (h->keyless) {
      R = 64;
   } else if (g.est == 0) {
      while ((size_t) S * 2 * slot_bytes <= lds_budget && S < 4096) S <<= 1;
   } else {
      S = (uint32_t) std::max<uint64_t>(8, next_pow2_u64(g.est * 2));
      if ((size_t) S * slot_bytes > lds_budget) {
         // more groups than LDS can pre-aggregate: the hit rate of a small cache is poor when
         // the input is not clustered, so go straight to the global table
         for (S = 1; (size_t) S * 2 * slot_bytes <= lds_budget;) S <<= 1;
         if (g.est > (uint64_t) S * 4) h->use_lds = 0;
      } else {
         while (R < 64 && (size_t) S * (R * 2) * slot_bytes <= lds_budget) R <<= 1;
      }
   }
   h->lds_slots = S;
   h->lds_reps = R;
   g.lds_bytes = h->use_lds ? (size_t) S * R * slot_bytes : 0;
   const uint64_t cap_guess = g.est ? g.est * 2 : std::min<uint64_t>((uint64_t) n_rows * 2, 1ull << 22);
   g.cap_max = next_pow2_u64(std::max<uint64_t>(1024, (uint64_t) n_rows * 2));
   g.cap = std::min(std::max<uint64_t>(1024, next_pow2_u64(cap_guess)), g.cap_max);
   return g;
}
// one turn of the retry loop: the table, the control words and the device descriptor of this attempt
struct GbAttempt {
   LdbBufs table; // released when the attempt ends, on every path (an error return included)
   uint64_t *gk = nullptr, *ga = nullptr;
   uint64_t max_groups = 0; // upper bound of groups = min(cap, rows) (1 for keyless); the sorted path knows the exact number
   unsigned long long* d_ctl = nullptr; // zeroed arena words, fresh ones per attempt (ldb_counters)
   LdbDesc<DGroupBy> desc; // given back after the attempt's control words are read, and on every error return
   explicit GbAttempt(ldb_ctx* ctx) : table(ctx), desc(ctx) {}
};
// what the attempt's flags ask for.  Anything but GB_DONE throws the attempt's outputs away (rare: the estimate was far too low).
enum GbVerdict { GB_DONE, GB_RETRY_HASHED, GB_RETRY_LARGER };
// what the phases of one call share
struct GbState {
   ldb_ctx* ctx;
   ldb_rel* in;
   const ldb_colref* keys;
   int32_t n_keys;
   const ldb_agg_spec* aggs;
   int32_t n_aggs;
   const std::vector<bool>& is_str; // aggregate a is a MIN / MAX over a dictionary string, str_ref[a] its column
   const std::vector<ldb_colref>& str_ref;
   DGroupBy* h;
   GbBuilder b;
   LdbBufs sorted_tmp; // the sorted path's chunk counts / offsets
   LdbBufs outs; // outputs of the current attempt: the survivors are kept into the result table, a failed attempt's are freed as a whole
   std::vector<ldb_coltype> otypes; // result column types (their widths: DOut::out_width)
   GbGeometry g{};
   unsigned __int128 key_range = 0; // ordered / direct slots: number of key values
   const ldb_column* direct_src = nullptr; // the key column where the kernels write the output keys themselves (direct slots; sorted keys with dense_keys)
   uint32_t* chunk_off = nullptr;
   uint64_t sorted_groups = 0, sorted_chunks = 0; // dense_sorted: number of groups / of 64-row chunks
   uint64_t* d_sorted_groups = nullptr; // the same count on the device (an arena word)
   void* direct_keys = nullptr;
   uint32_t* rep_rows = nullptr;
   std::vector<void*> out_vals;
   std::vector<uint8_t*> out_valid, bitmaps;
   // One control block per call, read back ONCE per attempt: [0] the kernel's overflow / long-probe flags, [1] the number of groups (total of
   // the occupancy scan), [2 + a] NULLs of aggregate a.
   unsigned long long ctl[2 + GB_MAX_OUT];
   void forget_outputs() {
      rep_rows = nullptr;
      direct_keys = nullptr;
      out_vals.assign((size_t) n_aggs, nullptr);
      out_valid = bitmaps = std::vector<uint8_t*>((size_t) n_aggs, nullptr);
   }
   bool any_fn() const { return std::any_of(aggs, aggs + n_aggs, [](const ldb_agg_spec& a) { return a.fn == LDB_AGG_ANY; }); }
   // aggregate a → its accumulators (h->accs, h->cpreds, h->word_init), its output descriptor h->outs[a] and its result column type
   int32_t lower_agg(int32_t a) {
      const ldb_agg_spec& sp = aggs[a];
      DOut& o = h->outs[a];
      memset(&o, 0, sizeof(o));
      o.fn = sp.fn;
      o.wide = sp.wide;
      o.avg_pow10 = sp.avg_pow10;
      o.acc = o.cnt_acc = o.cnt_rows_acc = o.cnt_pass_acc = -1;
      o.is_float = sp.arg.is_float && sp.fn != LDB_AGG_COUNT && sp.fn != LDB_AGG_COUNT_STAR;
      if (sp.n_preds < 0 || sp.n_preds > LDB_MAX_AGG_PREDS) LDB_FAIL(LDB_ERR_INVALID, "groupby: aggregate %d has %d predicates", a, sp.n_preds);
      if (sp.avg_pow10 < 0 || sp.avg_pow10 > 38) LDB_FAIL(LDB_ERR_INVALID, "groupby: avg_pow10 %d", sp.avg_pow10);
      DAcc acc;
      memset(&acc, 0, sizeof(acc));
      LDB_TRY(b.add_cpreds(sp, acc));
      bool nullable = false;
      const bool str = is_str[(size_t) a];
      if (str) { // grouped: only a dictionary makes a string a fixed-width value (an arg-min accumulator in every layout is the follow-up)
         const ldb_colref sr = str_ref[(size_t) a];
         if (sr.col < 0 || (size_t) sr.col >= in->sides[(size_t) sr.side].table->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "groupby: aggregate %d: column %d:%d out of range", a, sr.side, sr.col);
         const ldb_column& sc = in->sides[(size_t) sr.side].table->cols[(size_t) sr.col];
         if (!sc.dict_codes || !sc.dict) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: grouped MIN / MAX over a string column without a dictionary");
         o.wide = 0;
      }
      b.str_codes = str;
      if (sp.fn != LDB_AGG_COUNT_STAR) LDB_TRY(b.conv_expr(&sp.arg, &acc.e, &nullable));
      b.str_codes = false;
      o.e = acc.e;
      const bool is_min = sp.fn == LDB_AGG_MIN;
      switch (sp.fn) {
         case LDB_AGG_COUNT_STAR:
         case LDB_AGG_COUNT:
            acc.kind = ACC_COUNT;
            acc.count_rows = (sp.fn == LDB_AGG_COUNT_STAR || !nullable) ? 1 : 0;
            if (acc.count_rows) memset(&acc.e, 0, sizeof(acc.e));
            LDB_TRY(b.add_acc(acc, 1, 0, &o.acc));
            break;
         case LDB_AGG_SUM:
         case LDB_AGG_AVG: {
            acc.kind = sp.arg.is_float ? ACC_SUMF64 : sp.wide ? ACC_SUM128 : ACC_SUM64;
            LDB_TRY(b.add_acc(acc, acc.kind == ACC_SUM128 ? 2 : 1, 0, &o.acc));
            // a plain SUM over no non-NULL input is NULL; a conditional SUM (case … else 0) gets a
            // non-NULL 0 from every row failing its predicates (see DOut::cnt_rows_acc)
            if (sp.fn == LDB_AGG_AVG || nullable || (h->keyless && sp.n_preds == 0)) LDB_TRY(b.need_counter(sp, acc, nullable, &o.cnt_acc));
            if (sp.fn == LDB_AGG_SUM && sp.n_preds > 0 && (nullable || h->keyless)) {
               LDB_TRY(b.add_rows_counter(&o.cnt_rows_acc));
               if (nullable) {
                  DAcc passing = acc; // same predicates, counts rows
                  passing.kind = ACC_COUNT;
                  passing.count_rows = 1;
                  memset(&passing.e, 0, sizeof(passing.e));
                  LDB_TRY(b.add_acc(passing, 1, 0, &o.cnt_pass_acc));
               }
            }
            break;
         }
         case LDB_AGG_MIN:
         case LDB_AGG_MAX: {
            const bool wide = sp.wide && !sp.arg.is_float && !str; // low word, signed high word, lock word (d_sink_minmax128)
            const double inf = is_min ? __builtin_inf() : -__builtin_inf();
            uint64_t init = is_min ? (uint64_t) INT64_MAX : (uint64_t) INT64_MIN;
            if (sp.arg.is_float) memcpy(&init, &inf, 8);
            acc.kind = wide ? (is_min ? ACC_MIN128 : ACC_MAX128) : sp.arg.is_float ? (is_min ? ACC_MINF64 : ACC_MAXF64) : (is_min ? ACC_MIN64 : ACC_MAX64);
            LDB_TRY(b.add_acc(acc, wide ? 3 : 1, wide ? (is_min ? ~0ull : 0ull) : init, &o.acc));
            if (wide) h->word_init[h->accs[o.acc].word + 1] = init; // (the lock word starts at 0)
            if (nullable || h->keyless || sp.n_preds) LDB_TRY(b.need_counter(sp, acc, nullable, &o.cnt_acc));
            break;
         }
         case LDB_AGG_ANY: // evaluated on the group's representative row
            // the key-less group is pre-seeded with row 0 as its representative, which need not pass a fused filter
            if (h->keyless && h->n_preds > 0) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: ANY in a key-less aggregation with fused predicates (filter the relation first)");
            break;
         default: LDB_FAIL(LDB_ERR_INVALID, "groupby: unknown aggregate function %d", sp.fn);
      }
      ldb_coltype ot{};
      ot.type = sp.out_type;
      ot.precision = sp.out_precision;
      ot.scale = sp.out_scale;
      ot.nullable = 1;
      if (o.is_float) ot.type = LDB_T_FLOAT64;
      if (sp.fn == LDB_AGG_COUNT || sp.fn == LDB_AGG_COUNT_STAR) ot.type = LDB_T_INT64;
      if (str) ot.type = LDB_T_INT32; // the kernels write the winning code; the column becomes codes + the shared dictionary in result_table
      int w = ldb_width_of(ot, 0);
      if (w != 4 && w != 8 && w != 16) LDB_FAIL(LDB_ERR_INVALID, "groupby: aggregate %d output type %d unsupported", a, ot.type);
      o.out_width = w;
      otypes[(size_t) a] = ot;
      return LDB_OK;
   }
   int32_t lower_aggs() {
      h->n_outs = n_aggs;
      otypes.resize((size_t) n_aggs);
      for (int32_t a = 0; a < n_aggs; a++) LDB_TRY(lower_agg(a));
      int32_t idx;
      if (h->n_words == 0) LDB_TRY(b.add_rows_counter(&idx)); // at least one word so that every slot has something to initialise
      return LDB_OK;
   }
   // sorted key column, no filter (DGroupBy::dense_sorted): number the groups by key changes — the heads pass, its scan and the read-back
   int32_t sorted_layout(const ldb_column& kc) {
      const int64_t n_rows = in->n_rows, n_chunks = (n_rows + 63) / 64;
      uint32_t* chunk_cnt;
      LDB_TRY(sorted_tmp.alloc(&chunk_cnt, 4 * (size_t) n_chunks));
      LDB_TRY(sorted_tmp.alloc(&chunk_off, 4 * (size_t) n_chunks));
      LdbDesc<DGroupBy> dh_desc(ctx);
      LDB_TRY(dh_desc.upload(h, sizeof(*h)));
      DGroupBy* dh = dh_desc.p;
      {
         const int hgrid = ldb_grid_for(ctx, n_rows, 256, 8);
         hipFunction_t spec = nullptr;
         std::string why;
         if (ldb_jit_wanted(n_rows)) spec = ldb_jit_groupby_kernel(ctx->device, h, "k_gb_sorted_heads_spec", &why);
         LdbProf prof_(ctx, "k_gb_sorted_heads");
         if (spec) {
            void* params[] = {(void*) &dh, (void*) &chunk_cnt};
            LDB_HIP(hipModuleLaunchKernel(spec, (unsigned) hgrid, 1, 1, 256, 1, 1, 0, ctx->stream, params, nullptr));
         } else {
            hipLaunchKernelGGL(k_gb_sorted_heads, dim3(hgrid), dim3(256), 0, ctx->stream, dh, chunk_cnt);
         }
      }
      LDB_TRY(ldb_counters(ctx, 1, &d_sorted_groups));
      LDB_TRY(ldb_exclusive_scan_u32(ctx, chunk_cnt, chunk_off, n_chunks, d_sorted_groups));
      LDB_TRY(ldb_read_u64(ctx, d_sorted_groups, &sorted_groups));
      dh_desc.release();
      sorted_tmp.free(chunk_cnt);
      h->dense_sorted = 1;
      h->ordered_slots = 0;
      h->chunk_off = (uint64_t) chunk_off;
      g.cap = std::max<uint64_t>(1, sorted_groups); // the dense group array: exactly one slot per group
      sorted_chunks = (uint64_t) n_chunks;
      // groups inside one wave leave the kernel as final rows; the table shrinks to one slot per CHUNK for the groups that cross a
      // chunk boundary (DGroupBy::dense_out)
      h->dense_out = ldb_option("gb_dense_out", 1) != 0 ? 1 : 0;
      if (h->dense_out) g.cap = std::max<uint64_t>(1, sorted_chunks);
      // … and the key column itself: the first row of a group has its key in a register (no representative rows + gather afterwards: Q18's
      // 150 M keys, k_gather 0.72 ms); representative rows are still written when an ANY aggregate reads them
      if (h->dense_out && ldb_option("gb_dense_keys", 1) != 0 && !kc.validity && (kc.width == 4 || kc.width == 8 || kc.width == 16) && kc.type.type != LDB_T_UTF8 &&
          h->keys.cols[0].width == kc.width) {
         h->dense_keys = any_fn() ? 1 : 2;
         h->direct_key_width = kc.width;
         direct_src = &kc;
      }
      return LDB_OK;
   }
   // the global table's slot scheme for ONE integer key that LDS cannot pre-aggregate: ordered by key, dense over a sorted column, or addressed
   // directly by key - kmin; everything else keeps hashed slots
   int32_t choose_layout() {
      if (h->use_lds || n_keys != 1 || in->n_rows <= 0) return LDB_OK;
      const ldb_rel_side& ks = in->sides[(size_t) keys[0].side];
      const ldb_column& kc = ks.table->cols[(size_t) keys[0].col];
      // ordered global slots (DGroupBy::ordered_slots): a 32-bit value range
      if (ldb_option("gb_ordered", 1) != 0) {
         int64_t lo = 0, hi = -1;
         if (!kc.skewed && ldb_column_range(ctx, ks.table, keys[0].col, &lo, &hi) == LDB_OK && hi >= lo && (unsigned __int128) ((__int128) hi - lo) < ((unsigned __int128) 1 << 32)) {
            h->ordered_slots = 1;
            h->kmin = lo;
            key_range = (unsigned __int128) ((__int128) hi - lo) + 1;
         }
      }
      if (ldb_option("gb_sorted", 1) != 0 && h->n_preds == 0) {
         bool sorted = false;
         if (!ks.rowids) LDB_TRY(ldb_column_sorted(ctx, ks.table, keys[0].col, &sorted));
         if (sorted) LDB_TRY(sorted_layout(kc));
      }
      // direct-address slots (DGroupBy::direct): a NOT NULL key whose value range is at most twice the expected number of groups
      if (ldb_option("gb_direct", 1) != 0 && h->ordered_slots && !h->dense_sorted) {
         const uint64_t expect = std::max<uint64_t>(g.est ? g.est : (uint64_t) in->n_rows, 1024);
         if (!any_fn() && !kc.validity && !(ks.rowids && ks.may_null) && (kc.width == 4 || kc.width == 8 || kc.width == 16) && key_range <= (unsigned __int128) expect * 2 &&
             key_range <= ((unsigned __int128) 1 << 30)) {
            int32_t idx;
            LDB_TRY(b.add_rows_counter(&idx)); // (an existing COUNT(*) accumulator is reused)
            h->direct = 1;
            h->direct_word = h->accs[idx].word;
            h->direct_key_width = kc.width;
            direct_src = &kc;
            g.cap = std::max<uint64_t>(1024, next_pow2_u64((uint64_t) key_range));
         }
      }
      return LDB_OK;
   }

   int32_t attempt_alloc(GbAttempt& at) {
      const uint64_t cap = g.cap;
      h->g_cap = cap;
      h->kmult = h->ordered_slots ? (uint64_t) ((((unsigned __int128) cap) << 32) / key_range) : 0;
      uint8_t* cross = nullptr;
      if (!h->dense_out) LDB_TRY(at.table.alloc(&at.gk, 8 * (size_t) cap));
      LDB_TRY(at.table.alloc(&at.ga, 8 * (size_t) cap * (size_t) h->n_words));
      h->g_keys = (uint64_t) at.gk;
      h->g_acc = (uint64_t) at.ga;
      LDB_TRY(ldb_counters(ctx, 2 + GB_MAX_OUT, (uint64_t**) &at.d_ctl));
      h->g_flags = (uint64_t) at.d_ctl;
      const uint64_t max_groups = at.max_groups = std::max<uint64_t>(1, h->keyless ? 1 : h->dense_sorted ? sorted_groups : std::min<uint64_t>(cap, (uint64_t) in->n_rows));
      h->dense_groups = h->dense_sorted ? max_groups : 0;
      if (h->dense_out) {
         LDB_TRY(at.table.alloc(&cross, (size_t) sorted_chunks + 8));
         LDB_HIP(hipMemsetAsync(cross, 0, (size_t) sorted_chunks + 8, ctx->stream));
         h->cross_flags = (uint64_t) cross;
      }
      if (h->direct || h->dense_keys) {
         LDB_TRY(outs.alloc(&direct_keys, (size_t) h->direct_key_width * (size_t) max_groups));
         h->direct_keys_out = (uint64_t) direct_keys;
      }
      if (!h->direct && h->dense_keys != 2) {
         LDB_TRY(outs.alloc(&rep_rows, 4 * (size_t) max_groups));
         h->rep_rows_out = (uint64_t) rep_rows;
         // ordered slots give up on long probe runs, which depends on the insertion order: should a REPLAYED execution
         // (ldb_readback) meet that where the recorded one did not, its group count is too high until the trace ends and the
         // execution is repeated — the representative rows beyond the real count must then still be valid row numbers
         if (h->ordered_slots && ldb_replaying(ctx)) LDB_HIP(hipMemsetAsync(rep_rows, 0, 4 * (size_t) max_groups, ctx->stream));
      }
      for (int32_t a = 0; a < n_aggs; a++) {
         LDB_TRY(outs.alloc(&out_vals[(size_t) a], (size_t) h->outs[a].out_width * (size_t) max_groups));
         h->outs[a].out_values = (uint64_t) out_vals[(size_t) a];
         h->outs[a].out_valid = 0;
         if (h->outs[a].cnt_acc >= 0 || h->outs[a].cnt_rows_acc >= 0 || h->outs[a].fn == LDB_AGG_ANY) {
            LDB_TRY(outs.alloc(&out_valid[(size_t) a], (size_t) max_groups));
            LDB_TRY(outs.alloc(&bitmaps[(size_t) a], (size_t) ((max_groups + 7) / 8 + 1)));
            h->outs[a].out_valid = (uint64_t) out_valid[(size_t) a];
         }
      }
      return LDB_OK;
   }

   // ---- the four aggregation strategies
   // the rows' direct slots (+ their row numbers when `prow`) through the write-combining two-pass partition (ldb_wc.hip): written once as a dense
   // array, tile-sorted by partition in LDS and stored in full-line runs
   int32_t wc_partition(GbAttempt& at, LdbBufs& tmpb, uint32_t shift, uint32_t** slots, uint32_t** prow, uint32_t** part, uint32_t* chunks) {
      const int64_t n_rows = in->n_rows;
      uint32_t* raw;
      LDB_TRY(tmpb.alloc(&raw, 4 * (size_t) n_rows));
      LDB_TRY(tmpb.alloc(slots, 4 * (size_t) n_rows));
      if (prow) LDB_TRY(tmpb.alloc(prow, 4 * (size_t) n_rows));
      {
         LdbProf prof_(ctx, "k_gbp_slots");
         hipLaunchKernelGGL(k_gbp_slots, dim3(ldb_grid_for(ctx, n_rows, 256, 8)), dim3(256), 0, ctx->stream, (const DGroupBy*) at.desc.p, raw);
      }
      LDB_TRY(ldb_wc_partition(ctx, raw, nullptr, (uint64_t) n_rows, 0u, (uint32_t) (g.cap - 1), shift, (uint32_t) (g.cap >> shift), *slots, prow ? *prow : nullptr, part, chunks,
                               "k_gbp_hist", "k_gbp_scatter"));
      tmpb.adopt(*part);
      return LDB_OK;
   }
   // COUNT(*) per key over direct slots, partitioned with write-combining — the one-pass scatter below keeps nparts open 4-byte streams per
   // workgroup (Q13: 1 024), most of whose lines leave the L2 half written (2.4 ms for 148 M rows)
   int32_t count_partitioned_wc(GbAttempt& at, uint32_t nparts) {
      LdbBufs tmpb(ctx);
      uint32_t *slots, *part = nullptr, chunks = 1;
      LDB_TRY(wc_partition(at, tmpb, GBP_SHIFT, &slots, nullptr, &part, &chunks));
      LdbProf prof_(ctx, "k_gbp_count");
      hipLaunchKernelGGL(k_gbp_count, dim3(nparts), dim3(GBP_BLOCK), 0, ctx->stream, (const uint32_t*) slots, (const uint32_t*) part, chunks, nparts, (uint64_t) in->n_rows,
                         at.ga + (uint64_t) h->direct_word * g.cap);
      return LDB_OK;
   }
   // the same with the one-pass scatter: histogram, scan, scatter with workgroup-private cursors
   int32_t count_partitioned_scatter(GbAttempt& at, uint32_t nparts) {
      const int64_t n_rows = in->n_rows;
      const DGroupBy* d = at.desc.p;
      const uint32_t g0 = (uint32_t) std::max<int64_t>(1, std::min<int64_t>((int64_t) ctx->cus, (n_rows + 16383) / 16384));
      const uint64_t rows_per_wg = ((uint64_t) n_rows + g0 - 1) / g0;
      const size_t hn = (size_t) nparts * g0;
      LdbBufs tmpb(ctx);
      uint32_t *hist, *offs, *slots;
      LDB_TRY(tmpb.alloc(&hist, 4 * hn));
      LDB_TRY(tmpb.alloc(&offs, 4 * hn));
      LDB_TRY(tmpb.alloc(&slots, 4 * (size_t) n_rows));
      {
         LdbProf prof_(ctx, "k_gbp_hist");
         hipLaunchKernelGGL(k_gbp_hist, dim3(g0), dim3(GBP_SBLOCK), 0, ctx->stream, d, nparts, rows_per_wg, hist);
      }
      LDB_TRY(ldb_exclusive_scan_u32(ctx, hist, offs, (int64_t) hn, nullptr));
      {
         LdbProf prof_(ctx, "k_gbp_scatter");
         hipLaunchKernelGGL(k_gbp_scatter, dim3(g0), dim3(GBP_SBLOCK), 0, ctx->stream, d, nparts, rows_per_wg, (const uint32_t*) offs, slots);
      }
      LdbProf prof_(ctx, "k_gbp_count");
      hipLaunchKernelGGL(k_gbp_count, dim3(nparts), dim3(GBP_BLOCK), 0, ctx->stream, (const uint32_t*) slots, (const uint32_t*) offs, g0, nparts, (uint64_t) n_rows,
                         at.ga + (uint64_t) h->direct_word * g.cap);
      return LDB_OK;
   }
   // any aggregates over direct slots too many for the caches, many rows: partition (slot, row) pairs, aggregate every slot range in LDS
   int32_t aggregate_partitioned(GbAttempt& at, uint32_t pv_shift) {
      LdbBufs tmpb(ctx);
      uint32_t *slots, *prow, *part = nullptr, chunks = 1;
      LDB_TRY(wc_partition(at, tmpb, pv_shift, &slots, &prow, &part, &chunks));
      LdbProf prof_(ctx, "k_gbp_agg");
      hipLaunchKernelGGL(k_gbp_agg, dim3((uint32_t) (g.cap >> pv_shift)), dim3(GBP_BLOCK), (size_t) 8 * (size_t) h->n_words << pv_shift, ctx->stream, (const DGroupBy*) at.desc.p,
                         (const uint32_t*) slots, (const uint32_t*) prow, (const uint32_t*) part, chunks, (uint32_t) (g.cap >> pv_shift), (uint64_t) in->n_rows, pv_shift);
      return LDB_OK;
   }
   // the fused scan + aggregation kernel, generic or specialised
   int32_t aggregate_plain(GbAttempt& at) {
      const DGroupBy* d = at.desc.p;
      int per_cu = g.lds_bytes > 40 * 1024 ? 2 : 4;
      // (the sorted, LDS-free path was swept over 2 / 3 / 4 / 6 / 8 resident workgroups per CU: 5.52 / 4.22 / 3.90 / 3.70 / 3.83 ms on one box, but 6 gave 4.05 ms on the
      // next one where 4 gives ≈ 3.95: inside the box-to-box spread, so the default stays)
      if (const int64_t forced = ldb_option("gb_wgs_per_cu", 0)) per_cu = (int) std::max<int64_t>(1, std::min<int64_t>(forced, 16)); // experiments (Q1's line re-fetches)
      const int grid = ldb_grid_for(ctx, in->n_rows, GB_BLOCK, per_cu);
      hipFunction_t spec = nullptr;
      if (ldb_jit_wanted(in->n_rows)) {
         std::string why;
         spec = ldb_jit_groupby(ctx->device, h, &why);
         if (!spec) ldb_set_error("groupby: specialised kernel unavailable (%s); using the generic kernel", why.c_str());
      }
      LdbProf prof_(ctx, h->direct ? "k_groupby_direct" : "k_groupby"); // (the same kernel; the name tells the profile which slot scheme ran)
      if (spec) {
         void* params[] = {(void*) &d};
         LDB_HIP(hipModuleLaunchKernel(spec, (unsigned) grid, 1, 1, GB_BLOCK, 1, 1, (unsigned) g.lds_bytes, ctx->stream, params, nullptr));
      } else {
         hipLaunchKernelGGL(k_groupby, dim3(grid), dim3(GB_BLOCK), g.lds_bytes, ctx->stream, d);
      }
      return LDB_OK;
   }
   int32_t launch_aggregate(GbAttempt& at) {
      const int64_t n_rows = in->n_rows;
      const bool many_rows = n_rows >= ldb_option("gb_partition_min_rows", 8ll << 20) && (uint64_t) n_rows < (1ull << 32) && ldb_option("gb_partition", 1) != 0;
      // COUNT(*) per key over direct slots, many rows into a table far beyond the L2: partition, then count in LDS
      const bool partitioned = h->direct && h->n_words == 1 && h->n_accs == 1 && h->n_preds == 0 && h->n_cpreds == 0 && g.cap >= (1ull << 20) && (g.cap >> GBP_SHIFT) <= GBP_MAX_PARTS && many_rows;
      // the same for arbitrary aggregates (k_gbp_agg): as many slots per partition as their accumulator words fit into 60 KB of LDS
      uint32_t pv_shift = 0;
      while (pv_shift < 16 && ((size_t) 8 * (size_t) h->n_words << (pv_shift + 1)) <= 60 * 1024) pv_shift++;
      bool wide_minmax = false;
      for (int a = 0; a < h->n_accs; a++) wide_minmax = wide_minmax || h->accs[a].kind == ACC_MIN128 || h->accs[a].kind == ACC_MAX128;
      const bool part_values = !partitioned && h->direct && h->n_preds == 0 && !wide_minmax && g.cap >= (1ull << 20) && pv_shift >= 8 && (g.cap >> pv_shift) <= GBP_MAX_PARTS && many_rows &&
         ldb_option("gb_partition_values", 1) != 0;
      if (partitioned) {
         const uint32_t nparts = (uint32_t) (g.cap >> GBP_SHIFT);
         if (ldb_option("gb_partition_wc", 1) != 0 && nparts > 64) LDB_TRY(count_partitioned_wc(at, nparts));
         else LDB_TRY(count_partitioned_scatter(at, nparts));
      } else if (part_values) {
         LDB_TRY(aggregate_partitioned(at, pv_shift));
      } else if (n_rows) {
         LDB_TRY(aggregate_plain(at));
      }
      LDB_HIP(hipGetLastError());
      return LDB_OK;
   }

   // ---- finalize (speculative: queued right behind the aggregation without waiting for its flags; valid only if they come back clean)
   // per-group validity bytes → Arrow bitmaps + NULL counts; d_count = the device word that holds the number of groups
   void pack_valid(GbAttempt& at, const unsigned long long* d_count) {
      for (int32_t a = 0; a < n_aggs; a++)
         if (out_valid[(size_t) a])
            hipLaunchKernelGGL(k_pack_valid_bytes, dim3(ldb_grid_for(ctx, (int64_t) at.max_groups, 256 * 8, 4)), dim3(256), 0, ctx->stream, out_valid[(size_t) a], bitmaps[(size_t) a], d_count,
                               (uint64_t) at.max_groups, at.d_ctl + 2 + a);
   }
   // dense_out: every group inside one wave is final already — only the chunk-crossing groups are left, the count is known
   int32_t finalize_dense(GbAttempt& at) {
      LdbProf prof_(ctx, "k_gb_finalize");
      hipLaunchKernelGGL(k_gb_finalize_cross, dim3(ldb_grid_for(ctx, (int64_t) sorted_chunks, 256, 8)), dim3(256), 0, ctx->stream, (const DGroupBy*) at.desc.p, sorted_chunks,
                         (const unsigned long long*) d_sorted_groups);
      pack_valid(at, (const unsigned long long*) d_sorted_groups);
      LDB_HIP(hipGetLastError());
      return LDB_OK;
   }
   // occupied slots per 64-slot chunk → exclusive scan (the group count lands in ctl[1]) → k_gb_finalize compacts the groups
   int32_t finalize_slots(GbAttempt& at) {
      const uint64_t cap = g.cap;
      LdbProf prof_(ctx, "k_gb_finalize");
      const int64_t n_chunks = (int64_t) ((cap + 63) / 64);
      LdbBufs fin(ctx);
      uint32_t *pop = nullptr, *off;
      LDB_TRY(fin.alloc(&off, 4 * (size_t) n_chunks));
      const int fgrid = ldb_grid_for(ctx, (int64_t) cap, 256, 8);
      const uint64_t* occ = h->direct ? (const uint64_t*) h->g_acc + (uint64_t) h->direct_word * cap : (const uint64_t*) h->g_keys;
      if (ldb_option("scan_single_pass", 1) != 0) { // occupied slots per chunk + their exclusive scan + the group count: one chained launch
         const uint64_t n_tiles = ((uint64_t) n_chunks + GBO_TILE_CHUNKS - 1) / GBO_TILE_CHUNKS;
         ChainCall c;
         LDB_TRY(ldb_chain_begin(ctx, n_tiles, false, &c));
         hipLaunchKernelGGL(k_gb_occupancy_scan, dim3((unsigned) n_tiles), dim3(256), 0, ctx->stream, occ, cap, (uint64_t) n_chunks, n_tiles, off, at.d_ctl + 1, c.status, c.ticket, c.ticket_base,
                            c.epoch);
         if (hipGetLastError() != hipSuccess) return ldb_chain_failed(ctx);
      } else {
         LDB_TRY(fin.alloc(&pop, 4 * (size_t) n_chunks));
         hipLaunchKernelGGL(k_gb_occupancy, dim3(fgrid), dim3(256), 0, ctx->stream, occ, cap, pop);
         LDB_TRY(ldb_exclusive_scan_u32(ctx, pop, off, n_chunks, (uint64_t*) (at.d_ctl + 1)));
      }
      hipLaunchKernelGGL(k_gb_finalize, dim3(fgrid), dim3(256), 0, ctx->stream, (const DGroupBy*) at.desc.p, rep_rows, (const uint32_t*) off);
      pack_valid(at, at.d_ctl + 1);
      LDB_HIP(hipGetLastError());
      return LDB_OK;
   }
   int32_t verdict(GbVerdict* v) {
      const uint64_t flags = (uint64_t) ctl[0];
      *v = GB_DONE;
      if ((flags & 3) == 0) return LDB_OK;
      outs.free_all();
      forget_outputs();
      if ((flags & 2) && h->ordered_slots) { // long probe runs: this key distribution needs hashed slots
         h->ordered_slots = 0;
         in->sides[(size_t) keys[0].side].table->cols[(size_t) keys[0].col].skewed = true;
         *v = GB_RETRY_HASHED;
         if ((flags & 1) == 0) return LDB_OK;
      }
      // global table overflowed: retry larger (the estimate was too low)
      if (g.cap >= g.cap_max) LDB_FAIL(LDB_ERR_HIP, "groupby: global table overflow at maximum capacity");
      g.cap = std::min(g.cap * 8, g.cap_max);
      *v = GB_RETRY_LARGER;
      return LDB_OK;
   }
   int32_t attempt(GbVerdict* v) {
      GbAttempt at(ctx);
      LDB_TRY(attempt_alloc(at));
      LDB_TRY(at.desc.upload(h, sizeof(*h)));
      hipLaunchKernelGGL(k_gb_init, dim3(ldb_grid_for(ctx, (int64_t) g.cap, 256, 8)), dim3(256), 0, ctx->stream, at.gk, at.ga, (const DGroupBy*) at.desc.p);
      LDB_TRY(launch_aggregate(at));
      LDB_TRY(h->dense_out ? finalize_dense(at) : finalize_slots(at));
      static_assert(sizeof(ctl) <= 64 * sizeof(int64_t), "control block must fit the pinned scratch words");
      LDB_TRY(LDB_READBACK(ctx, ctl, at.d_ctl, sizeof(ctl)));
      if (h->dense_out) ctl[1] = sorted_groups; // (no occupancy scan ran: the heads pass counted the groups)
      at.desc.release();
      return verdict(v);
   }

   // key columns = gather of the representative rows (or what the kernels wrote themselves), then the aggregates
   int32_t result_table(ldb_table** out) {
      const uint64_t n_groups = (uint64_t) ctl[1];
      LdbTableHold res(ctx, new ldb_table());
      res->ctx = ctx;
      res->name = "groupby";
      res->n_rows = (int64_t) n_groups;
      res->cols.resize((size_t) (n_keys + n_aggs));
      if (h->direct || h->dense_keys) { // the key column was written by k_gb_finalize / by the sorted aggregation itself
         ldb_column& kc = res->cols[0];
         kc.name = direct_src->name;
         kc.type = direct_src->type;
         kc.width = direct_src->width;
         kc.values = direct_keys;
         outs.keep(direct_keys);
         kc.value_bytes = (int64_t) n_groups * kc.width;
         kc.owned = true;
         if (direct_src->has_range) { // the groups' keys are values of the source column: its cached range stays a valid superset
            kc.has_range = true;
            kc.vmin = direct_src->vmin;
            kc.vmax = direct_src->vmax;
         }
         outs.free(rep_rows); // (sorted keys with an ANY aggregate: the representative rows were only read by the finalisation)
      } else {
         LdbRelHold reps(ctx);
         outs.keep(rep_rows); // (ldb_rel_select takes the selection over)
         LDB_TRY(ldb_rel_select(ctx, in, rep_rows, (int64_t) n_groups, &reps.r));
         if (n_keys) LDB_TRY(ldb_gather_columns(ctx, reps.r, keys, n_keys, res->cols.data()));
      }
      for (int32_t a = 0; a < n_aggs; a++) {
         ldb_column& c = res->cols[(size_t) (n_keys + a)];
         char nm[32];
         snprintf(nm, sizeof(nm), "agg%d", a);
         c.name = nm;
         c.type = otypes[(size_t) a];
         c.width = h->outs[a].out_width;
         c.values = out_vals[(size_t) a];
         outs.keep(c.values);
         c.value_bytes = (int64_t) n_groups * c.width;
         c.owned = true;
         if (is_str[(size_t) a]) { // a LAZY utf8 column (ldb_column_is_lazy): the codes the kernels wrote + the argument column's dictionary
            const ldb_column& sc = in->sides[(size_t) str_ref[(size_t) a].side].table->cols[(size_t) str_ref[(size_t) a].col];
            c.type = sc.type;
            c.type.nullable = 1;
            c.width = sc.width;
            c.dict_codes = (uint32_t*) c.values;
            c.values = nullptr;
            c.value_bytes = -1;
            c.dict = sc.dict;
            c.dict->dict_refs++;
            c.dict_size = sc.dict_size;
            c.dict_pred_cache = new std::unordered_map<std::string, std::string>();
         }
         if (bitmaps[(size_t) a]) { // drop the bitmap when nothing is NULL
            const int64_t nulls = (int64_t) ctl[2 + a];
            if (nulls) {
               c.validity = bitmaps[(size_t) a];
               outs.keep(c.validity);
               c.null_count = nulls;
            } else {
               outs.free(bitmaps[(size_t) a]);
            }
         }
      }
      LDB_HIP(hipGetLastError());
      *out = res.release();
      return LDB_OK;
   }
};

extern "C" int32_t ldb_gpu_groupby(ldb_ctx* ctx, ldb_rel* in, const ldb_filter_desc* preds, int32_t n_preds, const ldb_colref* keys, int32_t n_keys,
                                   const ldb_agg_spec* aggs, int32_t n_aggs, int64_t est_groups, ldb_table** out) {
   if (!ctx || !in || !out) LDB_FAIL(LDB_ERR_INVALID, "groupby: NULL argument");
   if (n_preds < 0 || n_preds > LDB_MAX_PREDS) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: %d predicates (max %d)", n_preds, LDB_MAX_PREDS);
   // MIN / MAX over utf8 columns: key-less → the string reduction; grouped → the dictionary codes through the integer accumulators
   std::vector<bool> is_str((size_t) std::max(n_aggs, 0), false);
   std::vector<ldb_colref> str_ref((size_t) std::max(n_aggs, 0), ldb_colref{0, 0});
   bool any_str = false;
   if (n_aggs <= GB_MAX_OUT)
      for (int32_t a = 0; a < n_aggs; a++) {
         bool s = false;
         LDB_TRY(gb_str_arg(in, aggs[a], a, &s, &str_ref[(size_t) a]));
         is_str[(size_t) a] = s;
         any_str = any_str || s;
      }
   if (any_str && n_keys == 0) return gb_keyless_strings(ctx, in, preds, n_preds, aggs, n_aggs, is_str, str_ref, out);
   if (ldb_strset_any(in, preds, n_preds)) { // a string-set conjunct is evaluated by the scan alone: filter first, aggregate the filtered relation
      LdbRelHold filtered(ctx);
      LDB_TRY(ldb_gpu_scan_filter(ctx, in, preds, n_preds, &filtered.r));
      return ldb_gpu_groupby(ctx, filtered.r, nullptr, 0, keys, n_keys, aggs, n_aggs, est_groups, out);
   }
   if (in->pending.size() + (size_t) n_preds > LDB_MAX_PREDS) LDB_TRY(ldb_rel_force(ctx, in)); // else: a lazy input's conjuncts are fused below
   if (n_keys == 0 && !in->pending.empty()) // key-less ANY needs a representative row that passed the filter: materialise a lazy input
      for (int32_t a = 0; a < n_aggs; a++)
         if (aggs[a].fn == LDB_AGG_ANY) {
            LDB_TRY(ldb_rel_force(ctx, in));
            break;
         }
   // one integer key over a range too large for the caches, many rows, a lazy filter in front: the filter is evaluated FIRST — the partitioned
   // aggregation (k_gbp_agg) wants the surviving rows as a dense list, and a selective filter (Q15: 23 M of 600 M rows) then decides
   // whether it is worth it at all.  The fused alternative pays one global atomic per accumulator and surviving row.
   if (n_keys == 1 && n_preds == 0 && !in->pending.empty() && in->n_rows >= ldb_option("gb_partition_min_rows", 8ll << 20) && ldb_option("gb_partition", 1) != 0 &&
       ldb_option("gb_partition_values", 1) != 0 && ldb_option("gb_direct", 1) != 0 && est_groups >= (1 << 19)) {
      const ldb_rel_side& ks = in->sides[(size_t) keys[0].side];
      const ldb_column& kc = ks.table->cols[(size_t) keys[0].col];
      int64_t lo = 0, hi = -1;
      if (!kc.validity && !ks.rowids && (kc.width == 4 || kc.width == 8) && ldb_column_range(ctx, ks.table, keys[0].col, &lo, &hi) == LDB_OK && hi >= lo) {
         const unsigned __int128 range = (unsigned __int128) ((__int128) hi - lo) + 1;
         if (range >= ((unsigned __int128) 1 << 19) && range <= (unsigned __int128) est_groups * 2 && range <= ((unsigned __int128) 1 << 30)) LDB_TRY(ldb_rel_force(ctx, in));
      }
   }
   if (n_aggs < 0 || n_aggs > GB_MAX_OUT) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: %d aggregates (max %d)", n_aggs, GB_MAX_OUT);
   if (in->n_rows >= (int64_t) LDB_NULL_ROW) LDB_FAIL(LDB_ERR_UNSUPPORTED, "groupby: too many rows");
   auto hp = std::make_unique<DGroupBy>();
   DGroupBy* h = hp.get();
   memset(h, 0, sizeof(*h));
   h->n_rows = (uint64_t) in->n_rows;
   h->n_preds = n_preds;
   for (int32_t p = 0; p < n_preds; p++) LDB_TRY(ldb_make_dpred(in, &preds[p], &h->preds[p]));
   for (auto& dp : in->pending) h->preds[h->n_preds++] = dp;
   ldb_order_preds(h->preds, h->n_preds); // cheap conjuncts first, same-column neighbours marked
   h->batch_rows = h->n_preds >= 2 ? 8 : 4;
   LDB_TRY(ldb_make_dkeys_dict(in, keys, n_keys, &h->keys)); // (dictionary codes stand in for low-cardinality strings: hashing and equality only)
   h->keyless = n_keys == 0;

   GbState s{ctx, in, keys, n_keys, aggs, n_aggs, is_str, str_ref, h, {in, h, {}}, LdbBufs(ctx), LdbBufs(ctx)};
   s.forget_outputs();
   LDB_TRY(s.lower_aggs());
   s.g = gb_geometry(h, est_groups, in->n_rows);
   LDB_TRY(s.choose_layout());
   GbVerdict v = GB_RETRY_LARGER; // (nothing attempted yet)
   while (v != GB_DONE) LDB_TRY(s.attempt(&v));
   s.sorted_tmp.free(s.chunk_off);
   for (int32_t a = 0; a < n_aggs; a++) s.outs.free(s.out_valid[(size_t) a]);
   return s.result_table(out);
}
