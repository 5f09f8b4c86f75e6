// ldb_prims.hip — device primitives shared by the operators: exclusive scans (chained single-launch, and the three-level
// form), the chain's device state (ldb_chain.h), selection bitmap → ascending row numbers.
#include "ldb_internal.h"
#include "ldb_device.h"
#include "ldb_chain.h"
#include "ldb_expand.h"
#include <algorithm>

// ---------------------------------------------------------------- exclusive scans
// Small inputs: one workgroup (k_scan_block).  Everything else: ONE launch of a chained scan with decoupled look-back
// (k_scan_chain) — a tile of 2048 elements per workgroup, tile numbers handed out by a ticket counter (a tile only ever
// waits for tiles whose workgroups are already running), per-tile status words {epoch, state, value} that are never
// cleared: every call owns a fresh epoch, and a word of another epoch reads as "not there yet".  The three-level version
// this replaces (per-block sums → recursive scan → add back) was 22 % of all launches of a 22-query pass.
// Status word: value in the low VBITS bits, state (1 = the tile's own sum, 2 = inclusive prefix) above it, epoch on top.
template <typename T, typename TO, typename TT, int VBITS>
__global__ __launch_bounds__(256) void k_scan_chain(const T* __restrict__ in, TO* __restrict__ out, uint64_t n, uint64_t n_tiles, TT* __restrict__ total,
                                                    unsigned long long* __restrict__ status, unsigned long long* __restrict__ ticket, unsigned long long ticket_base,
                                                    unsigned long long epoch) {
   __shared__ unsigned long long s_tile;
   __shared__ TO s_wave[4];
   __shared__ TO s_prefix;
   if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1ull) - ticket_base;
   __syncthreads();
   const uint64_t tile = s_tile;
   const uint64_t base = tile * CHAIN_TILE + (uint64_t) threadIdx.x * CHAIN_ITEMS;
   TO v[CHAIN_ITEMS];
   TO sum = 0;
#pragma unroll
   for (int k = 0; k < CHAIN_ITEMS; k++) {
      v[k] = base + k < n ? (TO) in[base + k] : (TO) 0;
      sum += v[k];
   }
   TO agg;
   TO excl = d_block_scan256<TO>(sum, s_wave, &agg);
   if (threadIdx.x < 64) {
      const TO prefix = d_chain_prefix<TO, VBITS>(status, tile, epoch, agg, threadIdx.x);
      if (threadIdx.x == 0) s_prefix = prefix;
   }
   __syncthreads();
   excl += s_prefix;
   if (total && tile == n_tiles - 1 && threadIdx.x == 0) *total = (TT) (s_prefix + agg);
#pragma unroll
   for (int k = 0; k < CHAIN_ITEMS; k++) {
      if (base + k < n) out[base + k] = excl;
      excl += v[k];
   }
}
// the chain's device state: status words for `tiles` tiles in both formats (32-bit values / 42-bit values) + the ticket
// counter.  Returns the (masked) epoch of this call and the ticket base; grows the status arrays on demand.
int32_t ldb_chain_begin(ldb_ctx* ctx, uint64_t n_tiles, bool wide, ChainCall* c) {
   if (!ctx->chain.ticket) {
      LDB_HIP(hipMalloc((void**) &ctx->chain.ticket, 64));
      LDB_HIP(hipMemsetAsync(ctx->chain.ticket, 0, 64, ctx->stream));
      ctx->chain.ticket_base = 0;
   }
   if (n_tiles > ctx->chain.status_tiles) {
      size_t want = 4096;
      while (want < n_tiles) want *= 2;
      uint64_t* fresh = nullptr;
      LDB_HIP(hipMallocAsync((void**) &fresh, 16 * want, ctx->stream)); // [0, want): 32-bit format, [want, 2 want): 42-bit format
      LDB_HIP(hipMemsetAsync(fresh, 0, 16 * want, ctx->stream));
      if (ctx->chain.status) (void) hipFreeAsync(ctx->chain.status, ctx->stream);
      ctx->chain.status = fresh;
      ctx->chain.status_tiles = want;
   }
   // epochs: 30 bits beside a 32-bit value, 20 bits beside a 42-bit value; epoch 0 is "never written".  When the narrower
   // counter wraps, the words are cleared once (a stale word of the same epoch would read as ready)
   ctx->chain.epoch++;
   const uint32_t mask = wide ? (1u << 20) - 1 : (1u << 30) - 1;
   if ((ctx->chain.epoch & ((1u << 20) - 1)) == 0) {
      LDB_HIP(hipMemsetAsync(ctx->chain.status, 0, 16 * ctx->chain.status_tiles, ctx->stream));
      ctx->chain.epoch++;
   }
   c->status = (unsigned long long*) ctx->chain.status + (wide ? ctx->chain.status_tiles : 0);
   c->ticket = ctx->chain.ticket;
   c->ticket_base = ctx->chain.ticket_base;
   c->epoch = ctx->chain.epoch & mask;
   ctx->chain.ticket_base += n_tiles;
   return LDB_OK;
}
// a launch that did not happen took no tickets: the host mirror of the counter is re-based (the next tile numbers must
// start at 0 again, or every later chain would wait for tiles that never run)
int32_t ldb_chain_failed(ldb_ctx* ctx) {
   (void) hipMemsetAsync(ctx->chain.ticket, 0, 64, ctx->stream);
   ctx->chain.ticket_base = 0;
   LDB_FAIL(LDB_ERR_HIP, "chained scan: the launch failed");
}
void ldb_chain_teardown(ldb_ctx* ctx) {
   if (ctx->chain.status) (void) hipFree(ctx->chain.status);
   if (ctx->chain.ticket) (void) hipFree(ctx->chain.ticket);
}

// the three-level scan (option scan_single_pass = 0, and the single-workgroup case): per-block sums → recursive scan → add back
template <typename T, typename TO, typename TT>
__global__ void k_scan_block(const T* __restrict__ in, TO* __restrict__ out, TO* __restrict__ block_sums, uint64_t n, TT* __restrict__ total) {
   __shared__ TO sh[256];
   const int ITEMS = 8;
   uint64_t base = (uint64_t) blockIdx.x * 256 * ITEMS + (uint64_t) threadIdx.x * ITEMS;
   TO v[ITEMS];
   TO sum = 0;
#pragma unroll
   for (int k = 0; k < ITEMS; k++) {
      v[k] = base + k < n ? (TO) in[base + k] : (TO) 0;
      sum += v[k];
   }
   sh[threadIdx.x] = sum;
   __syncthreads();
   for (int off = 1; off < 256; off <<= 1) {
      TO t = threadIdx.x >= (unsigned) off ? sh[threadIdx.x - off] : (TO) 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
   }
   TO excl = sh[threadIdx.x] - sum;
   if (threadIdx.x == 255) {
      if (block_sums) block_sums[blockIdx.x] = sh[255];
      if (total && gridDim.x == 1) *total = (TT) sh[255]; // the last level of the recursion holds the grand total
   }
#pragma unroll
   for (int k = 0; k < ITEMS; k++) {
      if (base + k < n) out[base + k] = excl;
      excl += v[k];
   }
}
template <typename TO>
__global__ void k_scan_add(TO* __restrict__ out, const TO* __restrict__ block_offsets, uint64_t n) {
   const int ITEMS = 8;
   uint64_t base = (uint64_t) blockIdx.x * 256 * ITEMS + (uint64_t) threadIdx.x * ITEMS;
   TO add = block_offsets[blockIdx.x];
#pragma unroll
   for (int k = 0; k < ITEMS; k++)
      if (base + k < n) out[base + k] += add;
}
template <typename T, typename TO, typename TT, int VBITS>
static int32_t scan_impl(ldb_ctx* ctx, const T* d_in, TO* d_out, int64_t n, TT* d_total) {
   if (n <= 0) {
      if (d_total) LDB_HIP(hipMemsetAsync(d_total, 0, sizeof(TT), ctx->stream));
      return LDB_OK;
   }
   const int64_t per_block = 256 * 8;
   int64_t nb = (n + per_block - 1) / per_block;
   if (nb > 1 && ldb_option("scan_single_pass", 1) != 0) {
      ChainCall c;
      LDB_TRY(ldb_chain_begin(ctx, (uint64_t) nb, VBITS > 32, &c));
      hipLaunchKernelGGL((k_scan_chain<T, TO, TT, VBITS>), dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_in, d_out, (uint64_t) n, (uint64_t) nb, d_total, c.status, c.ticket, c.ticket_base,
                         c.epoch);
      if (hipGetLastError() != hipSuccess) return ldb_chain_failed(ctx);
      return LDB_OK;
   }
   LdbBufs tmp(ctx);
   TO* sums = nullptr;
   if (nb > 1) LDB_TRY(tmp.alloc(&sums, sizeof(TO) * (size_t) (nb + 1)));
   hipLaunchKernelGGL((k_scan_block<T, TO, TT>), dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_in, d_out, sums, (uint64_t) n, d_total);
   if (nb > 1) {
      TO* sums_scanned;
      LDB_TRY(tmp.alloc(&sums_scanned, sizeof(TO) * (size_t) (nb + 1)));
      LDB_TRY((scan_impl<TO, TO, TT, VBITS>(ctx, sums, sums_scanned, nb, d_total)));
      hipLaunchKernelGGL((k_scan_add<TO>), dim3((unsigned) nb), dim3(256), 0, ctx->stream, d_out, sums_scanned, (uint64_t) n);
   }
   LDB_HIP(hipGetLastError());
   return LDB_OK;
}
int32_t ldb_exclusive_scan_u32(ldb_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, int64_t n, uint64_t* d_total) {
   // the running sums are 32-bit (callers bound their totals by the uint32 row-id space); the total is stored widened
   return scan_impl<uint32_t, uint32_t, uint64_t, 32>(ctx, d_in, d_out, n, d_total);
}
int32_t ldb_exclusive_scan_i64(ldb_ctx* ctx, const int64_t* d_in, int64_t* d_out, int64_t n, int64_t* d_total) {
   // non-negative inputs (string lengths) whose total stays below 2^42 bytes — 15 x the HBM of one MI355X
   return scan_impl<int64_t, int64_t, int64_t, 42>(ctx, d_in, d_out, n, d_total);
}

// ---------------------------------------------------------------- bitmap → ascending row numbers, one launch
// A selection bitmap (one bit per row: ballot words of a probe / filter kernel) becomes the ascending list of set positions:
// popcount, chained scan (above) and expansion in ONE kernel — the word_pop + scan + expand sequence it replaces was five to
// seven launches and two temporaries per join.  A tile is 256 * BC_ITEMS words; its words and their offsets inside the tile
// go to LDS and are expanded by d_expand_tile (ldb_expand.h: row ids staged in LDS, then streamed out coalesced) — the same
// path at every density.  With `match` the kernel also writes second[j] = match[row] (the build row of a unique-key join's
// j-th result pair).  Entries [total, cap) are filled with row 0, so that a consumer that was sized from a REPLAYED count
// (ldb_readback) never meets an uninitialised row id.
// (the offsets are tile-local, so they are written before the look-back: the wait for the predecessors covers no work of the tile's own)
// (tile widths: ldb_bitmap_compact below)
template <int BC_ITEMS>
__global__ __launch_bounds__(256) void k_bitmap_compact(const uint64_t* __restrict__ bitmap, uint64_t n_words, uint64_t n_tiles, uint32_t* __restrict__ out, uint64_t cap,
                                                        const uint32_t* __restrict__ match, uint32_t* __restrict__ second, unsigned long long* __restrict__ total,
                                                        unsigned long long* __restrict__ status, unsigned long long* __restrict__ ticket, unsigned long long ticket_base,
                                                        unsigned long long epoch, uint32_t direct_min) {
   __shared__ unsigned long long s_tile;
   __shared__ uint32_t s_wave[4];
   __shared__ uint32_t s_prefix;
   constexpr uint32_t BC_TILE = 256 * BC_ITEMS;
   __shared__ __attribute__((aligned(16))) unsigned char s_lds[EXPAND_LDS_BYTES(BC_ITEMS)];
   if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1ull) - ticket_base;
   __syncthreads();
   const uint64_t tile = s_tile;
   const uint64_t word0 = tile * BC_TILE;
   const uint32_t agg = d_expand_load_scan<BC_ITEMS>(bitmap, word0, n_words, s_lds, s_wave);
   if (threadIdx.x < 64) {
      const uint32_t prefix = d_chain_prefix<uint32_t, 32>(status, tile, epoch, agg, threadIdx.x);
      if (threadIdx.x == 0) s_prefix = prefix;
   }
   __syncthreads();
   const uint32_t tile_base = s_prefix;
   if (tile == n_tiles - 1 && threadIdx.x == 0) {
      if (total) *total = (unsigned long long) tile_base + agg;
   }
   d_expand_tile<BC_ITEMS>(s_lds, agg, direct_min, (uint32_t) (word0 * 64), tile_base, out, cap, match, second);
   if (tile == n_tiles - 1) { // the tail behind the real count (see above)
      const uint64_t end = (uint64_t) tile_base + agg;
      for (uint64_t i = end + threadIdx.x; i < cap; i += 256) {
         out[i] = 0;
         if (match) second[i] = 0;
      }
   }
}
int32_t ldb_bitmap_compact(ldb_ctx* ctx, const uint64_t* bitmap, int64_t n_words, uint32_t* out, uint64_t cap, const uint32_t* match, uint32_t* second, uint64_t* d_total) {
   if (n_words <= 0) {
      if (d_total) LDB_HIP(hipMemsetAsync(d_total, 0, 8, ctx->stream));
      return LDB_OK;
   }
   // two words per thread where the bitmap is short, four or eight from 2 048 larger tiles on: a tile costs a fixed latency (ticket, loads, block scan,
   // look-back) whatever it holds.  Measured again with the staged expansion (256 M rows, profiles/expand_sweep.json): eight words win below 5 % set
   // (46 against 71 and 114 µs at 0.1 %), four from 50 % on (441 against 514 µs); joins compact a few per cent, so the defaults stand.
   const int64_t wide = ldb_option("compact_wide_tiles", 1); // 0 = two words per thread always, 1 = the default floor of 2 048 tiles, n > 1 = that floor
   const int64_t floor_tiles = wide > 1 ? wide : 2048;
   const int64_t most = ldb_option("compact_max_words", 8);
   const int items = !wide ? 2 : n_words >= floor_tiles * 256 * 16 && most >= 16 ? 16 : n_words >= floor_tiles * 256 * 8 ? 8 : n_words >= floor_tiles * 256 * 4 ? 4 : 2;
   const uint64_t n_tiles = ((uint64_t) n_words + 256u * items - 1) / (256u * items);
   ChainCall c;
   LDB_TRY(ldb_chain_begin(ctx, n_tiles, false, &c));
   LdbProf prof_(ctx, "k_bitmap_compact");
#define LDB_BC_LAUNCH(I) \
   hipLaunchKernelGGL(k_bitmap_compact<I>, dim3((unsigned) n_tiles), dim3(256), 0, ctx->stream, bitmap, (uint64_t) n_words, n_tiles, out, cap, match, second, (unsigned long long*) d_total, c.status, \
                      c.ticket, c.ticket_base, c.epoch, ldb_expand_direct_min(I, match != nullptr))
   if (items == 16) LDB_BC_LAUNCH(16);
   else if (items == 8) LDB_BC_LAUNCH(8);
   else if (items == 4) LDB_BC_LAUNCH(4);
   else LDB_BC_LAUNCH(2);
#undef LDB_BC_LAUNCH
   if (hipGetLastError() != hipSuccess) return ldb_chain_failed(ctx);
   return LDB_OK;
}
