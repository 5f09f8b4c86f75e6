// ldb_expand.h — a tile of selection-bitmap words → the ascending list of its set row numbers, for a workgroup of 256: the
// expansion shared by k_scan_expand (ldb_scan.hip) and k_bitmap_compact (ldb_prims.hip).
// A tile is 256 * ITEMS words; word w of the tile belongs to thread w % 256 (round w / 256).  The row ids go through an LDS
// staging buffer, EXPAND_CHUNK at a time: every thread drops the set bits of its own words at their output positions inside
// the chunk (LDS stores only), then the workgroup streams the chunk out — consecutive lanes write consecutive addresses, and
// with `match` every lane has EXPAND_GROUP independent gathers in flight.  That holds at every density but costs a dozen
// instructions per row id in the staging loop, and a chunk of a nearly full tile is 64 words: one wave's work.  A tile with at
// least `direct_min` set bits is therefore expanded a word per wave iteration straight from LDS: the lanes whose bit is set
// write one run, and a nearly full word's run is a whole coalesced store.  From which share of a tile's rows on: measured
// (tools/measure_expand.py, profiles/expand_sweep.json) — 50 % without `match`, 85 % with it (the staged form's gathers leave
// EXPAND_GROUP per lane at once and pay longer); option `expand_direct_pct` sets one share for both (0 = always, 101 = never).
#pragma once
#include "ldb_chain.h"
#include "ldb_device.h"
#define EXPAND_CHUNK 4096 // row ids staged per round (16 KB of LDS)
#define EXPAND_GROUP 4 // row ids per thread and streaming step
// LDS of a tile in bytes: its words (8 B) and offsets (4 B); the staging buffer takes their place once every thread holds its
// own words in registers
#define EXPAND_LDS_BYTES(ITEMS) (256 * (ITEMS) * 12 > EXPAND_CHUNK * 4 ? 256 * (ITEMS) * 12 : EXPAND_CHUNK * 4)
template <int ITEMS>
__device__ __forceinline__ uint64_t* d_expand_words(unsigned char* s_tile) { return (uint64_t*) s_tile; }
template <int ITEMS>
__device__ __forceinline__ uint32_t* d_expand_offsets(unsigned char* s_tile) { return (uint32_t*) (s_tile + 256 * ITEMS * 8); }

// Loads the tile's words (zero behind n_words) into s_tile (EXPAND_LDS_BYTES(ITEMS), 8-byte aligned) and leaves every word's
// exclusive offset INSIDE the tile beside them; returns the tile's number of set bits.  The caller puts a __syncthreads()
// between this and d_expand_tile.
template <int ITEMS>
__device__ __forceinline__ uint32_t d_expand_load_scan(const uint64_t* __restrict__ bitmap, uint64_t word0, uint64_t n_words, unsigned char* s_tile, uint32_t* s_wave) {
   uint64_t* s_words = d_expand_words<ITEMS>(s_tile);
   uint32_t* s_off = d_expand_offsets<ITEMS>(s_tile);
#pragma unroll
   for (int k = 0; k < ITEMS; k++) { // coalesced loads
      const uint64_t w = word0 + (uint64_t) k * 256 + threadIdx.x;
      const uint64_t m = w < n_words ? bitmap[w] : 0;
      s_words[k * 256 + threadIdx.x] = m;
      s_off[k * 256 + threadIdx.x] = (uint32_t) __popcll(m);
   }
   __syncthreads();
   // thread t scans words [ITEMS * t, ITEMS * t + ITEMS) of the tile (consecutive words → consecutive output positions)
   uint32_t own[ITEMS];
   uint32_t sum = 0;
#pragma unroll
   for (int k = 0; k < ITEMS; k++) {
      own[k] = s_off[threadIdx.x * ITEMS + k];
      sum += own[k];
   }
   uint32_t agg;
   uint32_t excl = d_block_scan256<uint32_t>(sum, s_wave, &agg); // (its barrier stands between the reads above and the writes below)
#pragma unroll
   for (int k = 0; k < ITEMS; k++) {
      s_off[threadIdx.x * ITEMS + k] = excl;
      excl += own[k];
   }
   return agg;
}

// the set bits a tile of 256 * items words needs for the word-per-wave expansion (host side)
inline uint32_t ldb_expand_direct_min(int items, bool with_match) {
   const int64_t set = ldb_option("expand_direct_pct", -1);
   const int64_t pct = set < 0 ? (with_match ? 85 : 50) : set > 101 ? 101 : set;
   return (uint32_t) ((int64_t) 256 * items * 64 * pct / 100);
}

// out[out_base + j] = the j-th set row of the tile (row0 = the row number of the tile's first bit), and with `match` also
// second[out_base + j] = match[that row]; nothing is written at or behind `cap`.  Called by all 256 threads; n_set, out_base,
// cap, match and direct_min are the same in every thread.
template <int ITEMS>
__device__ __forceinline__ void d_expand_tile(unsigned char* s_tile, uint32_t n_set, uint32_t direct_min, uint32_t row0, uint64_t out_base, uint32_t* __restrict__ out, uint64_t cap,
                                              const uint32_t* __restrict__ match, uint32_t* __restrict__ second) {
   const uint64_t* s_words = d_expand_words<ITEMS>(s_tile);
   const uint32_t* s_off = d_expand_offsets<ITEMS>(s_tile);
   if (n_set >= direct_min) { // nearly full: a word per wave iteration, EXPAND_GROUP words at a time
      const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      for (uint32_t w0 = wave; w0 < 256 * ITEMS; w0 += 4 * EXPAND_GROUP) {
         uint32_t row[EXPAND_GROUP];
         uint64_t at[EXPAND_GROUP];
         bool live[EXPAND_GROUP];
#pragma unroll
         for (int j = 0; j < EXPAND_GROUP; j++) {
            const uint32_t w = w0 + 4 * j;
            const uint64_t mm = s_words[w]; // wave-uniform
            at[j] = out_base + s_off[w] + d_rank_in(mm);
            live[j] = ((mm >> lane) & 1) && at[j] < cap;
            row[j] = live[j] ? row0 + w * 64 + lane : 0;
         }
         if (match) {
            uint32_t partner[EXPAND_GROUP];
#pragma unroll
            for (int j = 0; j < EXPAND_GROUP; j++) partner[j] = match[row[j]];
#pragma unroll
            for (int j = 0; j < EXPAND_GROUP; j++)
               if (live[j]) second[at[j]] = partner[j];
         }
#pragma unroll
         for (int j = 0; j < EXPAND_GROUP; j++)
            if (live[j]) out[at[j]] = row[j];
      }
      return;
   }
   uint32_t* s_stage = (uint32_t*) s_tile;
   // the bits not yet staged of the thread's words, and the tile position of the first of them
   uint64_t m[ITEMS];
   uint32_t pos[ITEMS];
#pragma unroll
   for (int k = 0; k < ITEMS; k++) {
      m[k] = s_words[k * 256 + threadIdx.x];
      pos[k] = s_off[k * 256 + threadIdx.x];
   }
   __syncthreads(); // from here on the tile's LDS is the staging buffer
   for (uint32_t c = 0; c < n_set; c += EXPAND_CHUNK) {
      if (c) __syncthreads(); // the chunk before this one has been streamed out
#pragma unroll
      for (int k = 0; k < ITEMS; k++) {
         uint64_t mm = m[k];
         if (!mm || pos[k] >= c + EXPAND_CHUNK) continue;
         const uint32_t row = row0 + (uint32_t) (k * 256 + threadIdx.x) * 64;
         uint32_t at = pos[k] - c; // (every bit in front of the chunk went out with an earlier one)
         while (mm && at < EXPAND_CHUNK) {
            s_stage[at++] = row + (uint32_t) __builtin_ctzll(mm);
            mm &= mm - 1;
         }
         m[k] = mm;
         pos[k] = c + at;
      }
      __syncthreads();
      const uint32_t n = n_set - c < EXPAND_CHUNK ? n_set - c : EXPAND_CHUNK;
      const uint64_t base = out_base + c;
      for (uint32_t g = 0; g < n; g += 256 * EXPAND_GROUP) {
         uint32_t row[EXPAND_GROUP];
         bool live[EXPAND_GROUP];
#pragma unroll
         for (int j = 0; j < EXPAND_GROUP; j++) {
            const uint32_t i = g + j * 256 + threadIdx.x;
            live[j] = i < n && base + i < cap; // (cap < the real count only under a wrong replayed count: never write past the buffer)
            row[j] = live[j] ? s_stage[i] : 0;
         }
         if (match) {
            uint32_t partner[EXPAND_GROUP];
#pragma unroll
            for (int j = 0; j < EXPAND_GROUP; j++) partner[j] = match[row[j]]; // unconditional (row 0 for an idle lane): the gathers leave together
#pragma unroll
            for (int j = 0; j < EXPAND_GROUP; j++)
               if (live[j]) second[base + g + j * 256 + threadIdx.x] = partner[j];
         }
#pragma unroll
         for (int j = 0; j < EXPAND_GROUP; j++)
            if (live[j]) out[base + g + j * 256 + threadIdx.x] = row[j];
      }
   }
}
