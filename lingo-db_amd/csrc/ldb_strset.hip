// ldb_strset.hip — one conjunct over a utf8 column against constants the inline descriptor (DPred) cannot hold:
//   col IN (c_0 … c_{n-1})  with any n ≥ 0 and any constant lengths, and
//   col OP c                with OP ∈ EQ, NEQ, LT, LTE, GT, GTE and a constant of any length (the same kernel: a set of one).
// Replaces (reference): the hash set an IN restriction keeps (src/runtime/storage/Restrictions.cpp:481-515) and the
// std::string_view comparisons of its other filters — unsigned bytes first, then length (StringRuntime::compareLt, the order
// ldb_strminmax.hip states).
//
// Host: the constants are sorted in that order and deduplicated (ldb_gpu_strset_plan — no device needed, so the CPU tests pin it);
// one device block holds, per distinct constant, an order-preserving 64-bit key — its first 8 bytes, big-endian, zero padded
// (smm_key of ldb_strminmax.hip) — its length and its offset into the blob of all constants, then the blob.
// Device: a workgroup stages the keys and lengths in LDS when they fit (LDB_STRSET_LDS_MAX), else the same search reads them from
// global memory (a few thousand constants are cache resident).  Per row: the two offsets, the row's key from its first ≤ 8
// bytes (at most two aligned 8-byte loads), a binary search for the first constant whose key is not smaller.  The key is monotone
// but not strict ("ab" and "ab\0" share one), so the RUN of constants that tie on the key is walked: lengths are compared there,
// and only for equal lengths above 8 the bytes behind the eighth against the blob.  A non-member usually leaves after the search
// without touching its ninth byte.  Four rows are in flight per lane (offsets → bytes is a dependent load pair).
// The result is what k_scan_bitmap writes — one ballot word per 64 rows, passing rows per (part of a) 16 384-row block — so the
// prefix scan, the replayable count read-back and k_scan_expand of scan_run_with (ldb_scan.hip) serve it unchanged.
// Branches on the descriptor are wave-uniform; the per-row loops (search, tie run, byte compare) are private to a lane: no lane
// waits for another.
#include "ldb_internal.h"
#include "ldb_device.h"
#include "ldb_scan_kernel.h"
#include "ldb_strset.h"
#include <algorithm>
#include <memory>

struct DStrSet {
   uint64_t n_rows;
   DCol col;
   uint64_t keys; // const uint64_t[n_set], ascending
   uint64_t lens; // const uint32_t[n_set]
   uint64_t offs; // const uint32_t[n_set]: start of constant k in blob
   uint64_t blob; // const uint8_t[]
   int32_t n_set;
   int32_t op; // LDB_F_IN, or a comparison against constant 0 (n_set == 1)
};

// LDS table: 8 bytes of key + 4 bytes of length per constant.  A workgroup may use 64 KB; 1 KB is left for the kernel's own words
// (s_cnt) and the allocation granularity, and the rest is cut to a multiple of the block size: (65536 - 1024) / 12 = 5376 = 21 * 256.
static_assert(LDB_STRSET_LDS_MAX * 12 + 1024 <= 65536 && LDB_STRSET_LDS_MAX % SCAN_BLOCK == 0, "the staged table fits a workgroup's 64 KB");

// first min(len, 8) bytes of p, big-endian, zero padded.  The bytes come from the one or two ALIGNED 8-byte words that hold them: each
// word holds at least one byte of the string, and an aligned word never crosses a page, so nothing outside the buffer's pages is touched.
__device__ __forceinline__ uint64_t strset_row_key(const uint8_t* p, uint32_t len) {
   const uint32_t m = len < 8 ? len : 8;
   if (m == 0) return 0;
   const uint64_t addr = (uint64_t) p;
   const uint32_t sh = (uint32_t) (addr & 7);
   const uint64_t* a = gptr<uint64_t>(addr - sh);
   uint64_t raw = a[0] >> (8 * sh);
   if (sh + m > 8) raw |= a[1] << (64 - 8 * sh); // (sh ≥ 1 here)
   const uint64_t k = __builtin_bswap64(raw);
   return m < 8 ? k & ~(~0ull >> (8 * m)) : k;
}

// sign of (row string) - (constant) for two strings whose keys tie: the first min(8, both lengths) bytes are equal already
__device__ __forceinline__ int strset_cmp_tail(const uint8_t* p, uint32_t len, const uint8_t* c, uint32_t clen) {
   const uint32_t m = len < clen ? len : clen;
   for (uint32_t j = 8; j < m; j++) {
      const uint8_t a = p[j], b = c[j];
      if (a != b) return a < b ? -1 : 1;
   }
   return len < clen ? -1 : (len > clen ? 1 : 0);
}

template <typename KEYS, typename LENS>
__device__ __forceinline__ bool strset_member(KEYS keys, LENS lens, const uint32_t* __restrict__ offs, const uint8_t* __restrict__ blob, uint32_t n_set, uint64_t key,
                                              const uint8_t* p, uint32_t len) {
   uint32_t lo = 0, hi = n_set; // first constant whose key is >= key
   while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1;
      else hi = mid;
   }
   for (; lo < n_set && keys[lo] == key; lo++) { // the tie run
      if (lens[lo] != len) continue;
      if (len <= 8 || strset_cmp_tail(p, len, blob + offs[lo], len) == 0) return true;
   }
   return false;
}

__device__ __forceinline__ bool strset_apply(int32_t op, int sign) {
   switch (op) {
      case LDB_F_EQ: return sign == 0;
      case LDB_F_NEQ: return sign != 0;
      case LDB_F_LT: return sign < 0;
      case LDB_F_LTE: return sign <= 0;
      case LDB_F_GT: return sign > 0;
      default: return sign >= 0; // LDB_F_GTE
   }
}

template <bool LDS>
__device__ __forceinline__ void strset_bitmap_body(const DStrSet* __restrict__ d, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ block_counts, uint32_t* s_cnt,
                                                   uint64_t* s_keys, uint32_t* s_lens) {
   const uint64_t n = d->n_rows;
   const uint32_t n_set = (uint32_t) d->n_set;
   const int32_t op = d->op;
   const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const uint32_t wpb = SCAN_WORDS_PER_BLOCK / gridDim.y; // (the split of a short input: see scan_bitmap_body)
   const uint64_t word0 = (uint64_t) blockIdx.x * SCAN_WORDS_PER_BLOCK + (uint64_t) blockIdx.y * wpb;
   const uint64_t* g_keys = gptr<uint64_t>(d->keys);
   const uint32_t* g_lens = gptr<uint32_t>(d->lens);
   const uint32_t* offs = gptr<uint32_t>(d->offs);
   const uint8_t* blob = gptr<uint8_t>(d->blob);
   if (LDS) {
      for (uint32_t k = threadIdx.x; k < n_set; k += SCAN_BLOCK) {
         s_keys[k] = g_keys[k];
         s_lens[k] = g_lens[k];
      }
      __syncthreads();
   }
   const uint32_t* rowids = gptr<uint32_t>(d->col.rowids);
   const uint8_t* validity = gptr<uint8_t>(d->col.validity);
   const int64_t* o = gptr<int64_t>(d->col.offsets);
   const uint8_t* values = gptr<uint8_t>(d->col.values);
   // the one constant of a comparison (uniform)
   const uint64_t c_key = g_keys[0];
   const uint32_t c_len = g_lens[0];
   const uint8_t* c_ptr = blob + offs[0];
   uint32_t cnt = 0;
   constexpr uint32_t WPW = SCAN_BLOCK / LDB_WAVE;
   constexpr int U = 4; // (wpb is a multiple of U * WPW = 16: the split is at most 16 ways)
   for (uint32_t w = wave; w < wpb; w += U * WPW) {
      bool ok[U];
      uint32_t row[U], len[U];
      const uint8_t* p[U];
      uint64_t key[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
         const uint64_t i = (word0 + w + u * WPW) * 64 + lane;
         ok[u] = i < n;
         row[u] = ok[u] ? (rowids ? rowids[i] : (uint32_t) i) : 0;
         if (rowids && row[u] == LDB_NULL_ROW) ok[u] = false; // outer-join padding
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
         if (ok[u] && validity) ok[u] = (validity[row[u] >> 3] >> (row[u] & 7)) & 1;
         int64_t b = 0, e = 0;
         if (ok[u]) {
            b = o[row[u]];
            e = o[row[u] + 1];
         }
         p[u] = values + b;
         len[u] = (uint32_t) (e - b);
      }
#pragma unroll
      for (int u = 0; u < U; u++) key[u] = ok[u] ? strset_row_key(p[u], len[u]) : 0;
#pragma unroll
      for (int u = 0; u < U; u++) {
         bool pass = false;
         if (ok[u]) {
            if (op == LDB_F_IN) { // (uniform)
               if (LDS) pass = strset_member(s_keys, s_lens, offs, blob, n_set, key[u], p[u], len[u]);
               else pass = strset_member(g_keys, g_lens, offs, blob, n_set, key[u], p[u], len[u]);
            } else {
               const int sign = key[u] != c_key ? (key[u] < c_key ? -1 : 1) : strset_cmp_tail(p[u], len[u], c_ptr, c_len);
               pass = strset_apply(op, sign);
            }
         }
         const uint64_t mask = __ballot(pass);
         if (lane == 0 && (word0 + w + u * WPW) * 64 < n) bitmap[word0 + w + u * WPW] = mask;
         cnt += (uint32_t) __popcll(mask);
      }
   }
   if (lane == 0) s_cnt[wave] = cnt;
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t t = 0;
      for (int k = 0; k < SCAN_BLOCK / LDB_WAVE; k++) t += s_cnt[k];
      block_counts[blockIdx.x * gridDim.y + blockIdx.y] = t;
   }
}

// the table staged in LDS: dynamic shared memory of 12 bytes per constant (keys first: 8-byte aligned, then the lengths)
__global__ __launch_bounds__(SCAN_BLOCK) void k_strset_bitmap_lds(const DStrSet* __restrict__ d, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ block_counts) {
   __shared__ uint32_t s_cnt[SCAN_BLOCK / LDB_WAVE];
   extern __shared__ __attribute__((aligned(8))) uint8_t s_table[];
   uint64_t* s_keys = (uint64_t*) s_table;
   uint32_t* s_lens = (uint32_t*) (s_table + 8 * (size_t) d->n_set);
   strset_bitmap_body<true>(d, bitmap, block_counts, s_cnt, s_keys, s_lens);
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_strset_bitmap_glb(const DStrSet* __restrict__ d, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ block_counts) {
   __shared__ uint32_t s_cnt[SCAN_BLOCK / LDB_WAVE];
   strset_bitmap_body<false>(d, bitmap, block_counts, s_cnt, nullptr, nullptr);
}

// ---------------------------------------------------------------- host
static inline uint64_t strset_key(const char* s, int32_t len) {
   uint64_t k = 0;
   for (int j = 0; j < 8; j++) k = (k << 8) | (j < len ? (uint64_t) (uint8_t) s[j] : 0ull);
   return k;
}
// unsigned bytes, then length
static inline int strset_cmp(const char* a, int32_t la, const char* b, int32_t lb) {
   const int c = memcmp(a, b, (size_t) std::min(la, lb));
   return c ? c : (la < lb ? -1 : (la > lb ? 1 : 0));
}

extern "C" int32_t ldb_gpu_strset_plan(const char* const* strs, const int32_t* lens, int32_t n, int32_t* order, uint64_t* keys, int32_t* n_distinct, int32_t* in_lds, int32_t* lds_max) {
   if (n < 0 || (n > 0 && (!strs || !lens)) || !n_distinct) LDB_FAIL(LDB_ERR_INVALID, "strset_plan: bad argument");
   for (int32_t k = 0; k < n; k++)
      if (lens[k] < 0 || (lens[k] > 0 && !strs[k])) LDB_FAIL(LDB_ERR_INVALID, "strset_plan: constant %d: bad pointer or length", k);
   std::vector<int32_t> idx((size_t) n);
   for (int32_t k = 0; k < n; k++) idx[(size_t) k] = k;
   // (stable: of equal constants the first one listed stands for all)
   std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return strset_cmp(strs[a], lens[a], strs[b], lens[b]) < 0; });
   int32_t m = 0;
   for (int32_t k = 0; k < n; k++) {
      const int32_t i = idx[(size_t) k];
      if (m > 0 && strset_cmp(strs[idx[(size_t) m - 1]], lens[idx[(size_t) m - 1]], strs[i], lens[i]) == 0) continue;
      idx[(size_t) m++] = i;
   }
   for (int32_t k = 0; k < m; k++) {
      if (order) order[k] = idx[(size_t) k];
      if (keys) keys[k] = strset_key(strs[idx[(size_t) k]], lens[idx[(size_t) k]]);
   }
   *n_distinct = m;
   if (in_lds) *in_lds = m <= LDB_STRSET_LDS_MAX ? 1 : 0;
   if (lds_max) *lds_max = LDB_STRSET_LDS_MAX;
   return LDB_OK;
}

static bool strset_col_plain(const ldb_rel* r, const ldb_filter_desc* p) {
   if (p->col.side < 0 || (size_t) p->col.side >= r->sides.size()) return false;
   const ldb_table* t = r->sides[(size_t) p->col.side].table;
   if (p->col.col < 0 || (size_t) p->col.col >= t->cols.size()) return false;
   const ldb_column& c = t->cols[(size_t) p->col.col];
   if (c.type.type != LDB_T_UTF8) return false;
   // a dictionary-encoded column tests its codes instead (ldb_dict_rewrite_pred evaluates the predicate over the dictionary's own rows)
   return !(c.dict_codes && c.dict && ldb_option("dict_encode", 1) != 0);
}

bool ldb_strset_wanted(const ldb_rel* r, const ldb_filter_desc* p) {
   if (!p || p->rhs_kind != LDB_RHS_STRING) return false;
   if (p->op == LDB_F_IN) {
      if (p->n_in < 0 || (p->n_in > 0 && (!p->in_strs || !p->in_str_lens))) return false; // (ldb_make_dpred reports it)
      bool big = p->n_in > LDB_MAX_IN || p->n_in >= ldb_option("scan_strset_min_in", LDB_MAX_IN + 1);
      int64_t bytes = 0;
      for (int32_t k = 0; k < p->n_in; k++) {
         if (p->in_str_lens[k] < 0) return false;
         bytes += p->in_str_lens[k];
      }
      big = big || bytes > (int64_t) sizeof(DPred::in_blob);
      return big && strset_col_plain(r, p);
   }
   if (p->op >= LDB_F_EQ && p->op <= LDB_F_GTE) return p->str_len > LDB_STR_INLINE && p->str && strset_col_plain(r, p);
   return false;
}
bool ldb_strset_any(const ldb_rel* r, const ldb_filter_desc* preds, int32_t n_preds) {
   for (int32_t p = 0; preds && p < n_preds; p++)
      if (ldb_strset_wanted(r, &preds[p])) return true;
   return false;
}

int32_t ldb_strset_run(ldb_ctx* ctx, ldb_rel* in, const ldb_filter_desc* p, uint32_t** sel_out, uint64_t* total_out) {
   if (!in->pending.empty()) LDB_FAIL(LDB_ERR_INVALID, "scan: string-set conjunct over a lazy relation");
   const bool is_in = p->op == LDB_F_IN;
   const int32_t n_in = is_in ? p->n_in : 1;
   const char* one_str = p->str;
   const int32_t one_len = p->str_len;
   const char* const* strs = is_in ? p->in_strs : &one_str;
   const int32_t* lens = is_in ? p->in_str_lens : &one_len;
   std::vector<int32_t> order((size_t) std::max(n_in, 1));
   std::vector<uint64_t> keys((size_t) std::max(n_in, 1));
   int32_t m = 0, in_lds = 0;
   LDB_TRY(ldb_gpu_strset_plan(strs, lens, n_in, order.data(), keys.data(), &m, &in_lds, nullptr));
   DStrSet h;
   memset(&h, 0, sizeof(h));
   h.n_rows = (uint64_t) in->n_rows;
   LDB_TRY(ldb_make_dcol(in, p->col, &h.col));
   h.n_set = m;
   h.op = p->op;
   const int64_t n = m == 0 ? 0 : in->n_rows; // an empty list passes nothing: no kernel
   LdbDesc<uint8_t> table(ctx);
   LdbDesc<DStrSet> desc(ctx);
   if (n) {
      // one block: keys | lengths | offsets | blob
      uint64_t blob_bytes = 0;
      for (int32_t k = 0; k < m; k++) blob_bytes += (uint64_t) lens[order[(size_t) k]];
      if (blob_bytes > 0x7FFFFFFFull) LDB_FAIL(LDB_ERR_UNSUPPORTED, "scan: the string constants of one conjunct total %llu bytes (their offsets are 32-bit: at most 2 GiB)", (unsigned long long) blob_bytes);
      const size_t at_lens = 8 * (size_t) m, at_offs = at_lens + 4 * (size_t) m, at_blob = at_offs + 4 * (size_t) m;
      std::vector<uint8_t> host((at_blob + (size_t) blob_bytes + 7) & ~(size_t) 7, 0);
      uint32_t pos = 0;
      for (int32_t k = 0; k < m; k++) {
         const int32_t i = order[(size_t) k];
         const uint32_t l = (uint32_t) lens[i];
         memcpy(host.data() + 8 * (size_t) k, &keys[(size_t) k], 8);
         memcpy(host.data() + at_lens + 4 * (size_t) k, &l, 4);
         memcpy(host.data() + at_offs + 4 * (size_t) k, &pos, 4);
         if (l) memcpy(host.data() + at_blob + pos, strs[i], l);
         pos += l;
      }
      LDB_TRY(table.upload(host.data(), host.size()));
      // a block too large for the pinned staging ring (128 KB: some 8 000 short constants) is copied from `host` itself, which dies with this call: wait for
      // the copy.  Inside a replayed plan that drains the queue once per such conjunct and execution — a cost only lists of that size pay (DESIGN.md §4 "String sets")
      if (((host.size() + 63) & ~(size_t) 63) > LDB_RING_BYTES / 8) LDB_HIP(hipStreamSynchronize(ctx->stream));
      h.keys = (uint64_t) table.p;
      h.lens = h.keys + at_lens;
      h.offs = h.keys + at_offs;
      h.blob = h.keys + at_blob;
      LDB_TRY(desc.upload(&h, sizeof(h)));
   }
   const DStrSet* d = desc.p;
   const unsigned lds_bytes = in_lds ? 12u * (unsigned) m : 0u;
   return ldb_scan_run_launch(ctx, n, [&](uint64_t* bitmap, uint32_t* counts, unsigned n_blocks, unsigned parts) -> int32_t {
      LdbProf prof_(ctx, in_lds ? "k_strset_bitmap_lds" : "k_strset_bitmap_glb");
      if (in_lds) hipLaunchKernelGGL(k_strset_bitmap_lds, dim3(n_blocks, parts), dim3(SCAN_BLOCK), lds_bytes, ctx->stream, d, bitmap, counts);
      else hipLaunchKernelGGL(k_strset_bitmap_glb, dim3(n_blocks, parts), dim3(SCAN_BLOCK), 0, ctx->stream, d, bitmap, counts);
      return LDB_OK;
   }, sel_out, total_out);
}
