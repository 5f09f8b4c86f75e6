// ldb_mem.hip — device memory of a context: block cache in front of the stream-ordered pool (ldb_dev_alloc / _free / _share),
// descriptor cache (ldb_dev_upload), pinned staging ring (ldb_h2d_small), and their statistics.
#include "ldb_internal.h"
#include <algorithm>
#include <cstdlib>
#include <functional>

// ---------------------------------------------------------------- memory
// size classes of the block cache: 8 per doubling (≤ 12.5 % internal waste), 256 B minimum
static size_t ldb_size_class(size_t bytes) {
   if (bytes <= 256) return 256;
   const int lg = 63 - __builtin_clzll((unsigned long long) (bytes - 1));
   const size_t step = (size_t) 1 << (lg >= 3 ? lg - 3 : 0);
   return (bytes + step - 1) / step * step;
}
static void ldb_cache_release(ldb_ctx* ctx) {
   for (auto& kv : ctx->mem.parked)
      for (void* p : kv.second) (void) hipFreeAsync(p, ctx->stream);
   ctx->mem.parked.clear();
   ctx->mem.parked_bytes = 0;
}
int32_t ldb_dev_alloc(ldb_ctx* ctx, void** out, size_t bytes) {
   // 16 bytes of slack behind every buffer: string kernels read through an 8-byte window (d_bytes8)
   const size_t cls = ctx->mem.cache_on ? ldb_size_class(bytes + 16) : bytes + 16;
   if (ctx->mem.cache_on) {
      auto it = ctx->mem.parked.find(cls);
      if (it != ctx->mem.parked.end() && !it->second.empty()) {
         // the LOWEST parked address of the class (min-heap): which block an allocation gets then depends only on the set of
         // free blocks, not on the order they were freed in — a plan that runs again finds its buffers at the same addresses,
         // so its descriptors are byte-identical (ldb_dev_upload's cache) from the second execution on
         std::pop_heap(it->second.begin(), it->second.end(), std::greater<void*>());
         *out = it->second.back();
         it->second.pop_back();
         ctx->mem.parked_bytes -= cls;
         ctx->mem.live[*out] = cls;
         return LDB_OK;
      }
   }
   hipError_t e;
   {
      LdbSlow slow_("hipMallocAsync", cls);
      e = hipMallocAsync(out, cls, ctx->stream);
   }
   if (e != hipSuccess && ctx->mem.parked_bytes) { // the parked blocks are the only memory we can give back
      (void) hipGetLastError();
      ldb_cache_release(ctx);
      (void) hipStreamSynchronize(ctx->stream);
      e = hipMallocAsync(out, cls, ctx->stream);
   }
   LDB_HIP(e);
   if (ctx->mem.cache_on) ctx->mem.live[*out] = cls;
   return LDB_OK;
}
void ldb_dev_free(ldb_ctx* ctx, void* p) {
   if (!p) return;
   auto dref = ctx->mem.desc_blocks.find(p);
   if (dref != ctx->mem.desc_blocks.end()) { // a cached descriptor (ldb_dev_upload): owned by the cache, this holder is done with it
      if (dref->second > 0) dref->second--;
      else {
         ctx->mem.desc_underflows++; // nobody held it: the count stays at 0 (never negative), and another holder's reference is not touched
         if (ldb_host_trace_threshold() >= 0) fprintf(stderr, "[ldb] descriptor %p given back twice\n", p);
      }
      return;
   }
   if (!ctx->mem.shared.empty()) {
      auto sh = ctx->mem.shared.find(p);
      if (sh != ctx->mem.shared.end()) { // another relation still reads this vector
         if (--sh->second == 0) ctx->mem.shared.erase(sh);
         return;
      }
   }
   auto it = ctx->mem.live.find(p);
   if (it == ctx->mem.live.end()) {
      LdbSlow slow_("hipFreeAsync (untracked block)");
      (void) hipFreeAsync(p, ctx->stream);
      return;
   }
   const size_t cls = it->second;
   ctx->mem.live.erase(it);
   if (ctx->mem.parked_bytes + cls <= ctx->mem.parked_cap) {
      auto& heap = ctx->mem.parked[cls];
      heap.push_back(p);
      std::push_heap(heap.begin(), heap.end(), std::greater<void*>());
      ctx->mem.parked_bytes += cls;
   } else {
      LdbSlow slow_("hipFreeAsync (cache full)", cls);
      (void) hipFreeAsync(p, ctx->stream);
   }
}
void ldb_dev_share(ldb_ctx* ctx, void* p) {
   if (p) ctx->mem.shared[p]++;
}
// Descriptor cache.  A plan that runs again builds byte-identical descriptors (same operators over the same buffers: the
// block cache above hands out the same addresses), so the device copy made by the previous execution can be used as it is:
// no staging, no H2D copy, no allocation.  Entries are keyed by a 64-bit content hash and verified by memcmp; kernels take
// descriptors as `const D*`, nothing on the device ever writes one.  ldb_dev_free recognises a cached block and leaves it
// alone (it only gives its reference back).  Bounded (desc_cache_mb, default 64 MB): when full, every entry that no operator
// holds any more is dropped (stream-ordered frees, so launches already queued are unaffected).  Option desc_cache = 0 switches it off.
static uint64_t desc_hash(const void* p, size_t bytes) {
   const uint8_t* b = (const uint8_t*) p;
   uint64_t h = 0x9E3779B97F4A7C15ull ^ bytes;
   size_t i = 0;
   for (; i + 8 <= bytes; i += 8) {
      uint64_t w;
      memcpy(&w, b + i, 8);
      h = (h ^ w) * 0xFF51AFD7ED558CCDull;
      h ^= h >> 29;
   }
   for (; i < bytes; i++) h = (h ^ b[i]) * 0x100000001B3ull;
   return h ^ (h >> 32);
}
// eviction: only entries no operator holds (reference count 0 — every ldb_dev_upload is paired with an ldb_dev_free of the pointer it
// returned); an entry that is still referenced keeps its device copy and its place in the cache, so a pointer handed out earlier never
// dangles and is never freed twice.  `force` (context teardown) drops everything.
static void desc_cache_drop(ldb_ctx* ctx, bool force = false) {
   for (auto it = ctx->mem.desc_cache.begin(); it != ctx->mem.desc_cache.end();) {
      auto ref = ctx->mem.desc_blocks.find(it->second.dev);
      if (!force && ref != ctx->mem.desc_blocks.end() && ref->second > 0) {
         ++it;
         continue;
      }
      (void) hipFreeAsync(it->second.dev, ctx->stream);
      ctx->mem.desc_bytes -= std::min(ctx->mem.desc_bytes, it->second.copy.size());
      if (ref != ctx->mem.desc_blocks.end()) ctx->mem.desc_blocks.erase(ref);
      it = ctx->mem.desc_cache.erase(it);
   }
   if (force) {
      ctx->mem.desc_blocks.clear();
      ctx->mem.desc_bytes = 0;
   }
}
int32_t ldb_h2d_small(ldb_ctx* ctx, void* dev, const void* host, size_t bytes) {
   // descriptors (a few KB) are staged through a pinned ring so that the copy is a plain async DMA
   // (a pageable source makes the runtime stage it synchronously, ~10 µs per call); `host` may be a
   // local either way.  A slot is reused only after the stream has drained (wrap → synchronize).
   const size_t need = (bytes + 63) & ~(size_t) 63;
   if (ctx->mem.h_ring && need <= LDB_RING_BYTES / 8) {
      if (ctx->mem.ring_pos + need > LDB_RING_BYTES) {
         LdbSlow slow_("staging ring wrap: hipStreamSynchronize");
         LDB_HIP(hipStreamSynchronize(ctx->stream));
         ctx->mem.ring_pos = 0;
      }
      void* slot = ctx->mem.h_ring + ctx->mem.ring_pos;
      ctx->mem.ring_pos += need;
      memcpy(slot, host, bytes);
      LDB_HIP(hipMemcpyAsync(dev, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
      return LDB_OK;
   }
   LDB_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
   return LDB_OK;
}
int32_t ldb_dev_upload(ldb_ctx* ctx, const void* host, size_t bytes, void** dev_out, bool cacheable) {
   const bool cache_wanted = ldb_option("desc_cache", 1) != 0;
   if (cacheable && cache_wanted && bytes >= 64 && bytes <= (64u << 10)) {
      const uint64_t h = desc_hash(host, bytes);
      auto range = ctx->mem.desc_cache.equal_range(h);
      for (auto it = range.first; it != range.second; ++it)
         if (it->second.copy.size() == bytes && memcmp(it->second.copy.data(), host, bytes) == 0) {
            *dev_out = it->second.dev;
            ctx->mem.desc_blocks[it->second.dev]++;
            ctx->mem.desc_hits++;
            return LDB_OK;
         }
      const size_t cap = (size_t) ldb_option("desc_cache_mb", 64) << 20;
      if (ctx->mem.desc_bytes + bytes > cap) desc_cache_drop(ctx);
      void* dev = nullptr;
      LDB_TRY(ldb_dev_alloc(ctx, &dev, bytes)); // from the block cache; the cache entry takes it out of circulation
      ctx->mem.live.erase(dev);
      int32_t st = ldb_h2d_small(ctx, dev, host, bytes);
      if (st != LDB_OK) {
         (void) hipFreeAsync(dev, ctx->stream);
         return st;
      }
      ldb_mem_state::DescEntry e;
      e.dev = dev;
      e.copy.assign((const uint8_t*) host, (const uint8_t*) host + bytes);
      ctx->mem.desc_cache.emplace(h, std::move(e));
      ctx->mem.desc_blocks[dev] = 1;
      ctx->mem.desc_bytes += bytes;
      ctx->mem.desc_misses++;
      *dev_out = dev;
      return LDB_OK;
   }
   LDB_TRY(ldb_dev_alloc(ctx, dev_out, bytes));
   return ldb_h2d_small(ctx, *dev_out, host, bytes);
}

// ---------------------------------------------------------------- set-up and teardown with the context
int32_t ldb_mem_init(ldb_ctx* ctx) {
   // keep freed blocks cached in the stream-ordered pool (operators allocate per call)
   hipMemPool_t pool;
   if (hipDeviceGetDefaultMemPool(&pool, ctx->device) == hipSuccess) {
      uint64_t thr = UINT64_MAX;
      (void) hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
   }
   const char* cache_env = getenv("LDB_ALLOC_CACHE");
   ctx->mem.cache_on = !(cache_env && cache_env[0] == '0');
   size_t hbm_free = 0, hbm_total = 0;
   if (hipMemGetInfo(&hbm_free, &hbm_total) == hipSuccess) ctx->mem.parked_cap = hbm_total / 4;
   LDB_HIP(hipHostMalloc((void**) &ctx->mem.h_ring, LDB_RING_BYTES, hipHostMallocDefault));
   return LDB_OK;
}
void ldb_mem_release_blocks(ldb_ctx* ctx) {
   desc_cache_drop(ctx, true);
   ldb_cache_release(ctx);
}
void ldb_mem_teardown(ldb_ctx* ctx) {
   if (ctx->mem.h_ring) (void) hipHostFree(ctx->mem.h_ring);
}
extern "C" int32_t ldb_gpu_desc_cache_held(ldb_ctx* ctx, int64_t* held, int64_t* underflows) {
   if (!ctx) LDB_FAIL(LDB_ERR_INVALID, "desc_cache_held: NULL ctx");
   int64_t n = 0;
   for (auto& b : ctx->mem.desc_blocks) n += b.second;
   if (held) *held = n;
   if (underflows) *underflows = ctx->mem.desc_underflows;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_mem_stats(ldb_ctx* ctx, int64_t* live_blocks, int64_t* live_bytes, int64_t* parked_bytes) {
   if (!ctx) LDB_FAIL(LDB_ERR_INVALID, "mem_stats: NULL ctx");
   int64_t blocks = 0, bytes = 0;
   for (auto& b : ctx->mem.live)
      if (!ctx->mem.desc_blocks.count(b.first)) {
         blocks++;
         bytes += (int64_t) b.second;
      }
   if (live_blocks) *live_blocks = blocks;
   if (live_bytes) *live_bytes = bytes;
   if (parked_bytes) *parked_bytes = (int64_t) ctx->mem.parked_bytes;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_desc_cache_stats(ldb_ctx* ctx, int64_t* hits, int64_t* misses, int64_t* bytes) {
   if (!ctx) LDB_FAIL(LDB_ERR_INVALID, "desc_cache_stats: NULL ctx");
   if (hits) *hits = ctx->mem.desc_hits;
   if (misses) *misses = ctx->mem.desc_misses;
   if (bytes) *bytes = (int64_t) ctx->mem.desc_bytes;
   return LDB_OK;
}
