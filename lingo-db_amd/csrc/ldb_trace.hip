// ldb_trace.hip — device → host read-backs and their trace (what a prepared plan records and replays, ldb_internal.h:
// ldb_readback), the counter arena the read values mostly live in, the registry of read-back sites.
#include "ldb_internal.h"
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>

// ---------------------------------------------------------------- read-backs (ldb_internal.h: ldb_readback)
// copies `bytes` (a multiple of 4 after padding) from device memory into the pinned log; one wave
__global__ void k_log_copy(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t bytes) {
   for (uint32_t i = threadIdx.x; i < bytes; i += blockDim.x) dst[i] = src[i];
}
// the deferred copies of a replaying trace: one kernel gathers every pending (source, bytes) into the pinned log
struct DLogList {
   uint32_t n, pad;
   ldb_rb_state::LogCopy e[255];
};
__global__ void k_log_gather(const DLogList* __restrict__ l, uint8_t* __restrict__ log) {
   for (uint32_t i = 0; i < l->n; i++) {
      const uint8_t* src = (const uint8_t*) l->e[i].src;
      for (uint32_t b = threadIdx.x; b < l->e[i].bytes; b += blockDim.x) log[l->e[i].off + b] = src[b];
   }
}
static int32_t log_flush(ldb_ctx* ctx) {
   size_t at = 0;
   while (at < ctx->rb.log_pending.size()) {
      auto l = std::make_unique<DLogList>();
      memset(l.get(), 0, sizeof(DLogList));
      l->n = (uint32_t) std::min<size_t>(255, ctx->rb.log_pending.size() - at);
      for (uint32_t i = 0; i < l->n; i++) l->e[i] = ctx->rb.log_pending[at + i];
      at += l->n;
      LdbDesc<DLogList> d(ctx);
      LDB_TRY(d.upload(l.get(), 8 + sizeof(ldb_rb_state::LogCopy) * l->n)); // (the same list every execution: served by the descriptor cache)
      hipLaunchKernelGGL(k_log_gather, dim3(1), dim3(64), 0, ctx->stream, (const DLogList*) d.p, ctx->rb.h_log);
   }
   ctx->rb.log_pending.clear();
   LDB_HIP(hipGetLastError());
   return LDB_OK;
}
int32_t ldb_counters(ldb_ctx* ctx, int n_words, uint64_t** out) {
   const size_t need = ((size_t) n_words + 7) & ~(size_t) 7;
   if (!ctx->rb.arena) {
      LDB_HIP(hipMalloc((void**) &ctx->rb.arena, 8 * LDB_ARENA_WORDS));
      LDB_HIP(hipMemsetAsync(ctx->rb.arena, 0, 8 * LDB_ARENA_WORDS, ctx->stream));
      ctx->rb.arena_pos = 0;
   }
   if (need > LDB_ARENA_WORDS) LDB_FAIL(LDB_ERR_INVALID, "ldb_counters: %d words", n_words);
   if (ctx->rb.arena_pos + need > LDB_ARENA_WORDS) { // wrap: what a replaying trace still wants from the old words is collected first
      LDB_TRY(log_flush(ctx));
      // words handed out earlier may not have been read back yet (a caller that allocates, launches and meets a nested allocation
      // before its read-back): nothing is cleared wholesale — from here until the next restart every allocation clears its own range
      ctx->rb.arena_wrapped = true;
      ctx->rb.arena_pos = 0;
   }
   *out = ctx->rb.arena + ctx->rb.arena_pos;
   if (ctx->rb.arena_wrapped) LDB_HIP(hipMemsetAsync(*out, 0, 8 * need, ctx->stream));
   ctx->rb.arena_pos += need;
   return LDB_OK;
}
// a plan starts at word 0 (the same words every execution → byte-identical descriptors): one clear of what the last one used
static int32_t arena_restart(ldb_ctx* ctx) {
   if (ctx->rb.arena && (ctx->rb.arena_pos || ctx->rb.arena_wrapped)) LDB_HIP(hipMemsetAsync(ctx->rb.arena, 0, 8 * (ctx->rb.arena_wrapped ? (size_t) LDB_ARENA_WORDS : ctx->rb.arena_pos), ctx->stream));
   ctx->rb.arena_pos = 0;
   ctx->rb.arena_wrapped = false;
   return LDB_OK;
}
static int32_t readback_sync(ldb_ctx* ctx, void* host, const void* dev, size_t bytes) {
   LdbSlow slow_("read-back with a stream wait", bytes);
   if (bytes <= 512 && ctx->h_scratch) { // a pinned landing area: the copy is a plain DMA / blit, no staging by the runtime
      LDB_HIP(hipMemcpyAsync(ctx->h_scratch, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
      LDB_HIP(hipStreamSynchronize(ctx->stream));
      memcpy(host, ctx->h_scratch, bytes);
      return LDB_OK;
   }
   LDB_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
   LDB_HIP(hipStreamSynchronize(ctx->stream));
   return LDB_OK;
}
static std::mutex g_site_mu;
static std::unordered_map<uint32_t, std::string> g_sites;
uint32_t ldb_site_note(uint32_t hash, const char* file, int line) {
   std::lock_guard<std::mutex> lock(g_site_mu);
   auto it = g_sites.find(hash);
   if (it == g_sites.end()) {
      const char* base = strrchr(file, '/');
      g_sites.emplace(hash, std::string(base ? base + 1 : file) + ":" + std::to_string(line));
   }
   return hash;
}
uint32_t ldb_site_derived(uint32_t base, uint32_t salt) {
   const uint32_t hash = base ^ (salt * 2654435761u);
   if (ldb_host_trace_threshold() < 0) return hash; // (names are only ever printed under LDB_HOST_TRACE)
   std::lock_guard<std::mutex> lock(g_site_mu);
   if (!g_sites.count(hash)) {
      auto it = g_sites.find(base);
      g_sites.emplace(hash, (it != g_sites.end() ? it->second : std::string("?")) + " n=" + std::to_string(salt));
   }
   return hash;
}
static std::atomic<int64_t> g_order_misses{0};
extern "C" int64_t ldb_gpu_order_dependent_misses(void) { return g_order_misses.load(); }
// replay: everything read so far must equal the record
static bool trace_prefix_ok(ldb_ctx* ctx, size_t upto_entries) {
   LdbSlow slow_("trace check: wait for the replayed plan", upto_entries);
   if (log_flush(ctx) != LDB_OK) return false;
   if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
   const ldb_trace* t = ctx->rb.trace;
   for (size_t i = 0; i < upto_entries; i++) {
      const ldb_trace_entry& e = t->entries[i];
      if (memcmp(ctx->rb.h_log + e.off, t->vals.data() + e.off, e.bytes) != 0) {
         if (e.flags & LDB_RB_ORDER_DEPENDENT) g_order_misses.fetch_add(1);
         if (ldb_host_trace_threshold() >= 0) { // which read-back was it, and what did it say
            std::lock_guard<std::mutex> lock(g_site_mu);
            auto it = g_sites.find(e.site);
            unsigned long long rec[2] = {0, 0}, got[2] = {0, 0};
            memcpy(rec, t->vals.data() + e.off, std::min<size_t>(16, e.bytes));
            memcpy(got, ctx->rb.h_log + e.off, std::min<size_t>(16, e.bytes));
            fprintf(stderr, "[ldb host] replayed read-back %zu of %zu differs (%s, %u bytes): recorded %llx %llx, now %llx %llx\n", i, t->entries.size(),
                    it != g_sites.end() ? it->second.c_str() : "?", e.bytes, rec[0], rec[1], got[0], got[1]);
         }
         return false;
      }
   }
   return true;
}
int32_t ldb_readback(ldb_ctx* ctx, void* host, const void* dev, size_t bytes, uint32_t site, int flags) {
   if (bytes == 0) return LDB_OK;
   if (ctx->rb.mode == ldb_rb_mode::off || bytes > LDB_RB_MAX) return readback_sync(ctx, host, dev, bytes);
   // a mis-speculated execution is void.  Alone, the rank stops at once (LDB_ERR_RETRY); inside a COLLECTIVE trace (a plan that exchanges rows
   // with other ranks) it runs on over the recorded counts — its peers are queued against exactly those transfer sizes and would wait for ever
   // for a rank that left — and the verdict at the trace's end makes every rank repeat the execution
   if (ctx->rb.poisoned && !ctx->rb.collective) LDB_FAIL(LDB_ERR_RETRY, "read-back after a mis-speculated value (the plan execution is being repeated)");
   ldb_trace* t = ctx->rb.trace;
   if (flags & LDB_RB_NEVER_REPLAY) { // not a function of the data alone: read for real, in both modes, and keep out of the record
      if (ctx->rb.mode == ldb_rb_mode::replay && !ctx->rb.poisoned && !trace_prefix_ok(ctx, ctx->rb.pos)) {
         ctx->rb.poisoned = true;
         t->misses++;
         if (!ctx->rb.collective) LDB_FAIL(LDB_ERR_RETRY, "a replayed read-back differs from the recorded value");
      }
      return readback_sync(ctx, host, dev, bytes);
   }
   if (ctx->rb.mode == ldb_rb_mode::replay) {
      if (ctx->rb.pos < t->entries.size() && t->entries[ctx->rb.pos].site == site && t->entries[ctx->rb.pos].bytes == bytes) {
         const ldb_trace_entry& e = t->entries[ctx->rb.pos++];
         const uint64_t* w = (const uint64_t*) dev;
         if (ctx->rb.arena && w >= ctx->rb.arena && w < ctx->rb.arena + LDB_ARENA_WORDS) { // an arena word keeps its value until the plan ends: collected with the others
            ctx->rb.log_pending.push_back({(uint64_t) dev, e.off, (uint32_t) bytes});
         } else {
            hipLaunchKernelGGL(k_log_copy, dim3(1), dim3(64), 0, ctx->stream, (const uint8_t*) dev, ctx->rb.h_log + e.off, (uint32_t) bytes);
            LDB_HIP(hipGetLastError());
         }
         memcpy(host, t->vals.data() + e.off, bytes);
         return LDB_OK;
      }
      // the execution took another path than the recorded one (a statistic is cached now, an option changed …): what was
      // replayed so far is checked, and from here on the execution records
      if (ctx->rb.poisoned || !trace_prefix_ok(ctx, ctx->rb.pos)) {
         if (!ctx->rb.poisoned) t->misses++;
         ctx->rb.poisoned = true;
         if (!ctx->rb.collective) LDB_FAIL(LDB_ERR_RETRY, "a replayed read-back differs from the recorded value");
         // collective: a rank on void data easily leaves the recorded sequence (an empty input skips a read, a table overflows …).  Its peers are
         // still inside their exchanges, queued against this rank's transfers: abandoning the plan here would stall them until the communicator's
         // time-out (shm) or for good (RCCL).  It reads the real value — consistent with what is on the device now — leaves the record alone and
         // goes on to the end, where the agreed verdict makes every rank repeat the execution
         return readback_sync(ctx, host, dev, bytes);
      }
      t->diverged++;
      t->entries.resize(ctx->rb.pos);
      t->vals.resize(ctx->rb.pos ? t->entries.back().off + ((t->entries.back().bytes + 7) & ~7u) : 0);
      ctx->rb.mode = ldb_rb_mode::record;
   }
   LDB_TRY(readback_sync(ctx, host, dev, bytes));
   const size_t off = t->vals.size();
   if (off + bytes + 8 <= LDB_LOG_BYTES) {
      t->entries.push_back({site, (uint32_t) bytes, (uint32_t) off, (uint32_t) (flags & LDB_RB_ORDER_DEPENDENT)});
      t->vals.resize(off + ((bytes + 7) & ~(size_t) 7), 0);
      memcpy(t->vals.data() + off, host, bytes);
   } else {
      t->complete = false;
      ctx->rb.mode = ldb_rb_mode::off; // more read-backs than the log holds: this plan is never replayed
      t->entries.clear();
      t->vals.clear();
   }
   return LDB_OK;
}
int32_t ldb_read_u64_at(ldb_ctx* ctx, const void* d_word, uint64_t* out, uint32_t site, int flags) { return ldb_readback(ctx, out, d_word, 8, site, flags); }

extern "C" int32_t ldb_gpu_trace_create(ldb_ctx* ctx, ldb_trace** out) {
   if (!ctx || !out) LDB_FAIL(LDB_ERR_INVALID, "trace_create: NULL argument");
   *out = new ldb_trace();
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_trace_destroy(ldb_ctx* ctx, ldb_trace* t) {
   if (ctx && ctx->rb.trace == t) {
      ctx->rb.trace = nullptr;
      ctx->rb.mode = ldb_rb_mode::off;
   }
   delete t;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_trace_begin(ldb_ctx* ctx, ldb_trace* t, int32_t allow_replay) {
   if (!ctx || !t) LDB_FAIL(LDB_ERR_INVALID, "trace_begin: NULL argument");
   if (ctx->rb.mode != ldb_rb_mode::off) LDB_FAIL(LDB_ERR_INVALID, "trace_begin: a trace is already active on this context");
   if (!ctx->rb.h_log) LDB_HIP(hipHostMalloc((void**) &ctx->rb.h_log, LDB_LOG_BYTES, hipHostMallocDefault));
   const bool replay_wanted = ldb_option("plan_replay", 1) != 0;
   ctx->rb.trace = t;
   ctx->rb.pos = 0;
   ctx->rb.poisoned = false;
   ctx->rb.collective = (allow_replay & LDB_TRACE_COLLECTIVE) != 0;
   ctx->rb.log_pending.clear();
   LDB_TRY(arena_restart(ctx));
   if ((allow_replay & 1) && replay_wanted && t->complete && !t->entries.empty()) {
      ctx->rb.mode = ldb_rb_mode::replay;
   } else {
      ctx->rb.mode = ldb_rb_mode::record;
      t->entries.clear();
      t->vals.clear();
   }
   t->complete = false;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_trace_end(ldb_ctx* ctx, int32_t* status) {
   if (!ctx || !status) LDB_FAIL(LDB_ERR_INVALID, "trace_end: NULL argument");
   ldb_trace* t = ctx->rb.trace;
   const ldb_rb_mode mode = ctx->rb.mode;
   ctx->rb.trace = nullptr;
   ctx->rb.mode = ldb_rb_mode::off;
   ctx->rb.collective = false;
   if (!t || mode == ldb_rb_mode::off) {
      *status = LDB_TRACE_OFF;
      if (t) t->complete = false;
      return LDB_OK;
   }
   if (ctx->rb.poisoned) {
      ctx->rb.poisoned = false;
      t->complete = false;
      t->entries.clear();
      t->vals.clear();
      (void) hipStreamSynchronize(ctx->stream);
      *status = LDB_TRACE_MISSED;
      return LDB_OK;
   }
   if (mode == ldb_rb_mode::replay) {
      ctx->rb.trace = t;
      const bool ok = trace_prefix_ok(ctx, ctx->rb.pos);
      ctx->rb.trace = nullptr;
      if (!ok) {
         t->misses++;
         t->complete = false;
         t->entries.clear();
         t->vals.clear();
         *status = LDB_TRACE_MISSED;
         return LDB_OK;
      }
      if (ctx->rb.pos < t->entries.size()) { // ended earlier than the record: keep what was used
         t->entries.resize(ctx->rb.pos);
         t->vals.resize(ctx->rb.pos ? t->entries.back().off + ((t->entries.back().bytes + 7) & ~7u) : 0);
      }
      t->replays++;
      t->complete = true;
      *status = LDB_TRACE_REPLAYED;
      return LDB_OK;
   }
   t->records++;
   t->complete = true;
   *status = LDB_TRACE_RECORDED;
   return LDB_OK;
}
// would ldb_gpu_trace_begin(ctx, t, 1) replay?  (what the ranks of a sharded plan agree on BEFORE any of them begins: they replay together or not at all)
extern "C" int32_t ldb_gpu_trace_replayable(const ldb_trace* t) { return t && t->complete && !t->entries.empty() && ldb_option("plan_replay", 1) != 0 ? 1 : 0; }
extern "C" int32_t ldb_gpu_trace_stats(const ldb_trace* t, int64_t* entries, int64_t* records, int64_t* replays, int64_t* misses) {
   if (!t) LDB_FAIL(LDB_ERR_INVALID, "trace_stats: NULL trace");
   if (entries) *entries = (int64_t) t->entries.size();
   if (records) *records = t->records;
   if (replays) *replays = t->replays;
   if (misses) *misses = t->misses;
   return LDB_OK;
}
void ldb_trace_teardown(ldb_ctx* ctx) {
   if (ctx->rb.h_log) (void) hipHostFree(ctx->rb.h_log);
   if (ctx->rb.arena) (void) hipFree(ctx->rb.arena);
}
