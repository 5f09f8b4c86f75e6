// ldb_core.hip — error text, process-wide options, the context (create / destroy / sync, device info), marker kernel, timers,
// per-kernel profiling.  Everything else a context owns lives with its subsystem: ldb_mem.hip (block cache, descriptor cache,
// staging ring), ldb_trace.hip (read-backs, their trace, the counter arena), ldb_prims.hip (scan chain).
// Replaces (reference): ExecutionContext (include/lingodb/runtime/ExecutionContext.h:62-127).
#include "ldb_internal.h"
#include <cstdlib>
#include <memory>

// ---------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";
void ldb_set_error(const char* fmt, ...) {
   va_list ap;
   va_start(ap, fmt);
   vsnprintf(g_err, sizeof(g_err), fmt, ap);
   va_end(ap);
}
extern "C" const char* ldb_gpu_last_error(void) { return g_err; }

// ---------------------------------------------------------------- options
// Process-wide tuning knobs: first read comes from the environment (LDB_<NAME>), later
// ldb_gpu_set_option calls override it — so a test can run the same process through both the
// generic and the run-time specialised / lazily fused code paths.
#include <atomic>
#include <functional>
#include <mutex>
static std::mutex g_opt_mu;
static std::atomic<int64_t> g_option_epoch{0}; // bumped by every ldb_gpu_set_option: a prepared plan recorded under other options is not replayed
static std::unordered_map<std::string, int64_t> g_opts;
int64_t ldb_option(const char* name, int64_t dflt) {
   std::lock_guard<std::mutex> lock(g_opt_mu);
   auto it = g_opts.find(name);
   if (it != g_opts.end()) return it->second;
   std::string env = "LDB_";
   for (const char* c = name; *c; c++) env += (char) toupper((unsigned char) *c);
   int64_t v = dflt;
   if (const char* e = getenv(env.c_str())) v = atoll(e);
   g_opts[name] = v;
   return v;
}
extern "C" int32_t ldb_gpu_set_option(const char* name, int64_t value) {
   if (!name) LDB_FAIL(LDB_ERR_INVALID, "set_option: NULL name");
   static const char* known[] = {"jit", "jit_min_rows", "lazy_filter", "lazy_min_rows", "join_ordered", "join_chained", "gb_ordered", "gb_sorted", "zone_maps", "zone_min_rows", "gb_direct", "gb_wgs_per_cu", "gb_partition", "gb_partition_min_rows", "join_radix", "join_radix_min_rows", "join_radix_min_table_bytes", "join_radix_part_bytes", "probe_batch", "debug_check", "join_direct", "join_rank", "join_coarse", "dict_encode", "dict_min_rows", "comm_transport", "comm_timeout_ms", "desc_cache", "desc_cache_mb", "plan_replay", "scan_single_pass", "lazy_strings", "lazy_strings_min_rows", "gb_partition_wc", "join_radix_wc", "join_radix_lds", "gb_dense_out", "gb_partition_values", "join_pair32", "gb_dense_keys", "jit_async", "jit_threads", "jit_disk_cache", "join_all_match", "topk_short_select", "gb_fits64", "join_coarse_fine", "join_coarse_filtered", "compact_wide_tiles", "compact_max_words", "join_fuse_max_conjuncts", "join_coarse_finest", "jit_min_rows_like", "scan_split", "jit_share_compiles", "scan_strset_min_in", "scan_expand_tiles", "scan_expand_zones", "expand_direct_pct"};
   bool ok = false;
   for (const char* k : known) ok |= strcmp(k, name) == 0;
   if (!ok) LDB_FAIL(LDB_ERR_INVALID, "set_option: unknown option '%s'", name);
   std::lock_guard<std::mutex> lock(g_opt_mu);
   g_opts[name] = value;
   g_option_epoch.fetch_add(1);
   return LDB_OK;
}
// the value in effect if the option was set or read before, else what LDB_<NAME> says, else -1 ("the
// use site's default"); never caches anything itself
extern "C" int64_t ldb_gpu_get_option(const char* name) {
   if (!name) return -1;
   std::lock_guard<std::mutex> lock(g_opt_mu);
   auto it = g_opts.find(name);
   if (it != g_opts.end()) return it->second;
   std::string env = "LDB_";
   for (const char* c = name; *c; c++) env += (char) toupper((unsigned char) *c);
   if (const char* e = getenv(env.c_str())) return atoll(e);
   return -1;
}
/* (ldb_gpu_set_option(name, v) with the use site's default restores the default behaviour) */

double ldb_host_trace_threshold() {
   static const double thr = [] {
      const char* e = getenv("LDB_HOST_TRACE");
      return e && *e ? atof(e) : -1.0;
   }();
   return thr;
}
extern "C" int64_t ldb_gpu_option_epoch(void) { return g_option_epoch.load(); }

// ---------------------------------------------------------------- context
extern "C" int32_t ldb_gpu_ctx_create(int32_t device_id, void* stream, ldb_ctx** out) {
   if (!out) LDB_FAIL(LDB_ERR_INVALID, "ctx_create: out is NULL");
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess || n == 0) LDB_FAIL(LDB_ERR_NO_DEVICE, "no HIP device visible (liblingodb_gpu has no CPU fallback)");
   if (device_id < 0 || device_id >= n) LDB_FAIL(LDB_ERR_INVALID, "device %d out of range (have %d)", device_id, n);
   LDB_HIP(hipSetDevice(device_id));
   auto ctx = std::make_unique<ldb_ctx>();
   ctx->device = device_id;
   if (stream) {
      ctx->stream = (hipStream_t) stream;
   } else {
      LDB_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
      ctx->own_stream = true;
   }
   hipDeviceProp_t prop;
   LDB_HIP(hipGetDeviceProperties(&prop, device_id));
   ctx->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
   LDB_HIP(hipHostMalloc((void**) &ctx->h_scratch, 64 * sizeof(int64_t), hipHostMallocDefault));
   LDB_TRY(ldb_mem_init(ctx.get()));
   LDB_HIP(hipMalloc((void**) &ctx->d_scratch, 64 * sizeof(int64_t)));
   *out = ctx.release();
   return LDB_OK;
}
static void ldb_prof_teardown(ldb_ctx* ctx);
// every subsystem frees what it allocated (the trace's log, the arena and the chain's words come into being on first use, in their own files)
extern "C" int32_t ldb_gpu_ctx_destroy(ldb_ctx* ctx) {
   if (!ctx) return LDB_OK;
   (void) hipSetDevice(ctx->device);
   ldb_mem_release_blocks(ctx);
   (void) hipStreamSynchronize(ctx->stream);
   for (auto e : ctx->timers) (void) hipEventDestroy(e);
   ldb_prof_teardown(ctx);
   if (ctx->h_scratch) (void) hipHostFree(ctx->h_scratch);
   ldb_mem_teardown(ctx);
   ldb_trace_teardown(ctx);
   if (ctx->d_scratch) (void) hipFree(ctx->d_scratch);
   ldb_chain_teardown(ctx);
   if (ctx->own_stream) (void) hipStreamDestroy(ctx->stream);
   delete ctx;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_ctx_sync(ldb_ctx* ctx) {
   LDB_HIP(hipStreamSynchronize(ctx->stream));
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_device_info(ldb_ctx* ctx, char* name, int32_t name_cap, int32_t* cus, int64_t* hbm_free, int64_t* hbm_total) {
   hipDeviceProp_t prop;
   LDB_HIP(hipGetDeviceProperties(&prop, ctx->device));
   if (name && name_cap > 0) snprintf(name, (size_t) name_cap, "%s (%s)", prop.name, prop.gcnArchName);
   if (cus) *cus = prop.multiProcessorCount;
   size_t f = 0, t = 0;
   LDB_HIP(hipMemGetInfo(&f, &t));
   if (hbm_free) *hbm_free = (int64_t) f;
   if (hbm_total) *hbm_total = (int64_t) t;
   return LDB_OK;
}

__global__ void k_ldb_marker() {}
extern "C" int32_t ldb_gpu_prof_marker(ldb_ctx* ctx, int32_t id) {
   if (!ctx || id < 1 || id > 65535) LDB_FAIL(LDB_ERR_INVALID, "prof_marker: id must be in 1..65535");
   hipLaunchKernelGGL(k_ldb_marker, dim3((unsigned) id), dim3(64), 0, ctx->stream);
   LDB_HIP(hipGetLastError());
   return LDB_OK;
}

extern "C" int32_t ldb_gpu_timer_create(ldb_ctx* ctx, int32_t* timer_id) {
   hipEvent_t a, b;
   LDB_HIP(hipEventCreate(&a));
   LDB_HIP(hipEventCreate(&b));
   *timer_id = (int32_t) (ctx->timers.size() / 2);
   ctx->timers.push_back(a);
   ctx->timers.push_back(b);
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_timer_start(ldb_ctx* ctx, int32_t id) {
   if (id < 0 || (size_t) id * 2 + 1 >= ctx->timers.size() + 0) LDB_FAIL(LDB_ERR_INVALID, "bad timer id %d", id);
   LDB_HIP(hipEventRecord(ctx->timers[(size_t) id * 2], ctx->stream));
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_timer_stop(ldb_ctx* ctx, int32_t id) {
   if (id < 0 || (size_t) id * 2 + 1 >= ctx->timers.size() + 0) LDB_FAIL(LDB_ERR_INVALID, "bad timer id %d", id);
   LDB_HIP(hipEventRecord(ctx->timers[(size_t) id * 2 + 1], ctx->stream));
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_timer_elapsed_ms(ldb_ctx* ctx, int32_t id, float* ms) {
   if (id < 0 || (size_t) id * 2 + 1 >= ctx->timers.size() + 0) LDB_FAIL(LDB_ERR_INVALID, "bad timer id %d", id);
   LDB_HIP(hipEventSynchronize(ctx->timers[(size_t) id * 2 + 1]));
   LDB_HIP(hipEventElapsedTime(ms, ctx->timers[(size_t) id * 2], ctx->timers[(size_t) id * 2 + 1]));
   return LDB_OK;
}

// ---------------------------------------------------------------- per-kernel profiling
static hipEvent_t prof_event(ldb_ctx* ctx) {
   if (!ctx->prof.free_events.empty()) {
      hipEvent_t e = ctx->prof.free_events.back();
      ctx->prof.free_events.pop_back();
      return e;
   }
   hipEvent_t e = nullptr;
   (void) hipEventCreate(&e);
   return e;
}
static void ldb_prof_teardown(ldb_ctx* ctx) {
   for (auto& p : ctx->prof.pending) {
      (void) hipEventDestroy(p.start);
      (void) hipEventDestroy(p.stop);
   }
   for (auto e : ctx->prof.free_events) (void) hipEventDestroy(e);
}
LdbProf::LdbProf(ldb_ctx* c, const char* name) : ctx(c) {
   if (!c->prof.on) return;
   ldb_prof_pending p{name, prof_event(c), prof_event(c)};
   if (!p.start || !p.stop) return;
   (void) hipEventRecord(p.start, c->stream);
   idx = c->prof.pending.size();
   c->prof.pending.push_back(p);
   active = true;
}
LdbProf::~LdbProf() {
   if (active) (void) hipEventRecord(ctx->prof.pending[idx].stop, ctx->stream);
}
static void prof_fold(ldb_ctx* ctx) {
   if (ctx->prof.pending.empty()) return;
   (void) hipStreamSynchronize(ctx->stream);
   for (auto& p : ctx->prof.pending) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
         ldb_prof_total* t = nullptr;
         for (auto& x : ctx->prof.totals)
            if (x.name == p.name) t = &x;
         if (!t) {
            ctx->prof.totals.push_back({p.name, 0, 0, 0});
            t = &ctx->prof.totals.back();
         }
         t->launches++;
         t->ms += ms;
         if (ms > t->max_ms) t->max_ms = ms;
      }
      ctx->prof.free_events.push_back(p.start);
      ctx->prof.free_events.push_back(p.stop);
   }
   ctx->prof.pending.clear();
}
extern "C" int32_t ldb_gpu_prof_enable(ldb_ctx* ctx, int32_t on) {
   if (!ctx) LDB_FAIL(LDB_ERR_INVALID, "prof_enable: NULL ctx");
   prof_fold(ctx);
   ctx->prof.on = on != 0;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_prof_reset(ldb_ctx* ctx) {
   if (!ctx) LDB_FAIL(LDB_ERR_INVALID, "prof_reset: NULL ctx");
   prof_fold(ctx);
   ctx->prof.totals.clear();
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_prof_get(ldb_ctx* ctx, const char* kernel_name, int64_t* launches, double* total_ms) {
   if (!ctx || !kernel_name) LDB_FAIL(LDB_ERR_INVALID, "prof_get: NULL argument");
   prof_fold(ctx);
   if (launches) *launches = 0;
   if (total_ms) *total_ms = 0;
   for (auto& x : ctx->prof.totals)
      if (x.name == kernel_name) {
         if (launches) *launches = x.launches;
         if (total_ms) *total_ms = x.ms;
      }
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_prof_get_max(ldb_ctx* ctx, const char* kernel_name, double* max_ms) {
   if (!ctx || !kernel_name || !max_ms) LDB_FAIL(LDB_ERR_INVALID, "prof_get_max: NULL argument");
   prof_fold(ctx);
   *max_ms = 0;
   for (auto& x : ctx->prof.totals)
      if (x.name == kernel_name) *max_ms = x.max_ms;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_prof_names(ldb_ctx* ctx, char* buf, int32_t cap) {
   if (!ctx || !buf || cap < 1) LDB_FAIL(LDB_ERR_INVALID, "prof_names: bad argument");
   prof_fold(ctx);
   std::string s;
   for (auto& x : ctx->prof.totals) s += x.name + "\n";
   snprintf(buf, (size_t) cap, "%s", s.c_str());
   return LDB_OK;
}
