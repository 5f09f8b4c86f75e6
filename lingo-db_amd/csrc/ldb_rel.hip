// ldb_rel.hip — relations (row-id vectors over tables), the device descriptors built from them (DCol, DPred, DKeys), LIKE
// planning, conjunct ordering, row-id composition, gather / materialise.
#include "ldb_internal.h"
#include "ldb_device.h"
#include <algorithm>

// ---------------------------------------------------------------- relations
ldb_rel* ldb_rel_new(ldb_ctx* ctx) {
   auto* r = new ldb_rel();
   r->ctx = ctx;
   return r;
}
extern "C" int32_t ldb_gpu_rel_from_table(ldb_ctx* ctx, const ldb_table* t, ldb_rel** out) {
   if (!ctx || !t || !out) LDB_FAIL(LDB_ERR_INVALID, "rel_from_table: NULL argument");
   ldb_rel* r = ldb_rel_new(ctx);
   r->n_rows = t->n_rows;
   r->sides.push_back({t, nullptr, false});
   *out = r;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_rel_release(ldb_ctx* ctx, ldb_rel* r) {
   if (!r) return LDB_OK;
   for (auto& s : r->sides)
      if (s.owned) ldb_dev_free(ctx, s.rowids);
   delete r;
   return LDB_OK;
}
extern "C" int64_t ldb_gpu_rel_rows(ldb_ctx* ctx, ldb_rel* r) {
   if (!r) return -1;
   if (!r->pending.empty() && ldb_rel_force(ctx ? ctx : r->ctx, r) != LDB_OK) return -1; // a lazy filter is evaluated now
   return r->n_rows;
}
extern "C" int32_t ldb_gpu_rel_sides(const ldb_rel* r) { return r ? (int32_t) r->sides.size() : -1; }

__global__ void k_iota_u32(uint32_t* out, uint64_t n) {
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) out[i] = (uint32_t) i;
}
extern "C" int32_t ldb_gpu_rel_read_rowids(ldb_ctx* ctx, ldb_rel* r, int32_t side, uint32_t* host_out, int64_t cap) {
   if (!r || side < 0 || (size_t) side >= r->sides.size()) LDB_FAIL(LDB_ERR_INVALID, "read_rowids: bad side %d", side);
   LDB_TRY(ldb_rel_force(ctx, r));
   if (cap < r->n_rows) LDB_FAIL(LDB_ERR_INVALID, "read_rowids: buffer too small");
   if (r->sides[(size_t) side].rowids) {
      if (r->n_rows) LDB_HIP(hipMemcpyAsync(host_out, r->sides[(size_t) side].rowids, (size_t) r->n_rows * 4, hipMemcpyDeviceToHost, ctx->stream));
      LDB_HIP(hipStreamSynchronize(ctx->stream));
   } else {
      for (int64_t i = 0; i < r->n_rows; i++) host_out[i] = (uint32_t) i;
   }
   return LDB_OK;
}

int32_t ldb_make_dcol(const ldb_rel* r, ldb_colref ref, DCol* out) {
   if (ref.side < 0 || (size_t) ref.side >= r->sides.size()) LDB_FAIL(LDB_ERR_INVALID, "column ref: side %d out of range", ref.side);
   const ldb_rel_side& s = r->sides[(size_t) ref.side];
   if (ref.col < 0 || (size_t) ref.col >= s.table->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "column ref: col %d out of range on side %d", ref.col, ref.side);
   const ldb_column& c = s.table->cols[(size_t) ref.col];
   if (ldb_column_is_lazy(c)) LDB_TRY(ldb_column_strings(r->ctx, c, s.table->n_rows)); // a byte-wise consumer: the strings are needed now
   out->values = (uint64_t) c.values;
   out->offsets = (uint64_t) c.offsets;
   out->validity = (uint64_t) c.validity;
   out->rowids = (uint64_t) s.rowids;
   out->type = c.type.type;
   out->width = c.width;
   out->precision = c.type.precision;
   out->scale = c.type.scale;
   return LDB_OK;
}

int32_t ldb_make_dpred(const ldb_rel* r, const ldb_filter_desc* p, DPred* out) {
   memset(out, 0, sizeof(*out));
   LDB_TRY(ldb_make_dcol(r, p->col, &out->col));
   out->op = p->op;
   out->rhs_kind = p->rhs_kind;
   out->lo = p->value_lo;
   out->hi = p->value_hi;
   out->f = p->value_f64;
   if (p->op < LDB_F_EQ || p->op > LDB_F_NOT_LIKE) LDB_FAIL(LDB_ERR_INVALID, "filter: bad op %d", p->op);
   if ((p->op == LDB_F_LIKE || p->op == LDB_F_NOT_LIKE) && (out->col.type != LDB_T_UTF8 || p->rhs_kind != LDB_RHS_STRING))
      LDB_FAIL(LDB_ERR_INVALID, "filter: LIKE needs a utf8 column and a string pattern");
   if (p->op == LDB_F_NOTNULL) return LDB_OK;
   bool is_str = out->col.type == LDB_T_UTF8;
   if (p->rhs_kind == LDB_RHS_COLUMN) {
      if (p->op == LDB_F_IN) LDB_FAIL(LDB_ERR_INVALID, "filter: IN needs constants");
      LDB_TRY(ldb_make_dcol(r, p->rhs_col, &out->rhs));
      if ((out->rhs.type == LDB_T_UTF8) != is_str) LDB_FAIL(LDB_ERR_INVALID, "filter: string compared with non-string column");
      return LDB_OK;
   }
   if (is_str != (p->rhs_kind == LDB_RHS_STRING)) LDB_FAIL(LDB_ERR_INVALID, "filter: constant kind %d does not match column type %d", p->rhs_kind, out->col.type);
   if (is_str) { // a dictionary-encoded column: the predicate becomes a test on the 4-byte codes
      bool done = false;
      LDB_TRY(ldb_dict_rewrite_pred(r, p, out, &done));
      if (done) return LDB_OK;
   }
   if (p->op == LDB_F_IN) {
      if (p->n_in < 0 || p->n_in > LDB_MAX_IN) LDB_FAIL(LDB_ERR_UNSUPPORTED, "filter: IN list of %d values (max %d inline; a longer list over a utf8 column is evaluated by ldb_gpu_scan_filter alone)", p->n_in, LDB_MAX_IN);
      out->n_in = p->n_in;
      if (is_str) {
         int32_t pos = 0;
         for (int k = 0; k < p->n_in; k++) {
            if (pos + p->in_str_lens[k] > (int32_t) sizeof(out->in_blob)) LDB_FAIL(LDB_ERR_UNSUPPORTED, "filter: IN string constants exceed %zu bytes inline (ldb_gpu_scan_filter alone evaluates longer ones)", sizeof(out->in_blob));
            out->in_off[k] = pos;
            memcpy(out->in_blob + pos, p->in_strs[k], (size_t) p->in_str_lens[k]);
            pos += p->in_str_lens[k];
         }
         out->in_off[p->n_in] = pos;
      } else {
         for (int k = 0; k < p->n_in; k++) {
            out->in_lo[k] = (uint64_t) p->in_values[2 * k];
            out->in_hi[k] = p->in_values[2 * k + 1];
         }
      }
      return LDB_OK;
   }
   // zone map: column-vs-constant comparison over a dense, NOT NULL integer-like column of a large base table
   if (!is_str && p->rhs_kind == LDB_RHS_INT && p->op >= LDB_F_EQ && p->op <= LDB_F_GTE && !out->col.rowids && !out->col.validity && out->hi == ((int64_t) out->lo >> 63) && r->ctx &&
       ldb_option("zone_maps", 1) != 0) {
      const ldb_table* zt = r->sides[(size_t) p->col.side].table;
      if (zt->n_rows >= ldb_option("zone_min_rows", 1 << 20)) LDB_TRY(ldb_column_zones(r->ctx, zt, p->col.col, &out->zmin, &out->zmax));
   }
   if (is_str) {
      if (p->str_len < 0 || p->str_len > LDB_STR_INLINE) LDB_FAIL(LDB_ERR_UNSUPPORTED, "filter: string constant of %d bytes (max %d inline; ldb_gpu_scan_filter alone compares longer ones, LIKE patterns excepted)", p->str_len, LDB_STR_INLINE);
      out->str_len = p->str_len;
      memcpy(out->str, p->str, (size_t) p->str_len);
      if (p->op == LDB_F_LIKE || p->op == LDB_F_NOT_LIKE) ldb_like_plan(out);
   }
   return LDB_OK;
}

// "Simple" LIKE patterns — ASCII literals separated by '%', no '_' and no escape: %A%B%, A%, %A,
// A%B … — are matched by position instead of by row (ldb_device.h d_like_simple_wave).  For such a
// pattern byte-wise substring search IS the reference's character-wise iterativeLike
// (StringRuntime.cpp:28-93): an ASCII pattern byte never equals a UTF-8 lead or continuation byte.
// Plan: n_in = number of literal segments (0 = not simple), in_off[2j] / in_off[2j+1] = start and
// length of segment j inside str, lo bit 0 / bit 1 = the pattern is anchored at the start / end.
void ldb_like_plan(DPred* d);
// the planner's verdict on a pattern, for host-side tests and for an emitter that wants to know which
// matcher a LIKE will get: *n_segments = 0 → general matcher; else seg[2j] / seg[2j+1] = start / length of
// literal j inside the pattern and *anchors bit 0 / bit 1 = anchored at the start / end.  No device needed.
extern "C" int32_t ldb_gpu_like_plan(const char* pattern, int32_t len, int32_t* n_segments, int32_t* seg, int32_t* anchors) {
   if (!pattern || !n_segments || len < 0 || len > LDB_STR_INLINE) LDB_FAIL(LDB_ERR_INVALID, "like_plan: bad argument (patterns are at most %d bytes)", LDB_STR_INLINE);
   DPred d;
   memset(&d, 0, sizeof(d));
   d.str_len = len;
   memcpy(d.str, pattern, (size_t) len);
   ldb_like_plan(&d);
   *n_segments = d.n_in;
   if (seg)
      for (int j = 0; j < 2 * d.n_in; j++) seg[j] = d.in_off[j];
   if (anchors) *anchors = d.n_in ? (int32_t) (d.lo & 3) : 0;
   return LDB_OK;
}
void ldb_like_plan(DPred* d) {
   d->n_in = 0;
   const int n = d->str_len;
   int nseg = 0, seg_start = -1, off[2 * LDB_LIKE_MAX_SEG];
   for (int k = 0; k <= n; k++) {
      const unsigned char c = k < n ? (unsigned char) d->str[k] : (unsigned char) '%';
      if (k < n && (c >= 0x80 || c == '_' || c == '\\')) return;
      if (c == '%') {
         if (seg_start >= 0) {
            if (nseg == LDB_LIKE_MAX_SEG || k - seg_start > 16) return;
            off[2 * nseg] = seg_start;
            off[2 * nseg + 1] = k - seg_start;
            nseg++;
            seg_start = -1;
         }
      } else if (seg_start < 0) {
         seg_start = k;
      }
   }
   if (nseg == 0) return; // "", "%", "%%": the general matcher decides at once
   for (int j = 0; j < 2 * nseg; j++) d->in_off[j] = off[j];
   d->n_in = nseg;
   d->lo = (d->str[0] != '%' ? 1u : 0u) | (d->str[n - 1] != '%' ? 2u : 0u);
}

// marks conjuncts whose lhs column is the previous conjunct's (range filters): the batched
// evaluator loads the column once for both (ldb_device.h d_eval_conj_batch)
// A conjunction may be evaluated in any order (no side effects; NULL operands just fail).  Cheap
// conjuncts go first so that the expensive ones (string compares: offsets + bytes per row) only
// run for the surviving lanes: Q12's lineitem filter lists l_shipmode IN ('MAIL','SHIP') first and
// spent 6.3 ms reading 600 M strings before the date conjuncts had rejected 97 % of the rows.
static int pred_cost(const DPred& p) {
   const bool str = p.col.type == LDB_T_UTF8;
   const bool wide = (p.col.type == LDB_T_DECIMAL128 && p.col.precision >= 19) || p.col.type == LDB_T_FLOAT64 || p.col.type == LDB_T_FLOAT32;
   if (p.op == LDB_F_NOTNULL) return 0;
   if (str) return p.op == LDB_F_LIKE || p.op == LDB_F_NOT_LIKE ? 7 : (p.op == LDB_F_IN || p.rhs_kind == LDB_RHS_COLUMN ? 6 : 5);
   if (wide) return 3;
   if (p.rhs_kind == LDB_RHS_COLUMN || p.op == LDB_F_IN) return 2;
   return 1;
}
void ldb_order_preds(DPred* preds, int32_t n) {
   std::stable_sort(preds, preds + n, [](const DPred& a, const DPred& b) { return pred_cost(a) < pred_cost(b); });
   ldb_mark_same_col(preds, n);
}

void ldb_mark_same_col(DPred* preds, int32_t n) {
   for (int32_t p = 1; p < n; p++) {
      const DCol &a = preds[p - 1].col, &b = preds[p].col;
      preds[p].same_col = a.values == b.values && a.offsets == b.offsets && a.validity == b.validity && a.rowids == b.rowids && a.type == b.type && a.width == b.width &&
                                a.precision == b.precision
                             ? 1
                             : 0;
   }
}

// ---------------------------------------------------------------- row-id composition
struct DComposeMulti {
   uint64_t n;
   const uint32_t* sel[2];
   const uint32_t* ids[12];
   uint32_t* out[12];
   int32_t n_out;
   uint8_t which[12];
};
__global__ void k_compose_multi(DComposeMulti d) {
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < d.n; i += (uint64_t) gridDim.x * blockDim.x) {
      const uint32_t s0 = d.sel[0][i];
      const uint32_t s1 = d.sel[1] ? d.sel[1][i] : 0u;
#pragma unroll
      for (int j = 0; j < 12; j++) {
         if (j >= d.n_out) break;
         const uint32_t s = d.which[j] ? s1 : s0;
         d.out[j][i] = s == LDB_NULL_ROW ? LDB_NULL_ROW : (d.ids[j] ? d.ids[j][s] : s);
      }
   }
}
int32_t ldb_compose_rowids(ldb_ctx* ctx, const uint32_t* sel0, const uint32_t* sel1, const LdbComposeJob* jobs, int n_jobs, uint64_t n) {
   if (!n || !n_jobs) return LDB_OK;
   LdbProf prof_(ctx, "k_compose_rowids");
   for (int at = 0; at < n_jobs; at += 12) {
      DComposeMulti d;
      memset(&d, 0, sizeof(d));
      d.n = n;
      d.sel[0] = sel0;
      d.sel[1] = sel1;
      d.n_out = std::min(12, n_jobs - at);
      for (int j = 0; j < d.n_out; j++) {
         d.ids[j] = jobs[at + j].ids;
         d.out[j] = jobs[at + j].out;
         d.which[j] = (uint8_t) jobs[at + j].which;
      }
      hipLaunchKernelGGL(k_compose_multi, dim3(ldb_grid_for(ctx, (int64_t) n, 256, 8)), dim3(256), 0, ctx->stream, d);
   }
   LDB_HIP(hipGetLastError());
   return LDB_OK;
}

// ---------------------------------------------------------------- gather / materialize
template <typename T>
__global__ void k_gather_fixed(const T* __restrict__ src, const uint32_t* __restrict__ rowids, T* __restrict__ dst, uint64_t n) {
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
      uint32_t r = rowids ? rowids[i] : (uint32_t) i;
      T v{};
      if (r != LDB_NULL_ROW) v = src[r];
      dst[i] = v;
   }
}
// validity bitmap of a gathered column + its NULL count in one pass: one row per lane, the wave's
// ballot is the 64-bit bitmap word (the bitmap buffer is 8-byte granular: ldb_dev_alloc pads)
__global__ void k_gather_validity(const uint8_t* __restrict__ validity, const uint32_t* __restrict__ rowids, uint64_t* __restrict__ bitmap_words, uint64_t n,
                                  unsigned long long* __restrict__ null_count) {
   const uint64_t n_pad = (n + 63) & ~(uint64_t) 63;
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n_pad; i += (uint64_t) gridDim.x * blockDim.x) {
      bool ok = false;
      if (i < n) {
         const uint32_t r = rowids ? rowids[i] : (uint32_t) i;
         ok = r != LDB_NULL_ROW && (!validity || ((validity[r >> 3] >> (r & 7)) & 1));
      }
      const uint64_t m = __ballot(ok);
      if ((threadIdx.x & 63) == 0) {
         bitmap_words[i >> 6] = m;
         const uint64_t rows_here = n - i >= 64 ? ~(uint64_t) 0 : (((uint64_t) 1 << (n - i)) - 1);
         const int nulls = __popcll(~m & rows_here);
         if (nulls) atomicAdd(null_count, (unsigned long long) nulls);
      }
   }
}
__global__ void k_str_lens(const int64_t* __restrict__ offsets, const uint32_t* __restrict__ rowids, int64_t* __restrict__ lens, uint64_t n) {
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
      uint32_t r = rowids ? rowids[i] : (uint32_t) i;
      lens[i] = r == LDB_NULL_ROW ? 0 : offsets[r + 1] - offsets[r];
   }
}
__global__ void k_str_copy(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off, const uint32_t* __restrict__ rowids,
                           int64_t* __restrict__ dst_off, uint8_t* __restrict__ dst, uint64_t n, int64_t total) {
   if (blockIdx.x == 0 && threadIdx.x == 0) dst_off[n] = total; // the closing offset of the Arrow layout
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
      uint32_t r = rowids ? rowids[i] : (uint32_t) i;
      if (r == LDB_NULL_ROW) continue;
      int64_t b = src_off[r], len = src_off[r + 1] - b, d = dst_off[i];
      if (d + len > total) len = total > d ? total - d : 0; // (total = the host's byte count; see ldb_readback)
      for (int64_t k = 0; k < len; k++) dst[d + k] = src[b + k];
   }
}

struct u128x {
   uint64_t a, b;
};

// Gather columns of `r` into new owned columns.  All launches of all columns are queued first; the
// NULL counts of the nullable ones and the byte totals of the string ones come back in ONE read
// (one stream synchronisation per call, none when no column is nullable or a string).  A column
// can be NULL in the result only if the source column has a validity bitmap or its side carries
// outer-join padding (ldb_rel_side::may_null).
int32_t ldb_gather_columns(ldb_ctx* ctx, const ldb_rel* r, const ldb_colref* refs, int32_t n_cols, ldb_column* outs) {
   const uint64_t n = (uint64_t) r->n_rows;
   const int grid = ldb_grid_for(ctx, (int64_t) n, 256, 8);
   struct Pending {
      int32_t col;
      int slot_nulls = -1, slot_bytes = -1;
      const uint32_t* rowids = nullptr;
      int64_t* lens = nullptr;
   };
   std::vector<Pending> pend((size_t) n_cols);
   LdbBufs tmp(ctx); // the string lengths; the outputs belong to the caller's columns
   int n_slots = 0;
   const bool lazy_on = ldb_option("lazy_strings", 1) != 0;
   const uint64_t lazy_min = (uint64_t) ldb_option("lazy_strings_min_rows", 4096);
   std::vector<ldb_column*> lazy_small; // lazy outputs too short to be worth keeping lazy: written out before returning
   for (int32_t c = 0; c < n_cols; c++) {
      const ldb_rel_side& side = r->sides[(size_t) refs[c].side];
      const ldb_column& src = side.table->cols[(size_t) refs[c].col];
      pend[(size_t) c].col = c;
      if (src.validity || (side.rowids && side.may_null)) pend[(size_t) c].slot_nulls = n_slots++;
      const bool will_be_lazy = src.type.type == LDB_T_UTF8 && src.dict_codes && src.dict && (ldb_column_is_lazy(src) || (n >= 64 && n >= lazy_min && lazy_on));
      if (src.type.type == LDB_T_UTF8 && !will_be_lazy) pend[(size_t) c].slot_bytes = n_slots++;
   }
   unsigned long long* d_words = nullptr;
   if (n_slots) LDB_TRY(ldb_counters(ctx, n_slots, (uint64_t**) &d_words)); // zeroed arena words
   LdbProf prof_(ctx, "k_gather"); // (all gather launches of the call; the string copies after the read-back are not inside)
   for (int32_t c = 0; c < n_cols; c++) {
      Pending& p = pend[(size_t) c];
      // (only the side's row ids are needed here; ldb_make_dcol would write a lazy source column's strings out — the very
      // thing a code-only gather avoids — and change its laziness between the slot assignment above and the branch below)
      p.rowids = r->sides[(size_t) refs[c].side].rowids;
      const ldb_column& src = r->sides[(size_t) refs[c].side].table->cols[(size_t) refs[c].col];
      ldb_column* out = &outs[c];
      out->name = src.name;
      out->type = src.type;
      out->width = src.width;
      out->owned = true;
      if (p.slot_nulls >= 0) {
         LDB_TRY(LdbBufs::alloc_into(ctx, &out->validity, (size_t) ((n + 7) / 8 + 8)));
         if (n) hipLaunchKernelGGL(k_gather_validity, dim3(grid), dim3(256), 0, ctx->stream, src.validity, p.rowids, (uint64_t*) out->validity, n, d_words + p.slot_nulls);
      }
      const bool src_lazy = ldb_column_is_lazy(src);
      if (src.type.type == LDB_T_UTF8 && src.dict_codes && src.dict && (n >= 64 || src_lazy)) {
         // the gathered column inherits the source's dictionary: codes gathered alongside, the dictionary table shared
         LDB_TRY(LdbBufs::alloc_into(ctx, &out->dict_codes, 4 * (size_t) (n ? n : 1)));
         if (n) hipLaunchKernelGGL(k_gather_fixed<uint32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const uint32_t*) src.dict_codes, p.rowids, out->dict_codes, n);
         out->dict = src.dict;
         out->dict->dict_refs++;
         out->dict_size = src.dict_size;
         out->dict_pred_cache = new std::unordered_map<std::string, std::string>();
      }
      if (src.type.type == LDB_T_UTF8 && out->dict_codes && (src_lazy || (n >= lazy_min && lazy_on))) {
         // LAZY: codes + dictionary only; whoever needs the bytes writes them out of the dictionary (ldb_column_strings)
         out->value_bytes = -1;
         p.slot_bytes = -1;
         lazy_small.push_back(src_lazy && n < 64 ? out : nullptr);
      } else if (src.type.type == LDB_T_UTF8) {
         LDB_TRY(tmp.alloc(&p.lens, sizeof(int64_t) * (size_t) (n + 1)));
         LDB_TRY(LdbBufs::alloc_into(ctx, &out->offsets, sizeof(int64_t) * (size_t) (n + 1)));
         hipLaunchKernelGGL(k_str_lens, dim3(grid), dim3(256), 0, ctx->stream, src.offsets, p.rowids, p.lens, n);
         LDB_TRY(ldb_exclusive_scan_i64(ctx, p.lens, out->offsets, (int64_t) n, (int64_t*) (d_words + p.slot_bytes)));
      } else {
         out->value_bytes = (int64_t) n * src.width;
         // the gathered values are a subset of the source's: its cached [min, max] stays a valid (superset) statistic of the new column —
         // an intermediate's key range is then known without a pass over it in every execution (Q18: 150 M group keys, k_column_range
         // 0.35 ms inside the timed run; Q14, Q7).  Not where padding rows (outer joins) or NULL slots carry other bytes.
         if (src.has_range && p.slot_nulls < 0) {
            out->has_range = true;
            out->vmin = src.vmin;
            out->vmax = src.vmax;
         }
         LDB_TRY(LdbBufs::alloc_into(ctx, &out->values, (size_t) out->value_bytes));
         switch (src.width) {
            case 1: hipLaunchKernelGGL(k_gather_fixed<uint8_t>, dim3(grid), dim3(256), 0, ctx->stream, (const uint8_t*) src.values, p.rowids, (uint8_t*) out->values, n); break;
            case 2: hipLaunchKernelGGL(k_gather_fixed<uint16_t>, dim3(grid), dim3(256), 0, ctx->stream, (const uint16_t*) src.values, p.rowids, (uint16_t*) out->values, n); break;
            case 4: hipLaunchKernelGGL(k_gather_fixed<uint32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const uint32_t*) src.values, p.rowids, (uint32_t*) out->values, n); break;
            case 8: hipLaunchKernelGGL(k_gather_fixed<uint64_t>, dim3(grid), dim3(256), 0, ctx->stream, (const uint64_t*) src.values, p.rowids, (uint64_t*) out->values, n); break;
            default: hipLaunchKernelGGL(k_gather_fixed<u128x>, dim3(grid), dim3(256), 0, ctx->stream, (const u128x*) src.values, p.rowids, (u128x*) out->values, n); break;
         }
      }
   }
   LDB_HIP(hipGetLastError());
   auto finish_lazy = [&]() -> int32_t {
      for (ldb_column* lc : lazy_small)
         if (lc) LDB_TRY(ldb_column_strings(ctx, *lc, (int64_t) n));
      return LDB_OK;
   };
   if (!n_slots) return finish_lazy();
   std::vector<unsigned long long> words((size_t) n_slots);
   LDB_TRY(LDB_READBACK(ctx, words.data(), d_words, 8 * (size_t) n_slots));
   for (int32_t c = 0; c < n_cols; c++) {
      Pending& p = pend[(size_t) c];
      ldb_column* out = &outs[c];
      if (p.slot_nulls >= 0) {
         out->null_count = (int64_t) words[(size_t) p.slot_nulls];
         if (out->null_count == 0) {
            LdbBufs::drop(ctx, &out->validity);
         }
      }
      if (p.slot_bytes >= 0) {
         const ldb_column& src = r->sides[(size_t) refs[c].side].table->cols[(size_t) refs[c].col];
         const uint64_t total = words[(size_t) p.slot_bytes];
         tmp.free(p.lens);
         out->value_bytes = (int64_t) total;
         LDB_TRY(LdbBufs::alloc_into(ctx, &out->values, (size_t) total));
         hipLaunchKernelGGL(k_str_copy, dim3(grid), dim3(256), 0, ctx->stream, (const uint8_t*) src.values, src.offsets, p.rowids, out->offsets, (uint8_t*) out->values, n,
                            (int64_t) total);
      }
   }
   LDB_HIP(hipGetLastError());
   return finish_lazy();
}

// writes a lazy utf8 column's strings out of its dictionary: string i = dictionary[code i] (a NULL code gives the empty string;
// the column's validity bitmap is separate).  The column object is logically const (the same value, another representation).
int32_t ldb_column_strings(ldb_ctx* ctx, const ldb_column& cc, int64_t n_rows) {
   if (!ldb_column_is_lazy(cc)) return LDB_OK;
   ldb_column& c = const_cast<ldb_column&>(cc);
   const ldb_column& dict = c.dict->cols[0];
   const uint64_t n = (uint64_t) n_rows;
   const int grid = ldb_grid_for(ctx, n_rows, 256, 8);
   int64_t *lens = nullptr, *offsets = nullptr;
   LdbBufs tmp(ctx);
   LDB_TRY(tmp.alloc(&lens, 8 * (size_t) (n + 1)));
   LDB_TRY(tmp.alloc(&offsets, 8 * (size_t) (n + 1)));
   uint64_t* d_total;
   LDB_TRY(ldb_counters(ctx, 1, &d_total));
   if (n) hipLaunchKernelGGL(k_str_lens, dim3(grid), dim3(256), 0, ctx->stream, (const int64_t*) dict.offsets, (const uint32_t*) c.dict_codes, lens, n);
   LDB_TRY(ldb_exclusive_scan_i64(ctx, lens, offsets, n_rows, (int64_t*) d_total));
   uint64_t total = 0;
   LDB_TRY(ldb_read_u64(ctx, d_total, &total));
   void* values = nullptr;
   LDB_TRY(tmp.alloc((uint8_t**) &values, (size_t) total));
   hipLaunchKernelGGL(k_str_copy, dim3(grid > 0 ? grid : 1), dim3(256), 0, ctx->stream, (const uint8_t*) dict.values, (const int64_t*) dict.offsets, (const uint32_t*) c.dict_codes, offsets, (uint8_t*) values, n,
                      (int64_t) total);
   LDB_HIP(hipGetLastError());
   tmp.keep(offsets);
   tmp.keep(values);
   c.offsets = offsets;
   c.values = values;
   c.value_bytes = (int64_t) total;
   return LDB_OK;
}

extern "C" int32_t ldb_gpu_materialize(ldb_ctx* ctx, ldb_rel* r, const ldb_colref* cols, int32_t n_cols, ldb_table** out) {
   if (!ctx || !r || !out || n_cols < 0) LDB_FAIL(LDB_ERR_INVALID, "materialize: bad argument");
   LDB_TRY(ldb_rel_force(ctx, r));
   for (int32_t c = 0; c < n_cols; c++)
      if (cols[c].side < 0 || (size_t) cols[c].side >= r->sides.size() || cols[c].col < 0 || (size_t) cols[c].col >= r->sides[(size_t) cols[c].side].table->cols.size())
         LDB_FAIL(LDB_ERR_INVALID, "materialize: column %d:%d out of range", cols[c].side, cols[c].col);
   LdbTableHold t(ctx, new ldb_table());
   t->ctx = ctx;
   t->name = "materialized";
   t->n_rows = r->n_rows;
   t->cols.resize((size_t) n_cols);
   LDB_TRY(ldb_gather_columns(ctx, r, cols, n_cols, t->cols.data()));
   *out = t.release();
   return LDB_OK;
}
