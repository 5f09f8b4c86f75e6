// ldb_table.hip — device tables: Arrow C Data Interface in (ldb_gpu_table_register) and out (ldb_gpu_export), allocation, hash
// indexes, accessors, fixed-width reads and writes, the content stamp of prepared plans.
// Replaces (reference): LingoDBTable::ensureLoaded + TableChunk flattening (src/runtime/storage/LingoDBTable.cpp:27-54,
// 200-225) and the Arrow side of result materialisation (ArrowColumnBuilder, include/lingodb/runtime/ArrowColumn.h:15-37).
#include "ldb_internal.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>

static std::atomic<uint64_t> g_serial{1};
uint64_t ldb_next_serial() { return g_serial.fetch_add(1); }
extern "C" uint64_t ldb_gpu_table_stamp(const ldb_table* t) { return t ? t->serial : 0; }
// ---------------------------------------------------------------- tables
int32_t ldb_width_of(const ldb_coltype& t, int narrow) {
   switch (t.type) {
      case LDB_T_INT8:
      case LDB_T_BOOL8: return 1;
      case LDB_T_INT16: return 2;
      case LDB_T_INT32:
      case LDB_T_DATE32:
      case LDB_T_CHAR4:
      case LDB_T_FLOAT32: return 4;
      case LDB_T_INT64:
      case LDB_T_FLOAT64: return 8;
      case LDB_T_DECIMAL128: return (narrow && t.precision < 19) ? 8 : 16;
      default: return 0;
   }
}

// narrow == 2 (round 6, "compressed resident format"): a column whose values fit is stored at the narrowest of 1 / 2 / 4 / 8 bytes — decimals of
// precision < 19 (the generated code truncates those to 64 bits anyway, LowerToStd.cpp:128-132) and char(1) (one byte when every value is ASCII).
// Kernels widen in registers (d_load_i64 dispatches on the column's width) and compute in i64 / i128 exactly as before: results are bit-identical.
int32_t ldb_narrowest_width(int64_t lo, int64_t hi) {
   if (lo >= -128 && hi <= 127) return 1;
   if (lo >= -32768 && hi <= 32767) return 2;
   if (lo >= INT32_MIN && hi <= INT32_MAX) return 4;
   return 8;
}
bool ldb_type_narrows(const ldb_coltype& t) { return (t.type == LDB_T_DECIMAL128 && t.precision < 19) || t.type == LDB_T_CHAR4; }

static int parse_format(const char* f, ldb_coltype* t, bool* large) {
   *large = false;
   t->precision = t->scale = 0;
   if (!strcmp(f, "c")) t->type = LDB_T_INT8;
   else if (!strcmp(f, "s")) t->type = LDB_T_INT16;
   else if (!strcmp(f, "i")) t->type = LDB_T_INT32;
   else if (!strcmp(f, "l")) t->type = LDB_T_INT64;
   else if (!strcmp(f, "tdD")) t->type = LDB_T_DATE32;
   else if (!strcmp(f, "g")) t->type = LDB_T_FLOAT64;
   else if (!strcmp(f, "f")) t->type = LDB_T_FLOAT32;
   else if (!strcmp(f, "u")) t->type = LDB_T_UTF8;
   else if (!strcmp(f, "U")) {
      t->type = LDB_T_UTF8;
      *large = true;
   } else if (!strcmp(f, "w:4")) t->type = LDB_T_CHAR4;
   else if (!strncmp(f, "d:", 2)) {
      int p = 0, s = 0, bits = 128;
      int n = sscanf(f + 2, "%d,%d,%d", &p, &s, &bits);
      if (n < 2 || bits != 128) return -1;
      t->type = LDB_T_DECIMAL128;
      t->precision = p;
      t->scale = s;
   } else
      return -1;
   return 0;
}

extern "C" int32_t ldb_gpu_table_register(ldb_ctx* ctx, const char* name, struct ArrowSchema* schema, struct ArrowArray** batches,
                                          int64_t n_batches, int32_t narrow, ldb_table** out) {
   if (!ctx || !schema || !out) LDB_FAIL(LDB_ERR_INVALID, "table_register: NULL argument");
   if (strcmp(schema->format, "+s")) LDB_FAIL(LDB_ERR_INVALID, "table_register: schema must be a struct (+s), got %s", schema->format);
   LdbTableHold t(ctx, new ldb_table());
   t->ctx = ctx;
   t->name = name ? name : "";
   int64_t rows = 0;
   for (int64_t b = 0; b < n_batches; b++) {
      if (batches[b]->n_children != schema->n_children) LDB_FAIL(LDB_ERR_INVALID, "batch %ld has %ld children, schema %ld", (long) b, (long) batches[b]->n_children, (long) schema->n_children);
      // a sliced struct array (parent offset / length) selects rows [offset, offset + length) of every child
      for (int64_t c = 0; c < schema->n_children; c++) {
         const struct ArrowArray* ch = batches[b]->children[c];
         if (batches[b]->offset < 0 || batches[b]->length < 0 || ch->length < batches[b]->offset + batches[b]->length)
            LDB_FAIL(LDB_ERR_INVALID, "batch %ld: child %ld has %ld rows, the struct slice needs %ld", (long) b, (long) c, (long) ch->length, (long) (batches[b]->offset + batches[b]->length));
      }
      rows += batches[b]->length;
   }
   if (rows >= (int64_t) LDB_NULL_ROW) LDB_FAIL(LDB_ERR_UNSUPPORTED, "table_register: %ld rows exceed uint32 row ids", (long) rows);
   t->n_rows = rows;
   t->cols.resize((size_t) schema->n_children);
   for (int64_t c = 0; c < schema->n_children; c++) {
      ldb_column& col = t->cols[(size_t) c];
      struct ArrowSchema* cs = schema->children[c];
      col.name = cs->name ? cs->name : "";
      bool large = false;
      if (parse_format(cs->format, &col.type, &large)) LDB_FAIL(LDB_ERR_UNSUPPORTED, "column %s: Arrow format '%s' not supported", col.name.c_str(), cs->format);
      col.type.nullable = (cs->flags & ARROW_FLAG_NULLABLE) ? 1 : 0;
      col.width = ldb_width_of(col.type, narrow);
      // validity: only materialised when some batch really has nulls
      bool any_null = false;
      for (int64_t b = 0; b < n_batches; b++) {
         struct ArrowArray* a = batches[b]->children[c];
            const int64_t alen = batches[b]->length, aoff = batches[b]->offset + a->offset; // the parent's slice applies to every child
         if (a->null_count != 0 && a->buffers[0]) {
            const uint8_t* v = (const uint8_t*) a->buffers[0];
            for (int64_t i = 0; i < alen && !any_null; i++) {
               int64_t k = i + aoff;
               if (!((v[k >> 3] >> (k & 7)) & 1)) any_null = true;
            }
         }
      }
      if (any_null) {
         std::vector<uint8_t> bm((size_t) ((rows + 7) / 8), 0);
         int64_t pos = 0;
         for (int64_t b = 0; b < n_batches; b++) {
            struct ArrowArray* a = batches[b]->children[c];
            const int64_t alen = batches[b]->length, aoff = batches[b]->offset + a->offset; // the parent's slice applies to every child
            const uint8_t* v = (const uint8_t*) a->buffers[0];
            for (int64_t i = 0; i < alen; i++, pos++) {
               int64_t k = i + aoff;
               bool ok = !v || ((v[k >> 3] >> (k & 7)) & 1);
               if (ok) bm[(size_t) (pos >> 3)] |= (uint8_t) (1u << (pos & 7));
               else col.null_count++;
            }
         }
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.validity, bm.size()));
         LDB_HIP(hipMemcpyAsync(col.validity, bm.data(), bm.size(), hipMemcpyHostToDevice, ctx->stream));
         LDB_HIP(hipStreamSynchronize(ctx->stream));
      }
      if (col.type.type == LDB_T_UTF8) {
         std::vector<int64_t> offs((size_t) rows + 1);
         int64_t pos = 0, bytes = 0;
         offs[0] = 0;
         for (int64_t b = 0; b < n_batches; b++) {
            struct ArrowArray* a = batches[b]->children[c];
            const int64_t alen = batches[b]->length, aoff = batches[b]->offset + a->offset; // the parent's slice applies to every child
            for (int64_t i = 0; i < alen; i++) {
               int64_t lo, hi;
               if (large) {
                  const int64_t* o = (const int64_t*) a->buffers[1] + aoff;
                  lo = o[i];
                  hi = o[i + 1];
               } else {
                  const int32_t* o = (const int32_t*) a->buffers[1] + aoff;
                  lo = o[i];
                  hi = o[i + 1];
               }
               bytes += hi - lo;
               offs[(size_t) ++pos] = bytes;
            }
         }
         col.value_bytes = bytes;
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.values, (size_t) bytes));
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.offsets, sizeof(int64_t) * ((size_t) rows + 1)));
         LDB_HIP(hipMemcpyAsync(col.offsets, offs.data(), sizeof(int64_t) * ((size_t) rows + 1), hipMemcpyHostToDevice, ctx->stream));
         int64_t dpos = 0;
         for (int64_t b = 0; b < n_batches; b++) {
            struct ArrowArray* a = batches[b]->children[c];
            const int64_t alen = batches[b]->length, aoff = batches[b]->offset + a->offset; // the parent's slice applies to every child
            if (alen == 0) continue;
            int64_t lo, hi;
            if (large) {
               const int64_t* o = (const int64_t*) a->buffers[1] + aoff;
               lo = o[0];
               hi = o[alen];
            } else {
               const int32_t* o = (const int32_t*) a->buffers[1] + aoff;
               lo = o[0];
               hi = o[alen];
            }
            if (hi > lo) LDB_HIP(hipMemcpyAsync((uint8_t*) col.values + dpos, (const uint8_t*) a->buffers[2] + lo, (size_t) (hi - lo), hipMemcpyHostToDevice, ctx->stream));
            dpos += hi - lo;
         }
         LDB_HIP(hipStreamSynchronize(ctx->stream));
      } else {
         int src_w = ldb_width_of(col.type, 0);
         if (narrow >= 2 && ldb_type_narrows(col.type)) { // the narrowest width the column's value range allows (NULL slots count too: they only ever widen it)
            int64_t lo = INT64_MAX, hi = INT64_MIN;
            for (int64_t b = 0; b < n_batches; b++) {
               struct ArrowArray* a = batches[b]->children[c];
               const int64_t alen = batches[b]->length, aoff = batches[b]->offset + a->offset;
               const uint8_t* src = (const uint8_t*) a->buffers[1] + aoff * src_w;
               for (int64_t i = 0; i < alen; i++) {
                  int64_t v = 0;
                  if (src_w == 16) {
                     memcpy(&v, src + i * 16, 8);
                  } else {
                     int32_t w32;
                     memcpy(&w32, src + i * 4, 4);
                     v = w32;
                  }
                  lo = std::min(lo, v);
                  hi = std::max(hi, v);
               }
            }
            if (lo > hi) lo = hi = 0;
            col.width = ldb_narrowest_width(lo, hi);
            if (col.type.type == LDB_T_CHAR4 && (col.width > 1 || lo < 0)) col.width = 4; // (a byte >= 0x80 or a second character: the four raw bytes stay)
         }
         col.value_bytes = rows * col.width;
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.values, (size_t) col.value_bytes));
         int64_t pos = 0;
         std::vector<int64_t> tmp;
         for (int64_t b = 0; b < n_batches; b++) {
            struct ArrowArray* a = batches[b]->children[c];
            const int64_t alen = batches[b]->length, aoff = batches[b]->offset + a->offset; // the parent's slice applies to every child
            if (alen == 0) continue;
            const uint8_t* src = (const uint8_t*) a->buffers[1] + aoff * src_w;
            if (src_w == col.width) {
               LDB_HIP(hipMemcpyAsync((uint8_t*) col.values + pos * col.width, src, (size_t) (alen * src_w), hipMemcpyHostToDevice, ctx->stream));
            } else { // narrowed column: keep the low `width` bytes (little-endian two's complement: the value fits)
               const size_t w = (size_t) col.width;
               tmp.resize((size_t) ((alen * (int64_t) w + 7) / 8));
               uint8_t* dstb = (uint8_t*) tmp.data();
               for (int64_t i = 0; i < alen; i++) memcpy(dstb + (size_t) i * w, src + i * src_w, w);
               LDB_HIP(hipMemcpyAsync((uint8_t*) col.values + pos * (int64_t) w, tmp.data(), (size_t) alen * w, hipMemcpyHostToDevice, ctx->stream));
               LDB_HIP(hipStreamSynchronize(ctx->stream));
            }
            pos += alen;
         }
         LDB_HIP(hipStreamSynchronize(ctx->stream));
      }
   }
   LDB_TRY(ldb_table_dict_encode_all(ctx, t.t)); // low-cardinality utf8 columns get an order-preserving dictionary
   *out = t.release();
   return LDB_OK;
}

extern "C" int32_t ldb_gpu_table_alloc(ldb_ctx* ctx, const char* name, int32_t n_cols, const ldb_coltype* types, const char* const* col_names,
                                       int64_t n_rows, const int64_t* data_bytes, int32_t narrow, ldb_table** out) {
   if (!ctx || !out || n_cols < 0) LDB_FAIL(LDB_ERR_INVALID, "table_alloc: bad argument");
   if (n_rows >= (int64_t) LDB_NULL_ROW) LDB_FAIL(LDB_ERR_UNSUPPORTED, "table_alloc: %ld rows exceed uint32 row ids", (long) n_rows);
   LdbTableHold t(ctx, new ldb_table());
   t->ctx = ctx;
   t->name = name ? name : "";
   t->n_rows = n_rows;
   t->cols.resize((size_t) n_cols);
   for (int32_t c = 0; c < n_cols; c++) {
      ldb_column& col = t->cols[(size_t) c];
      col.name = col_names && col_names[c] ? col_names[c] : "";
      col.type = types[c];
      col.width = ldb_width_of(col.type, narrow);
      if (col.type.type == LDB_T_UTF8) {
         col.value_bytes = data_bytes ? data_bytes[c] : 0;
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.values, (size_t) col.value_bytes));
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.offsets, sizeof(int64_t) * ((size_t) n_rows + 1)));
      } else {
         col.value_bytes = n_rows * col.width;
         LDB_TRY(LdbBufs::alloc_into(ctx, &col.values, (size_t) col.value_bytes));
      }
   }
   *out = t.release();
   return LDB_OK;
}
// The table's hash index over `cols` (primary key): built on first use with ldb_gpu_join_build over ALL rows, owned by the
// table, released with it.  Replaces the reference's persisted LingoDBHashIndex (LingoDBHashIndex.h:18-61: hash → row id,
// looked up by index nested-loop joins when the inner side is a bare base table whose primary key equals the join
// columns, translateINLJ RelAlgToSubOp.cpp:1129-1205, OptimizeImplementations.cpp:226-245): here the index IS a join
// table — for a dense primary key the rank-bitmap layout, range / 4 bytes — so probing it is the ordinary probe.
extern "C" int32_t ldb_gpu_table_index(ldb_ctx* ctx, ldb_table* t, const int32_t* cols, int32_t n_cols, ldb_hashtable** out) {
   if (!ctx || !t || !cols || !out || n_cols < 1 || n_cols > LDB_MAX_KEYS) LDB_FAIL(LDB_ERR_INVALID, "table_index: bad argument");
   for (auto& ix : t->indexes)
      if (ix.cols.size() == (size_t) n_cols && std::equal(ix.cols.begin(), ix.cols.end(), cols)) {
         *out = ix.ht;
         return LDB_OK;
      }
   ldb_table::Index ix;
   ix.cols.assign(cols, cols + n_cols);
   std::vector<ldb_colref> keys;
   for (int32_t k = 0; k < n_cols; k++) {
      if (cols[k] < 0 || (size_t) cols[k] >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "table_index: column %d out of range", cols[k]);
      keys.push_back({0, cols[k]});
   }
   LDB_TRY(ldb_gpu_rel_from_table(ctx, t, &ix.rel));
   const int32_t st = ldb_gpu_join_build(ctx, ix.rel, keys.data(), n_cols, 1, &ix.ht);
   if (st != LDB_OK) {
      ldb_gpu_rel_release(ctx, ix.rel);
      return st;
   }
   t->indexes.push_back(ix);
   *out = ix.ht;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_release(ldb_ctx* ctx, ldb_table* t) {
   if (!t) return LDB_OK;
   for (auto& ix : t->indexes) {
      ldb_gpu_hashtable_release(ctx, ix.ht);
      ldb_gpu_rel_release(ctx, ix.rel);
   }
   t->indexes.clear();
   for (auto& c : t->cols) {
      if (!c.owned) continue;
      ldb_dev_free(ctx, c.values);
      ldb_dev_free(ctx, c.offsets);
      ldb_dev_free(ctx, c.validity);
      ldb_dev_free(ctx, c.zone_min);
      ldb_dev_free(ctx, c.zone_max);
      ldb_column_dict_release(ctx, c);
   }
   delete t;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_rename_col(ldb_table* t, int32_t col, const char* name) {
   if (!t || !name || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "rename_col: bad argument");
   t->cols[(size_t) col].name = name;
   return LDB_OK;
}
extern "C" int64_t ldb_gpu_table_rows(const ldb_table* t) { return t ? t->n_rows : -1; }
extern "C" int32_t ldb_gpu_table_cols(const ldb_table* t) { return t ? (int32_t) t->cols.size() : -1; }
extern "C" int32_t ldb_gpu_table_coltype(const ldb_table* t, int32_t col, ldb_coltype* out) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "coltype: bad column %d", col);
   *out = t->cols[(size_t) col].type;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_col_index(const ldb_table* t, const char* name) {
   for (size_t i = 0; i < t->cols.size(); i++)
      if (t->cols[i].name == name) return (int32_t) i;
   return -1;
}
extern "C" const char* ldb_gpu_table_col_name(const ldb_table* t, int32_t col) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) return nullptr;
   return t->cols[(size_t) col].name.c_str();
}
extern "C" int32_t ldb_gpu_table_col_width(const ldb_table* t, int32_t col) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) return -1;
   return t->cols[(size_t) col].width;
}
extern "C" int32_t ldb_gpu_table_col_ptrs(const ldb_table* t, int32_t col, void** values, void** offsets, void** validity, int64_t* value_bytes) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "col_ptrs: bad column %d", col);
   const ldb_column& c = t->cols[(size_t) col];
   if (ldb_column_is_lazy(c)) LDB_TRY(ldb_column_strings(t->ctx, c, t->n_rows));
   c.has_range = false, c.sorted_state = -1, c.skewed = false; // the caller may write through the raw pointers
   if (values) *values = c.values;
   if (offsets) *offsets = c.offsets;
   if (validity) *validity = c.validity;
   if (value_bytes) *value_bytes = c.value_bytes;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_set_rows(ldb_table* t, int64_t n_rows) {
   if (!t || n_rows < 0) LDB_FAIL(LDB_ERR_INVALID, "set_rows: bad argument");
   for (auto& c : t->cols)
      if (c.type.type != LDB_T_UTF8 && n_rows * c.width > c.value_bytes) LDB_FAIL(LDB_ERR_INVALID, "set_rows: %ld rows exceed capacity of column %s", (long) n_rows, c.name.c_str());
   t->n_rows = n_rows;
   t->serial = ldb_next_serial();
   for (auto& c : t->cols) c.has_range = false, c.sorted_state = -1, c.skewed = false;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_read_fixed(ldb_ctx* ctx, const ldb_table* t, int32_t col, void* host_out, int64_t out_bytes) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "read_fixed: bad column %d", col);
   const ldb_column& c = t->cols[(size_t) col];
   if (c.type.type == LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "read_fixed: column %s is utf8 (use export)", c.name.c_str());
   int64_t need = t->n_rows * c.width;
   if (out_bytes < need) LDB_FAIL(LDB_ERR_INVALID, "read_fixed: buffer %ld < %ld bytes", (long) out_bytes, (long) need);
   // (a scalar-subquery result read by the plan layer is a read-back like any count: recorded / replayed inside a trace)
   if (need) return LDB_READBACK(ctx, host_out, c.values, (size_t) need);
   LDB_HIP(hipStreamSynchronize(ctx->stream));
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_row_valid(ldb_ctx* ctx, const ldb_table* t, int32_t col, int64_t row, int32_t* valid) {
   if (!ctx || !t || !valid || col < 0 || (size_t) col >= t->cols.size() || row < 0 || row >= t->n_rows) LDB_FAIL(LDB_ERR_INVALID, "row_valid: bad argument");
   const ldb_column& c = t->cols[(size_t) col];
   *valid = 1;
   if (!c.validity) return LDB_OK;
   uint8_t byte = 0xFF;
   LDB_TRY(LDB_READBACK(ctx, &byte, c.validity + (row >> 3), 1));
   *valid = (byte >> (row & 7)) & 1;
   return LDB_OK;
}
extern "C" int32_t ldb_gpu_table_write_fixed(ldb_ctx* ctx, ldb_table* t, int32_t col, const void* host_in, int64_t in_bytes) {
   if (!t || col < 0 || (size_t) col >= t->cols.size()) LDB_FAIL(LDB_ERR_INVALID, "write_fixed: bad column %d", col);
   ldb_column& c = t->cols[(size_t) col];
   if (c.type.type == LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "write_fixed: column %s is utf8", c.name.c_str());
   if (in_bytes > c.value_bytes) LDB_FAIL(LDB_ERR_INVALID, "write_fixed: %ld bytes exceed column capacity %ld", (long) in_bytes, (long) c.value_bytes);
   if (in_bytes) LDB_HIP(hipMemcpyAsync(c.values, host_in, (size_t) in_bytes, hipMemcpyHostToDevice, ctx->stream));
   LDB_HIP(hipStreamSynchronize(ctx->stream));
   c.has_range = false, c.sorted_state = -1, c.skewed = false;
   t->serial = ldb_next_serial();
   return LDB_OK;
}

extern "C" int32_t ldb_gpu_memcpy_d2d(ldb_ctx* ctx, void* dst, const void* src, int64_t bytes) {
   if (!ctx || bytes < 0 || (bytes && (!dst || !src))) LDB_FAIL(LDB_ERR_INVALID, "memcpy_d2d: bad argument");
   if (bytes) LDB_HIP(hipMemcpyAsync(dst, src, (size_t) bytes, hipMemcpyDeviceToDevice, ctx->stream));
   return LDB_OK;
}

// ---------------------------------------------------------------- export (Arrow C Data Interface out)
struct ExportPriv {
   std::vector<void*> bufs;
   std::vector<struct ArrowArray*> child_arrays;
   std::vector<struct ArrowSchema*> child_schemas;
   std::vector<char*> strings;
   const void** buffers = nullptr;
};
static void release_array(struct ArrowArray* a) {
   if (!a || !a->release) return;
   ExportPriv* p = (ExportPriv*) a->private_data;
   for (int64_t i = 0; i < a->n_children; i++) {
      if (a->children[i]->release) a->children[i]->release(a->children[i]);
      free(a->children[i]);
   }
   free(a->children);
   for (void* b : p->bufs) free(b);
   free(p->buffers);
   delete p;
   a->release = nullptr;
}
static void release_schema(struct ArrowSchema* s) {
   if (!s || !s->release) return;
   ExportPriv* p = (ExportPriv*) s->private_data;
   for (int64_t i = 0; i < s->n_children; i++) {
      if (s->children[i]->release) s->children[i]->release(s->children[i]);
      free(s->children[i]);
   }
   free(s->children);
   for (char* c : p->strings) free(c);
   delete p;
   s->release = nullptr;
}
static char* dup_str(ExportPriv* p, const std::string& s) {
   char* c = strdup(s.c_str());
   p->strings.push_back(c);
   return c;
}

// all buffers of a small result → the pinned ring in ONE launch (a hipMemcpyAsync per buffer was 10 – 17 copy launches for a
// TPC-H result with string columns): workgroup b copies buffer b, 8 bytes per lane and step
struct DExportPack {
   int32_t n, pad;
   const uint8_t* src[32];
   uint8_t* dst[32];
   uint64_t bytes[32];
};
__global__ __launch_bounds__(256) void k_export_pack(DExportPack d) {
   const int b = blockIdx.x;
   if (b >= d.n) return;
   const uint64_t words = d.bytes[b] / 8;
   const uint64_t* s8 = (const uint64_t*) d.src[b];
   uint64_t* d8 = (uint64_t*) d.dst[b];
   for (uint64_t i = threadIdx.x; i < words; i += 256) d8[i] = s8[i];
   for (uint64_t i = words * 8 + threadIdx.x; i < d.bytes[b]; i += 256) d.dst[b][i] = d.src[b][i];
}
extern "C" int32_t ldb_gpu_export(ldb_ctx* ctx, const ldb_table* t, struct ArrowSchema* out_schema, struct ArrowArray* out_array) {
   if (!ctx || !t || !out_schema || !out_array) LDB_FAIL(LDB_ERR_INVALID, "export: NULL argument");
   const int64_t n = t->n_rows;
   const int64_t nc = (int64_t) t->cols.size();
   for (auto& col : t->cols)
      if (ldb_column_is_lazy(col)) LDB_TRY(ldb_column_strings(ctx, col, n)); // (dictionary-coded strings are written out only here)
   // Small results (the usual case: a query's final rows) come over in ONE batch: every device
   // buffer is copied asynchronously into the pinned ring, one synchronize, then plain memcpys —
   // instead of a blocking pageable hipMemcpy (~20 µs) per buffer.
   struct Staged {
      const uint8_t *validity = nullptr, *offsets = nullptr, *values = nullptr;
   };
   std::vector<Staged> staged((size_t) nc);
   {
      auto pad = [](size_t b) { return (b + 63) & ~(size_t) 63; };
      size_t total = 0;
      bool ok = ctx->mem.h_ring != nullptr && n <= 65536;
      for (int64_t c = 0; c < nc && ok; c++) {
         const ldb_column& col = t->cols[(size_t) c];
         if (col.validity) total += pad((size_t) ((n + 7) / 8));
         if (col.type.type == LDB_T_UTF8) {
            if (col.value_bytes < 0) ok = false;
            total += pad(sizeof(int64_t) * ((size_t) n + 1)) + pad((size_t) col.value_bytes);
         } else {
            total += pad((size_t) n * (size_t) col.width);
         }
      }
      if (ok && total <= LDB_RING_BYTES / 4 && n > 0) {
         if (ctx->mem.ring_pos + total > LDB_RING_BYTES) {
            LDB_HIP(hipStreamSynchronize(ctx->stream));
            ctx->mem.ring_pos = 0;
         }
         DExportPack pack;
         memset(&pack, 0, sizeof(pack));
         auto flush = [&]() {
            if (pack.n) hipLaunchKernelGGL(k_export_pack, dim3((unsigned) pack.n), dim3(256), 0, ctx->stream, pack);
            pack.n = 0;
         };
         auto fetch = [&](const void* src, size_t bytes, const uint8_t** slot_out) -> int32_t {
            if (!bytes) return LDB_OK;
            uint8_t* slot = ctx->mem.h_ring + ctx->mem.ring_pos;
            ctx->mem.ring_pos += pad(bytes);
            if (((uintptr_t) src & 7) == 0) { // (device buffers are 256-byte aligned; a view's base need not be)
               if (pack.n == 32) flush();
               pack.src[pack.n] = (const uint8_t*) src;
               pack.dst[pack.n] = slot;
               pack.bytes[pack.n] = bytes;
               pack.n++;
            } else {
               LDB_HIP(hipMemcpyAsync(slot, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
            }
            *slot_out = slot;
            return LDB_OK;
         };
         for (int64_t c = 0; c < nc; c++) {
            const ldb_column& col = t->cols[(size_t) c];
            Staged& st = staged[(size_t) c];
            if (col.validity) LDB_TRY(fetch(col.validity, (size_t) ((n + 7) / 8), &st.validity));
            if (col.type.type == LDB_T_UTF8) {
               LDB_TRY(fetch(col.offsets, sizeof(int64_t) * ((size_t) n + 1), &st.offsets));
               LDB_TRY(fetch(col.values, (size_t) col.value_bytes, &st.values));
            } else {
               LDB_TRY(fetch(col.values, (size_t) n * (size_t) col.width, &st.values));
            }
         }
         flush();
         LDB_HIP(hipGetLastError());
      }
   }
   LDB_HIP(hipStreamSynchronize(ctx->stream));
   auto d2h = [&](void* dst, const void* src, size_t bytes, const uint8_t* from_ring) -> int32_t {
      if (!bytes) return LDB_OK;
      if (from_ring) {
         memcpy(dst, from_ring, bytes);
         return LDB_OK;
      }
      LDB_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
      return LDB_OK;
   };
   memset(out_schema, 0, sizeof(*out_schema));
   memset(out_array, 0, sizeof(*out_array));
   auto* sp = new ExportPriv();
   out_schema->format = dup_str(sp, "+s");
   out_schema->name = dup_str(sp, t->name);
   out_schema->n_children = nc;
   out_schema->children = (struct ArrowSchema**) calloc((size_t) (nc ? nc : 1), sizeof(void*));
   out_schema->release = release_schema;
   out_schema->private_data = sp;
   auto* ap = new ExportPriv();
   ap->buffers = (const void**) calloc(1, sizeof(void*));
   out_array->length = n;
   out_array->n_buffers = 1;
   out_array->buffers = ap->buffers;
   out_array->n_children = nc;
   out_array->children = (struct ArrowArray**) calloc((size_t) (nc ? nc : 1), sizeof(void*));
   out_array->release = release_array;
   out_array->private_data = ap;
   for (int64_t c = 0; c < nc; c++) {
      const ldb_column& col = t->cols[(size_t) c];
      auto* cs = (struct ArrowSchema*) calloc(1, sizeof(struct ArrowSchema));
      auto* ca = (struct ArrowArray*) calloc(1, sizeof(struct ArrowArray));
      out_schema->children[c] = cs;
      out_array->children[c] = ca;
      auto* csp = new ExportPriv();
      auto* cap = new ExportPriv();
      cs->release = release_schema;
      cs->private_data = csp;
      cs->children = nullptr;
      ca->release = release_array;
      ca->private_data = cap;
      cs->name = dup_str(csp, col.name);
      cs->flags = ARROW_FLAG_NULLABLE;
      ca->length = n;
      ca->null_count = col.validity ? col.null_count : 0;
      char fmt[64];
      bool utf8 = col.type.type == LDB_T_UTF8;
      bool large = false;
      switch (col.type.type) {
         case LDB_T_INT8: strcpy(fmt, "c"); break;
         case LDB_T_BOOL8: strcpy(fmt, "C"); break; // uint8 0/1
         case LDB_T_INT16: strcpy(fmt, "s"); break;
         case LDB_T_INT32: strcpy(fmt, "i"); break;
         case LDB_T_INT64: strcpy(fmt, "l"); break;
         case LDB_T_DATE32: strcpy(fmt, "tdD"); break;
         case LDB_T_FLOAT64: strcpy(fmt, "g"); break;
         case LDB_T_FLOAT32: strcpy(fmt, "f"); break;
         case LDB_T_CHAR4: strcpy(fmt, "w:4"); break;
         case LDB_T_DECIMAL128: snprintf(fmt, sizeof(fmt), "d:%d,%d", col.type.precision, col.type.scale); break;
         case LDB_T_UTF8:
            large = col.value_bytes > 0x7fffffffLL;
            strcpy(fmt, large ? "U" : "u");
            break;
         default: LDB_FAIL(LDB_ERR_UNSUPPORTED, "export: column type %d", col.type.type);
      }
      cs->format = dup_str(csp, fmt);
      ca->n_buffers = utf8 ? 3 : 2;
      cap->buffers = (const void**) calloc(3, sizeof(void*));
      ca->buffers = cap->buffers;
      if (col.validity) {
         size_t vb = (size_t) ((n + 7) / 8);
         void* hv = malloc(vb ? vb : 1);
         cap->bufs.push_back(hv);
         LDB_TRY(d2h(hv, col.validity, vb, staged[(size_t) c].validity));
         cap->buffers[0] = hv;
      }
      if (utf8) {
         std::vector<int64_t> offs((size_t) n + 1, 0);
         LDB_TRY(d2h(offs.data(), col.offsets, sizeof(int64_t) * ((size_t) n + 1), staged[(size_t) c].offsets));
         int64_t bytes = offs[(size_t) n];
         void* data = malloc((size_t) (bytes ? bytes : 1));
         cap->bufs.push_back(data);
         LDB_TRY(d2h(data, col.values, (size_t) bytes, bytes <= col.value_bytes ? staged[(size_t) c].values : nullptr));
         if (large) {
            void* ho = malloc(sizeof(int64_t) * ((size_t) n + 1));
            memcpy(ho, offs.data(), sizeof(int64_t) * ((size_t) n + 1));
            cap->bufs.push_back(ho);
            cap->buffers[1] = ho;
         } else {
            int32_t* ho = (int32_t*) malloc(sizeof(int32_t) * ((size_t) n + 1));
            for (int64_t i = 0; i <= n; i++) ho[i] = (int32_t) offs[(size_t) i];
            cap->bufs.push_back(ho);
            cap->buffers[1] = ho;
         }
         cap->buffers[2] = data;
      } else {
         int out_w = ldb_width_of(col.type, 0);
         size_t bytes = (size_t) (n * out_w);
         uint8_t* hv = (uint8_t*) malloc(bytes ? bytes : 1);
         cap->bufs.push_back(hv);
         if (out_w == col.width) {
            LDB_TRY(d2h(hv, col.values, bytes, staged[(size_t) c].values));
         } else { // narrowed column → sign-extend back to its Arrow width (decimal128: reference LowerToStd.cpp:211-298; char(1): its byte + three zero bytes)
            const size_t w = (size_t) col.width;
            std::vector<uint8_t> tmp((size_t) n * w + 8);
            LDB_TRY(d2h(tmp.data(), col.values, (size_t) n * w, staged[(size_t) c].values));
            for (int64_t i = 0; i < n; i++) {
               int64_t lo = 0;
               switch (w) {
                  case 1: lo = (int8_t) tmp[(size_t) i]; break;
                  case 2: { int16_t v; memcpy(&v, tmp.data() + (size_t) i * 2, 2); lo = v; break; }
                  case 4: { int32_t v; memcpy(&v, tmp.data() + (size_t) i * 4, 4); lo = v; break; }
                  default: memcpy(&lo, tmp.data() + (size_t) i * 8, 8); break;
               }
               const int64_t hi = lo >> 63;
               memcpy(hv + i * out_w, &lo, (size_t) std::min(out_w, 8));
               if (out_w == 16) memcpy(hv + i * 16 + 8, &hi, 8);
            }
         }
         cap->buffers[1] = hv;
      }
   }
   return LDB_OK;
}
