// ldb_expr.hip — general scalar projection: computed columns from expression programs, substr.
// Replaces (reference): the per-tuple scalar code the DB dialect lowers inside `subop.map`
// (src/compiler/Conversion/DBToStd/LowerToStd.cpp): DecimalBinOpLowering / DecimalMulOpLowering /
// DecimalOpScaledLowering (:622-699), the comparison lowerings (:374-466), `scf.if` on
// db.derive_truth for CASE (:1022-1045), NULL propagation (NullHandler), and the runtime call
// StringRuntime::substr (src/runtime/StringRuntime.cpp:292-319).
//
// An expression arrives as a POSTFIX program (ldb_xinstr[]) over the columns of a relation.  It is
// evaluated per row on a small stack of nullable 128-bit integers in wrapping arithmetic — the
// value domain of every integer / decimal / date / bool the generated code computes with; the
// caller has already fixed the scales (casts are MUL_POW10 / SDIV_POW10), exactly as the frontend
// inserts db.cast before db.add / db.compare (sql_analyzer.cpp:3058-3159).
#include "ldb_internal.h"
#include "ldb_device.h"
#include <memory>

#include "ldb_expr_kernel.h"
#include "ldb_fexpr_kernel.h"
#include "ldb_strfn.h"
#include "ldb_jit.h"

__global__ void k_pack_bytes_to_bits_x(const uint8_t* __restrict__ bytes, uint8_t* __restrict__ bitmap, uint64_t n) {
   const uint64_t nb = (n + 7) / 8;
   for (uint64_t b = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; b < nb; b += (uint64_t) gridDim.x * blockDim.x) {
      uint8_t m = 0;
      for (int k = 0; k < 8; k++)
         if (b * 8 + k < n && bytes[b * 8 + k]) m |= (uint8_t) (1u << k);
      bitmap[b] = m;
   }
}

__global__ void k_map_expr(const DXProg* __restrict__ prog, uint64_t n, void* __restrict__ out, uint8_t* __restrict__ valid_bytes) { map_expr_body(*prog, prog, n, out, valid_bytes); }
// run-time specialised variant (hiprtc): the program — opcodes, constants, column types — as compile-time constants, so the
// interpreter loop unrolls into straight-line code and the value stack lives in registers
static const char* XPR_SPEC_SRC =
   "extern \"C\" __global__ void k_map_expr_spec(const DXProg* __restrict__ prog, uint64_t n, void* __restrict__ out, uint8_t* __restrict__ valid_bytes) {\n"
   "   map_expr_body(LDB_META, prog, n, out, valid_bytes);\n"
   "}\n";
bool ldb_expr_jit_check(std::string* log) { // coalesce(count, 0) * 2 <= 10 over a nullable int64 column
   auto m = std::make_unique<DXProg>();
   memset(m.get(), 0, sizeof(DXProg));
   const int32_t ops[] = {LDB_X_COL, LDB_X_CONST, LDB_X_COALESCE, LDB_X_CONST, LDB_X_MUL, LDB_X_CONST, LDB_X_CMP};
   m->n = 7;
   m->out_width = 1;
   for (int k = 0; k < 7; k++) m->ins[k].op = ops[k];
   m->ins[0].col.type = LDB_T_INT64;
   m->ins[0].col.width = 8;
   m->ins[0].col.validity = 1;
   m->ins[3].lo = 2;
   m->ins[5].lo = 10;
   m->ins[6].arg = LDB_F_LTE;
   return ldb_jit_compile_only("ldb_expr_kernel.h", "DXProg", XPR_SPEC_SRC, m.get(), sizeof(DXProg), log);
}

// ---- programs that compute with floats (ldb_fexpr_kernel.h): typed slots, validity written as bitmap words by the kernel
__global__ void k_map_fexpr(const DFProg* __restrict__ prog, uint64_t n, void* __restrict__ out, uint64_t* __restrict__ valid_words) { map_fexpr_body(*prog, prog, n, out, valid_words); }
static const char* FXPR_SPEC_SRC =
   "extern \"C\" __global__ void k_map_fexpr_spec(const DFProg* __restrict__ prog, uint64_t n, void* __restrict__ out, uint64_t* __restrict__ valid_words) {\n"
   "   map_fexpr_body(LDB_META, prog, n, out, valid_words);\n"
   "}\n";
static uint64_t f64_bits(double v) {
   uint64_t b;
   memcpy(&b, &v, 8);
   return b;
}
static uint64_t f32_bits(float v) {
   uint32_t b;
   memcpy(&b, &v, 4);
   return b;
}
bool ldb_fexpr_jit_check(std::string* log) { // cast(a * b + c as double) < 0.5 over nullable f32 columns
   auto m = std::make_unique<DFProg>();
   memset(m.get(), 0, sizeof(DFProg));
   const int32_t ops[] = {LDB_X_COL, LDB_X_COL, LDB_X_FMUL, LDB_X_COL, LDB_X_FADD, LDB_X_FCVT, LDB_X_FCONST, LDB_X_FCMP};
   m->n = 8;
   m->out_width = 1;
   for (int k = 0; k < 8; k++) {
      m->ins[k].op = ops[k];
      m->ins[k].cls = k < 6 ? LDB_XT_F32 : LDB_XT_F64;
      if (ops[k] == LDB_X_COL) {
         m->ins[k].col.type = LDB_T_FLOAT32;
         m->ins[k].col.width = 4;
         m->ins[k].col.validity = 1;
      }
   }
   m->ins[5].arg = 64;
   m->ins[6].arg = 64;
   m->ins[6].lo = f64_bits(0.5);
   m->ins[7].arg = LDB_F_LT;
   return ldb_jit_compile_only("ldb_fexpr_kernel.h", "DFProg", FXPR_SPEC_SRC, m.get(), sizeof(DFProg), log);
}

static int32_t map_fexpr_launch(ldb_ctx* ctx, const DFProg* hp, int64_t n, ldb_table* res) {
   // one 64-bit word per 64 rows, written whole by the wave that holds those rows
   LDB_TRY(LdbBufs::alloc_into(ctx, &res->cols[0].validity, (size_t) ((n + 63) / 64 + 1) * 8));
   uint64_t* bm = (uint64_t*) res->cols[0].validity;
   if (n) {
      const int grid = ldb_grid_for(ctx, (n + FX_ROWS - 1) / FX_ROWS, 256, 8);
      LdbDesc<DFProg> d_desc(ctx);
      LDB_TRY(d_desc.upload(hp, sizeof(DFProg)));
      DFProg* d = d_desc.p;
      hipFunction_t spec = nullptr;
      if (ldb_jit_wanted(n)) {
         auto meta = std::make_unique<DFProg>();
         memcpy(meta.get(), hp, sizeof(DFProg));
         for (int k = 0; k < LDB_MAX_XPROG; k++) ldb_jit_strip_col(meta->ins[k].col);
         std::string why;
         spec = ldb_jit_kernel(ctx->device, "ldb_fexpr_kernel.h", "DFProg", FXPR_SPEC_SRC, "k_map_fexpr_spec", meta.get(), sizeof(DFProg), &why);
      }
      {
         LdbProf prof_(ctx, "k_map_fexpr");
         if (spec) {
            uint64_t nn = (uint64_t) n;
            void* ov = res->cols[0].values;
            void* params[] = {(void*) &d, (void*) &nn, (void*) &ov, (void*) &bm};
            LDB_HIP(hipModuleLaunchKernel(spec, (unsigned) grid, 1, 1, 256, 1, 1, 0, ctx->stream, params, nullptr));
         } else {
            hipLaunchKernelGGL(k_map_fexpr, dim3(grid), dim3(256), 0, ctx->stream, (const DFProg*) d, (uint64_t) n, res->cols[0].values, bm);
         }
      }
      d_desc.release();
   }
   res->cols[0].null_count = -1; // unknown (Arrow convention)
   res->cols[0].type.nullable = 1;
   LDB_HIP(hipGetLastError());
   return LDB_OK;
}

static const char* xt_name(int t) { return t == LDB_XT_F32 ? "f32" : t == LDB_XT_F64 ? "f64" : t == LDB_XT_BOOL ? "bool" : "integer"; }
static inline bool xt_is_float(int t) { return t == LDB_XT_F32 || t == LDB_XT_F64; }

extern "C" int32_t ldb_gpu_map_expr(ldb_ctx* ctx, ldb_rel* in, const ldb_xinstr* prog, int32_t n_instr, ldb_coltype out_type, const char* name, ldb_table** out) {
   if (!ctx || !in || !prog || !out) LDB_FAIL(LDB_ERR_INVALID, "map_expr: NULL argument");
   if (n_instr < 1 || n_instr > LDB_MAX_XPROG) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_expr: %d instructions (max %d)", n_instr, LDB_MAX_XPROG);
   switch (out_type.type) {
      case LDB_T_INT32:
      case LDB_T_INT64:
      case LDB_T_DATE32:
      case LDB_T_DECIMAL128:
      case LDB_T_BOOL8:
      case LDB_T_FLOAT32:
      case LDB_T_FLOAT64: break;
      default: LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_expr: result type %d (integer, date, decimal, bool or float expected)", out_type.type);
   }
   const int out_cls = out_type.type == LDB_T_FLOAT32 ? LDB_XT_F32 : out_type.type == LDB_T_FLOAT64 ? LDB_XT_F64 : LDB_XT_INT;
   LDB_TRY(ldb_rel_force(ctx, in));
   auto fp = std::make_unique<DFProg>();
   memset(fp.get(), 0, sizeof(DFProg));
   fp->n = n_instr;
   // verify the program on the host: stack depth and the class of every slot (integer, bool, f32, f64)
   int depth = 0;
   int ty[XSTACK + 1];
   bool has_float = xt_is_float(out_cls);
   for (int32_t k = 0; k < n_instr; k++) {
      DFInstr& x = fp->ins[k];
      x.op = prog[k].op;
      x.arg = prog[k].arg;
      x.lo = (uint64_t) prog[k].lo;
      x.hi = prog[k].hi;
      int pops = 0;
      switch (x.op) {
         case LDB_X_COL:
         case LDB_X_CONST:
         case LDB_X_ROW:
         case LDB_X_FCONST: break;
         case LDB_X_ADD:
         case LDB_X_SUB:
         case LDB_X_MUL:
         case LDB_X_SDIV:
         case LDB_X_AND:
         case LDB_X_OR:
         case LDB_X_COALESCE:
         case LDB_X_CMP:
         case LDB_X_FADD:
         case LDB_X_FSUB:
         case LDB_X_FMUL:
         case LDB_X_FDIV:
         case LDB_X_FCMP: pops = 2; break;
         case LDB_X_MUL_POW10:
         case LDB_X_SDIV_POW10:
         case LDB_X_NEG:
         case LDB_X_NOT:
         case LDB_X_ISNULL:
         case LDB_X_I2F:
         case LDB_X_F2I:
         case LDB_X_FCVT: pops = 1; break;
         case LDB_X_SELECT: pops = 3; break;
         default: LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: unknown op %d", k, x.op);
      }
      if (depth < pops) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d pops %d of %d stack entries", k, pops, depth);
      const int* top = ty + depth - pops; // the operands, bottom first
      int push = LDB_XT_INT;
      auto need_int = [&](int from) -> bool {
         for (int j = from; j < pops; j++)
            if (xt_is_float(top[j])) return false;
         return true;
      };
      switch (x.op) {
         case LDB_X_COL: {
            LDB_TRY(ldb_make_dcol(in, prog[k].col, &x.col));
            if (x.col.type == LDB_T_UTF8) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_expr: instruction %d: integer / decimal / date / bool / float columns only", k);
            push = x.col.type == LDB_T_FLOAT32 ? LDB_XT_F32 : x.col.type == LDB_T_FLOAT64 ? LDB_XT_F64 : x.col.type == LDB_T_BOOL8 ? LDB_XT_BOOL : LDB_XT_INT;
            x.cls = push;
            break;
         }
         case LDB_X_CONST:
         case LDB_X_ROW: break;
         case LDB_X_FCONST: {
            if (x.arg != 32 && x.arg != 64) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: float width %d (32 or 64)", k, x.arg);
            if (x.arg == 32) { // the slot holds the constant at its own width
               double v;
               memcpy(&v, &x.lo, 8);
               x.lo = f32_bits((float) v);
            }
            x.hi = 0;
            push = x.arg == 32 ? LDB_XT_F32 : LDB_XT_F64;
            break;
         }
         case LDB_X_CMP:
            if (x.arg < LDB_F_EQ || x.arg > LDB_F_GTE) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: bad comparison %d", k, x.arg);
            if (!need_int(0)) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: integer comparison of %s and %s (floats compare with FCMP)", k, xt_name(top[0]), xt_name(top[1]));
            push = LDB_XT_BOOL;
            break;
         case LDB_X_MUL_POW10:
         case LDB_X_SDIV_POW10:
            if (x.arg < 0 || x.arg > 38) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: exponent %d", k, x.arg);
            [[fallthrough]];
         case LDB_X_ADD:
         case LDB_X_SUB:
         case LDB_X_MUL:
         case LDB_X_SDIV:
         case LDB_X_NEG:
            if (!need_int(0)) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: a float operand under an integer instruction (op %d)", k, x.op);
            break;
         case LDB_X_AND:
         case LDB_X_OR:
         case LDB_X_NOT:
            if (!need_int(0)) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: a float operand under a boolean instruction (op %d)", k, x.op);
            push = LDB_XT_BOOL;
            break;
         case LDB_X_ISNULL: push = LDB_XT_BOOL; break;
         case LDB_X_SELECT:
         case LDB_X_COALESCE: {
            const int a = top[pops - 2], b = top[pops - 1];
            if (x.op == LDB_X_SELECT && xt_is_float(top[0])) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: a float condition", k);
            if ((xt_is_float(a) || xt_is_float(b)) && a != b) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: value operands of different classes (%s, %s)", k, xt_name(a), xt_name(b));
            push = a == b ? a : LDB_XT_INT;
            x.cls = push;
            break;
         }
         case LDB_X_FADD:
         case LDB_X_FSUB:
         case LDB_X_FMUL:
         case LDB_X_FDIV:
         case LDB_X_FCMP:
            if (!xt_is_float(top[0]) || !xt_is_float(top[1])) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: float instruction over %s and %s", k, xt_name(top[0]), xt_name(top[1]));
            if (top[0] != top[1]) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: mixed float widths (%s, %s)", k, xt_name(top[0]), xt_name(top[1]));
            if (x.op == LDB_X_FCMP && (x.arg < LDB_F_EQ || x.arg > LDB_F_GTE)) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: bad comparison %d", k, x.arg);
            x.cls = top[0];
            push = x.op == LDB_X_FCMP ? LDB_XT_BOOL : top[0];
            break;
         case LDB_X_I2F:
            if (x.arg != 32 && x.arg != 64) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: float width %d (32 or 64)", k, x.arg);
            if (xt_is_float(top[0])) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: I2F of a float (FCVT converts between widths)", k);
            push = x.arg == 32 ? LDB_XT_F32 : LDB_XT_F64;
            break;
         case LDB_X_F2I:
            if (!xt_is_float(top[0])) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: F2I of an %s", k, xt_name(top[0]));
            x.cls = top[0];
            break;
         default: // LDB_X_FCVT
            if (x.arg != 32 && x.arg != 64) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: float width %d (32 or 64)", k, x.arg);
            if (!xt_is_float(top[0])) LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: FCVT of an %s (I2F converts integers)", k, xt_name(top[0]));
            x.cls = top[0];
            push = x.arg == 32 ? LDB_XT_F32 : LDB_XT_F64;
            break;
      }
      depth -= pops;
      if (depth + 1 > XSTACK) LDB_FAIL(LDB_ERR_UNSUPPORTED, "map_expr: stack deeper than %d", XSTACK);
      ty[depth++] = push;
      has_float = has_float || xt_is_float(push) || x.op == LDB_X_F2I || x.op == LDB_X_FCMP;
   }
   if (depth != 1) LDB_FAIL(LDB_ERR_INVALID, "map_expr: the program leaves %d values (1 expected)", depth);
   if (xt_is_float(ty[0]) ? ty[0] != out_cls : xt_is_float(out_cls))
      LDB_FAIL(LDB_ERR_INVALID, "map_expr: instruction %d: the program's result is %s, out_type %d is not of that class", n_instr - 1, xt_name(ty[0]), out_type.type);
   const char* nm = name ? name : "expr";
   LdbTableHold res(ctx);
   LDB_TRY(ldb_gpu_table_alloc(ctx, "mapped", 1, &out_type, &nm, in->n_rows, nullptr, 0, &res.t));
   const int64_t n = in->n_rows;
   if (has_float) { // typed slots: the float kernel
      fp->out_width = res->cols[0].width;
      LDB_TRY(map_fexpr_launch(ctx, fp.get(), n, res.t));
      *out = res.release();
      return LDB_OK;
   }
   // integer program: the 128-bit integer interpreter, as it always was
   auto hp = std::make_unique<DXProg>();
   memset(hp.get(), 0, sizeof(DXProg));
   hp->n = n_instr;
   for (int32_t k = 0; k < n_instr; k++) {
      const DFInstr& x = fp->ins[k];
      hp->ins[k].op = x.op;
      hp->ins[k].arg = x.arg;
      hp->ins[k].col = x.col;
      hp->ins[k].lo = x.lo;
      hp->ins[k].hi = x.hi;
   }
   hp->out_width = res->cols[0].width;
   LdbBufs tmp(ctx);
   uint8_t* vb;
   LDB_TRY(tmp.alloc(&vb, (size_t) (n ? n : 1)));
   LDB_TRY(LdbBufs::alloc_into(ctx, &res->cols[0].validity, (size_t) ((n + 7) / 8 + 1)));
   uint8_t* bm = res->cols[0].validity;
   const int grid = ldb_grid_for(ctx, n, 256, 8);
   if (n) {
      LdbDesc<DXProg> d_desc(ctx);
      LDB_TRY(d_desc.upload(hp.get(), sizeof(DXProg)));
      DXProg* d = d_desc.p;
      {
         hipFunction_t spec = nullptr;
         if (ldb_jit_wanted(n)) {
            auto meta = std::make_unique<DXProg>();
            memcpy(meta.get(), hp.get(), sizeof(DXProg));
            for (int k = 0; k < LDB_MAX_XPROG; k++) ldb_jit_strip_col(meta->ins[k].col);
            std::string why;
            spec = ldb_jit_kernel(ctx->device, "ldb_expr_kernel.h", "DXProg", XPR_SPEC_SRC, "k_map_expr_spec", meta.get(), sizeof(DXProg), &why);
         }
         LdbProf prof_(ctx, "k_map_expr");
         if (spec) {
            uint64_t nn = (uint64_t) n;
            void* ov = res->cols[0].values;
            void* params[] = {(void*) &d, (void*) &nn, (void*) &ov, (void*) &vb};
            LDB_HIP(hipModuleLaunchKernel(spec, (unsigned) grid, 1, 1, 256, 1, 1, 0, ctx->stream, params, nullptr));
         } else {
            hipLaunchKernelGGL(k_map_expr, dim3(grid), dim3(256), 0, ctx->stream, (const DXProg*) d, (uint64_t) n, res->cols[0].values, vb);
         }
      }
      hipLaunchKernelGGL(k_pack_bytes_to_bits_x, dim3(grid), dim3(256), 0, ctx->stream, (const uint8_t*) vb, bm, (uint64_t) n);
      d_desc.release();
   }
   res->cols[0].null_count = -1; // unknown (Arrow convention)
   res->cols[0].type.nullable = 1;
   LDB_HIP(hipGetLastError());
   *out = res.release();
   return LDB_OK;
}

// ---------------------------------------------------------------- substr
// (d_substr_range: ldb_strfn.h, shared with the concatenation kernels)
__global__ void k_substr_lens(DCol col, int64_t from, int64_t for_len, uint64_t n, int64_t* __restrict__ lens, uint8_t* __restrict__ valid_bytes) {
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
      const uint32_t row = d_phys_row(col, i);
      const bool ok = d_valid(col, row);
      int64_t l = 0;
      if (ok) {
         uint32_t len, b0, b1;
         const uint8_t* s = d_load_str(col, row, &len);
         d_substr_range(s, len, from, for_len, &b0, &b1);
         l = (int64_t) (b1 - b0);
      }
      lens[i] = l;
      if (valid_bytes) valid_bytes[i] = ok ? 1 : 0;
   }
}
__global__ void k_substr_fill(DCol col, int64_t from, int64_t for_len, uint64_t n, const int64_t* __restrict__ offs, uint8_t* __restrict__ out) {
   for (uint64_t i = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
      const uint32_t row = d_phys_row(col, i);
      if (!d_valid(col, row)) continue;
      uint32_t len, b0, b1;
      const uint8_t* s = d_load_str(col, row, &len);
      d_substr_range(s, len, from, for_len, &b0, &b1);
      const int64_t o = offs[i];
      for (uint32_t b = b0; b < b1; b++) out[o + (b - b0)] = s[b];
   }
}

extern "C" int32_t ldb_gpu_map_substr(ldb_ctx* ctx, ldb_rel* in, ldb_colref col, int64_t from, int64_t for_len, const char* name, ldb_table** out) {
   if (!ctx || !in || !out) LDB_FAIL(LDB_ERR_INVALID, "map_substr: NULL argument");
   LDB_TRY(ldb_rel_force(ctx, in));
   DCol dc;
   LDB_TRY(ldb_make_dcol(in, col, &dc));
   if (dc.type != LDB_T_UTF8) LDB_FAIL(LDB_ERR_INVALID, "map_substr: utf8 column expected");
   const int64_t n = in->n_rows;
   const bool nullable = dc.validity || dc.rowids;
   const int grid = ldb_grid_for(ctx, n, 256, 8);
   LdbBufs tmp(ctx);
   int64_t* lens;
   uint8_t* vb = nullptr;
   LDB_TRY(tmp.alloc(&lens, 8 * (size_t) (n + 1)));
   if (nullable) LDB_TRY(tmp.alloc(&vb, (size_t) (n ? n : 1)));
   if (n) hipLaunchKernelGGL(k_substr_lens, dim3(grid), dim3(256), 0, ctx->stream, dc, from, for_len, (uint64_t) n, lens, vb);
   int64_t* offs;
   LDB_TRY(tmp.alloc(&offs, 8 * (size_t) (n + 1)));
   LDB_TRY(ldb_exclusive_scan_i64(ctx, lens, offs, n, offs + n));
   uint64_t total = 0;
   LDB_TRY(ldb_read_u64(ctx, offs + n, &total));
   tmp.free(lens);
   ldb_coltype t = {LDB_T_UTF8, 0, 0, nullable ? 1 : 0};
   const char* nm = name ? name : "substr";
   const int64_t cap = (int64_t) total;
   LdbTableHold res(ctx);
   LDB_TRY(ldb_gpu_table_alloc(ctx, "mapped", 1, &t, &nm, n, &cap, 0, &res.t));
   LDB_HIP(hipMemcpyAsync(res->cols[0].offsets, offs, 8 * (size_t) (n + 1), hipMemcpyDeviceToDevice, ctx->stream));
   res->cols[0].value_bytes = cap;
   if (n) hipLaunchKernelGGL(k_substr_fill, dim3(grid), dim3(256), 0, ctx->stream, dc, from, for_len, (uint64_t) n, (const int64_t*) offs, (uint8_t*) res->cols[0].values);
   tmp.free(offs);
   if (nullable) {
      LDB_TRY(LdbBufs::alloc_into(ctx, &res->cols[0].validity, (size_t) ((n + 7) / 8 + 1)));
      if (n) hipLaunchKernelGGL(k_pack_bytes_to_bits_x, dim3(grid), dim3(256), 0, ctx->stream, (const uint8_t*) vb, res->cols[0].validity, (uint64_t) n);
      res->cols[0].null_count = -1;
   }
   LDB_HIP(hipGetLastError());
   *out = res.release();
   return LDB_OK;
}
