// ldb_fexpr_kernel.h — device code of the scalar-expression interpreter for programs that compute with f32 / f64
// (ldb_gpu_map_expr with a float column, a float instruction or a float result): the postfix program of ldb_expr_kernel.h
// with typed stack slots.  A slot is an integer (nullable 128-bit, as on the integer path), an f32 or an f64; a float lives
// in the slot as its IEEE-754 bit pattern (low 32 / 64 bits), so SELECT / COALESCE / ISNULL and the final store move bits
// and never look at the class.  The host verifier has typed every slot and stamped the class of each instruction's
// operands into the program (`cls`): the kernel never tests a type at run time beyond the per-instruction switch, and the
// run-time specialised build folds the switch away.  Compiled ahead of time (generic) and by hiprtc (program as a
// compile-time constant) from this one source.
// Reference: BinOpLowering<db::AddOp.., FloatType, arith::AddF..> (src/compiler/Conversion/DBToStd/LowerToStd.cpp:1593-1596),
// CmpOpLowering::translateFPredicate (:870-895, the ORDERED predicates: any NaN operand → false, `neq` = ONE),
// CastOpLowering (:947-1018: sitofp / fptosi / extf / truncf).
#pragma once
#include "ldb_device.h"

#define FXSTACK 8
// class of a stack slot (host verifier: ldb_gpu_map_expr)
#define LDB_XT_INT 0
#define LDB_XT_F32 1
#define LDB_XT_F64 2
#define LDB_XT_BOOL 3 // an integer slot holding 0 / 1

struct DFInstr {
   int32_t op;
   int32_t arg;
   int32_t cls; // class of the operands (FADD.. FCMP, F2I, FCVT) or of the pushed slot (COL)
   int32_t pad;
   DCol col;
   uint64_t lo; // CONST: low word; FCONST: the bit pattern of the constant AT THE SLOT'S WIDTH (the host has rounded f64 → f32)
   int64_t hi;
};
struct DFProg {
   int32_t n;
   int32_t out_width; // 1, 4, 8 or 16 bytes per output value (a float result: 4 / 8, its bit pattern)
   DFInstr ins[LDB_MAX_XPROG];
};

#define FX_ROWS 2 // rows in flight per lane (the loads of one iteration's rows are independent and issue back to back)

__device__ __forceinline__ float fx_f32(i128 s) { return __uint_as_float((uint32_t) s); }
__device__ __forceinline__ double fx_f64(i128 s) { return __longlong_as_double((long long) (uint64_t) s); }
__device__ __forceinline__ i128 fx_slot(float v) { return (i128) (u128) __float_as_uint(v); }
__device__ __forceinline__ i128 fx_slot(double v) { return (i128) (u128) (uint64_t) __double_as_longlong(v); }

// ordered comparison (arith.cmpf oeq / one / olt / ole / ogt / oge): false when an operand is NaN
template <typename T>
__device__ __forceinline__ bool fx_cmp(int op, T a, T b) {
   switch (op) {
      case LDB_F_EQ: return a == b;
      case LDB_F_NEQ: return a < b || a > b;
      case LDB_F_LT: return a < b;
      case LDB_F_LTE: return a <= b;
      case LDB_F_GT: return a > b;
      default: return a >= b;
   }
}
// sitofp of a 128-bit integer with ONE rounding (to nearest even): |v| is reduced to 64 bits with the lost bits OR-ed into
// bit 0 (64 significant bits are far more than a mantissa + guard bit, so the sticky bit decides ties exactly as the lost
// bits would), converted — the 64-bit conversion rounds once — and scaled by the exact power of two.  |v| <= 2^127 stays
// below the largest f32 (2^128 - 2^104).
template <typename T>
__device__ __forceinline__ T fx_i2f(i128 v) {
#pragma clang fp contract(off)
   const bool neg = v < 0;
   const u128 m = neg ? (u128) 0 - (u128) v : (u128) v;
   const uint64_t hi = (uint64_t) (m >> 64);
   T r;
   if (hi == 0) {
      r = (T) (uint64_t) m;
   } else {
      const int sh = 64 - __builtin_clzll(hi); // 1 … 64
      const uint64_t lost = sh == 64 ? (uint64_t) m : ((uint64_t) m & ((1ull << sh) - 1ull));
      const uint64_t top = (uint64_t) (m >> sh) | (lost ? 1ull : 0ull);
      T scale;
      if (sizeof(T) == 4) scale = (T) __uint_as_float((uint32_t) (127 + sh) << 23);
      else scale = (T) __longlong_as_double((long long) ((uint64_t) (1023 + sh) << 52));
      r = (T) top * scale;
   }
   return neg ? -r : r;
}
// fptosi to i64; false (→ NULL) for NaN and values outside [-2^63, 2^63), which the reference leaves undefined
template <typename T>
__device__ __forceinline__ bool fx_f2i(T v, int64_t* out) {
   const bool ok = v >= (T) -9223372036854775808.0 && v < (T) 9223372036854775808.0;
   *out = ok ? (int64_t) v : 0;
   return ok;
}

// one row: the program's value (bit pattern for a float result) into *val, returns "is NULL".  `in` = the row exists
// (lanes behind the last row run along so that the whole wave reaches the ballot; they load nothing)
__device__ __forceinline__ bool fexpr_row(const DFProg& m, const DFProg* __restrict__ d, uint64_t i, bool in, i128* val) {
// arith.mulf + arith.addf stay two roundings: no fused multiply-add (the compiler contracts a*b+c by default)
#pragma clang fp contract(off)
   i128 st[FXSTACK];
   bool nul[FXSTACK];
   int sp = 0;
   const int np = m.n;
   LDB_UNROLL
   for (int k = 0; k < LDB_MAX_XPROG; k++) {
      if (k >= np) break;
      const DFInstr& x = m.ins[k];
      switch (x.op) {
         case LDB_X_COL: {
            const CV col(x.col, d->ins[k].col);
            bool ok = false;
            i128 v = 0;
            if (in) {
               const uint32_t row = d_phys_row(col, i);
               ok = d_valid(col, row);
               if (ok) {
                  if (x.cls == LDB_XT_F32) v = (i128) (u128) gptr<uint32_t>(col.p.values)[row];
                  else if (x.cls == LDB_XT_F64) v = (i128) (u128) gptr<uint64_t>(col.p.values)[row];
                  else v = d_load_i128(col, row);
               }
            }
            st[sp] = v;
            nul[sp] = !ok;
            sp++;
            break;
         }
         case LDB_X_CONST:
            st[sp] = (i128) (((u128) (uint64_t) x.hi << 64) | x.lo);
            nul[sp] = false;
            sp++;
            break;
         case LDB_X_FCONST:
            st[sp] = (i128) (u128) x.lo;
            nul[sp] = false;
            sp++;
            break;
         case LDB_X_ROW:
            st[sp] = (i128) i;
            nul[sp] = false;
            sp++;
            break;
         case LDB_X_ADD:
         case LDB_X_SUB:
         case LDB_X_MUL:
         case LDB_X_SDIV: {
            const i128 b = st[--sp], a = st[sp - 1];
            const bool nb = nul[sp];
            bool nn = nul[sp - 1] || nb;
            i128 r = 0;
            if (!nn) {
               if (x.op == LDB_X_ADD) r = (i128) ((u128) a + (u128) b);
               else if (x.op == LDB_X_SUB) r = (i128) ((u128) a - (u128) b);
               else if (x.op == LDB_X_MUL) r = (i128) ((u128) a * (u128) b);
               else if (b == 0) nn = true; // arith.divsi by zero is undefined in the reference: NULL here
               else r = d_sdiv128(a, b);
            }
            st[sp - 1] = r;
            nul[sp - 1] = nn;
            break;
         }
         case LDB_X_FADD:
         case LDB_X_FSUB:
         case LDB_X_FMUL:
         case LDB_X_FDIV: { // IEEE: x / 0 is ±inf or NaN, not NULL
            const i128 b = st[--sp], a = st[sp - 1];
            nul[sp - 1] = nul[sp - 1] || nul[sp];
            if (x.cls == LDB_XT_F32) {
               const float fa = fx_f32(a), fb = fx_f32(b);
               st[sp - 1] = fx_slot(x.op == LDB_X_FADD ? fa + fb : x.op == LDB_X_FSUB ? fa - fb : x.op == LDB_X_FMUL ? fa * fb : fa / fb);
            } else {
               const double fa = fx_f64(a), fb = fx_f64(b);
               st[sp - 1] = fx_slot(x.op == LDB_X_FADD ? fa + fb : x.op == LDB_X_FSUB ? fa - fb : x.op == LDB_X_FMUL ? fa * fb : fa / fb);
            }
            break;
         }
         case LDB_X_FCMP: {
            const i128 b = st[--sp], a = st[sp - 1];
            nul[sp - 1] = nul[sp - 1] || nul[sp];
            st[sp - 1] = (x.cls == LDB_XT_F32 ? fx_cmp<float>(x.arg, fx_f32(a), fx_f32(b)) : fx_cmp<double>(x.arg, fx_f64(a), fx_f64(b))) ? 1 : 0;
            break;
         }
         case LDB_X_I2F: st[sp - 1] = x.arg == 32 ? fx_slot(fx_i2f<float>(st[sp - 1])) : fx_slot(fx_i2f<double>(st[sp - 1])); break;
         case LDB_X_F2I: {
            int64_t r;
            const bool ok = x.cls == LDB_XT_F32 ? fx_f2i<float>(fx_f32(st[sp - 1]), &r) : fx_f2i<double>(fx_f64(st[sp - 1]), &r);
            st[sp - 1] = (i128) r;
            nul[sp - 1] = nul[sp - 1] || !ok;
            break;
         }
         case LDB_X_FCVT:
            if (x.cls == LDB_XT_F32 && x.arg == 64) st[sp - 1] = fx_slot((double) fx_f32(st[sp - 1])); // arith.extf (exact)
            else if (x.cls == LDB_XT_F64 && x.arg == 32) st[sp - 1] = fx_slot((float) fx_f64(st[sp - 1])); // arith.truncf (nearest even)
            break;
         case LDB_X_MUL_POW10: st[sp - 1] = (i128) ((u128) st[sp - 1] * (u128) d_pow10(x.arg)); break;
         case LDB_X_SDIV_POW10: st[sp - 1] = d_sdiv128(st[sp - 1], d_pow10(x.arg)); break;
         case LDB_X_NEG: st[sp - 1] = (i128) ((u128) 0 - (u128) st[sp - 1]); break;
         case LDB_X_CMP: {
            const i128 b = st[--sp], a = st[sp - 1];
            nul[sp - 1] = nul[sp - 1] || nul[sp];
            st[sp - 1] = d_cmp_vals<i128>(x.arg, a, b) ? 1 : 0;
            break;
         }
         case LDB_X_AND: { // three-valued: false wins over NULL
            const i128 b = st[--sp], a = st[sp - 1];
            const bool na = nul[sp - 1], nb = nul[sp];
            const bool fa = !na && a == 0, fb = !nb && b == 0;
            nul[sp - 1] = !(fa || fb) && (na || nb);
            st[sp - 1] = (fa || fb || na || nb) ? 0 : 1;
            break;
         }
         case LDB_X_OR: { // three-valued: true wins over NULL
            const i128 b = st[--sp], a = st[sp - 1];
            const bool na = nul[sp - 1], nb = nul[sp];
            const bool ta = !na && a != 0, tb = !nb && b != 0;
            nul[sp - 1] = !(ta || tb) && (na || nb);
            st[sp - 1] = (ta || tb) ? 1 : 0;
            break;
         }
         case LDB_X_NOT: st[sp - 1] = st[sp - 1] == 0 ? 1 : 0; break;
         case LDB_X_SELECT: { // cond a b → cond (true and not NULL, db.derive_truth) ? a : b
            const i128 b = st[--sp], a = st[--sp];
            const bool nb = nul[sp + 1], na = nul[sp];
            const bool c = !nul[sp - 1] && st[sp - 1] != 0;
            st[sp - 1] = c ? a : b;
            nul[sp - 1] = c ? na : nb;
            break;
         }
         case LDB_X_ISNULL:
            st[sp - 1] = nul[sp - 1] ? 1 : 0;
            nul[sp - 1] = false;
            break;
         default: { // LDB_X_COALESCE: a b → a unless NULL
            const i128 b = st[--sp];
            const bool nb = nul[sp];
            if (nul[sp - 1]) {
               st[sp - 1] = b;
               nul[sp - 1] = nb;
            }
            break;
         }
      }
   }
   *val = nul[0] ? (i128) 0 : st[0];
   return nul[0];
}

// Thread t of the grid takes rows t, t + T, t + 2T … (T = threads of the grid, a multiple of 64): the 64 lanes of a wave
// hold 64 consecutive rows starting at a multiple of 64, i.e. exactly one 64-bit word of the Arrow validity bitmap, which
// the wave writes with one ballot — no byte array, no pack pass.  The loop runs on the wave's first row, so every lane of
// the last, partial wave reaches the ballot; `valid_words` holds ceil(n / 64) words.
__device__ __forceinline__ void map_fexpr_body(const DFProg& m, const DFProg* __restrict__ d, uint64_t n, void* __restrict__ out, uint64_t* __restrict__ valid_words) {
   const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
   const uint64_t first = blockIdx.x * (uint64_t) blockDim.x + threadIdx.x;
   const uint32_t lane = d_lane_id();
   for (uint64_t i0 = first; i0 - lane < n; i0 += FX_ROWS * stride) {
      i128 v[FX_ROWS];
      bool nul[FX_ROWS];
#pragma unroll
      for (int u = 0; u < FX_ROWS; u++) {
         const uint64_t i = i0 + (uint64_t) u * stride;
         nul[u] = fexpr_row(m, d, i, i < n, &v[u]);
      }
#pragma unroll
      for (int u = 0; u < FX_ROWS; u++) {
         const uint64_t i = i0 + (uint64_t) u * stride;
         const bool in = i < n;
         if (in) {
            switch (m.out_width) {
               case 1: ((uint8_t*) out)[i] = v[u] != 0 ? 1 : 0; break;
               case 4: ((uint32_t*) out)[i] = (uint32_t) v[u]; break;
               case 8: ((uint64_t*) out)[i] = (uint64_t) v[u]; break;
               default: ((i128*) out)[i] = v[u]; break;
            }
         }
         const uint64_t word = __ballot(in && !nul[u]);
         if (lane == 0 && i < n) valid_words[i >> 6] = word; // (lane 0 holds the wave's first row)
      }
   }
}
