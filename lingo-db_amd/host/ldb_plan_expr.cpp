// ldb_plan_expr.cpp — the plan interpreter's predicates and expressions: filter descriptors typed against their columns, scalar
// subquery read-back, IN lists as semi joins, expression trees compiled to postfix programs, the aggregate normal form.
#include "ldb_plan_interp.hpp"
#include <cctype>
#include <cmath>
#include <cstring>

namespace ldbplan {

// ------------------------------------------------------------ predicates
int32_t Interp::opOf(const std::string& op) {
   static const std::map<std::string, int32_t> ops = {{"EQ", LDB_F_EQ},   {"NEQ", LDB_F_NEQ}, {"LT", LDB_F_LT}, {"LTE", LDB_F_LTE},   {"GT", LDB_F_GT},
                                                      {"GTE", LDB_F_GTE}, {"NOTNULL", LDB_F_NOTNULL}, {"IN", LDB_F_IN}, {"LIKE", LDB_F_LIKE}, {"NOT LIKE", LDB_F_NOT_LIKE}};
   auto it = ops.find(op);
   if (it == ops.end()) throw std::runtime_error("plan: unknown comparison '" + op + "'");
   return it->second;
}
// value of row 0 of a 1-row table's column as a 128-bit integer (scalar subquery results)
__int128 Interp::readScalar(const std::string& table, const std::string& col) {
   Value& v = val(table);
   if (v.kind != Value::TABLE) throw std::runtime_error("plan: scalar source '" + table + "' must be a table");
   if (ldb_gpu_table_rows(v.table) < 1) throw std::runtime_error("plan: scalar source '" + table + "' is empty");
   const int32_t c = ldb_gpu_table_col_index(v.table, col.c_str());
   if (c < 0) throw std::runtime_error("plan: scalar source has no column '" + col + "'");
   const int32_t w = ldb_gpu_table_col_width(v.table, c);
   const int64_t rows = ldb_gpu_table_rows(v.table);
   std::vector<uint8_t> buf((size_t) (rows * w));
   check(ldb_gpu_table_read_fixed(ctx, v.table, c, buf.data(), (int64_t) buf.size()), "scalar read");
   __int128 x = 0;
   if (w == 16) memcpy(&x, buf.data(), 16);
   else if (w == 8) {
      int64_t t;
      memcpy(&t, buf.data(), 8);
      x = t;
   } else if (w == 4) {
      int32_t t;
      memcpy(&t, buf.data(), 4);
      x = t;
   } else if (w == 2) {
      int16_t t;
      memcpy(&t, buf.data(), 2);
      x = t;
   } else if (w == 1) { // int8 / bool
      x = (int8_t) buf[0];
   } else {
      throw std::runtime_error("plan: scalar source column of width " + std::to_string(w));
   }
   return x;
}
// row 0 of the scalar source is NULL (SimpleState over an empty input yields one NULL row)
bool Interp::scalarIsNull(const std::string& table, const std::string& col) {
   Value& v = val(table);
   if (v.kind != Value::TABLE) throw std::runtime_error("plan: scalar source '" + table + "' must be a table");
   const int32_t c = ldb_gpu_table_col_index(v.table, col.c_str());
   if (c < 0) throw std::runtime_error("plan: scalar source has no column '" + col + "'");
   int32_t valid = 1;
   check(ldb_gpu_table_row_valid(ctx, v.table, c, 0, &valid), "scalar validity");
   return valid == 0;
}
static __int128 floorDiv(__int128 a, __int128 b) {
   __int128 q = a / b;
   if ((a % b != 0) && ((a < 0) != (b < 0))) q--;
   return q;
}
ldb_filter_desc Interp::pred(const std::vector<const ldb_table*>& sides, const J& jp) {
   const std::string& opName = jp.s("op");
   const int32_t op = opOf(opName);
   const ldb_colref c = resolve(sides, jp.s("col"), "filter");
   const ldb_table* tab = sides[(size_t) c.side];
   const std::string colName = ldb_gpu_table_col_name(tab, c.col);
   if (const J* rc = jp.get("rhs_col")) { // residual column-vs-column conjunct (generated db.compare in the reference)
      ldb_filter_desc d;
      memset(&d, 0, sizeof(d));
      d.col = c;
      d.op = op;
      d.rhs_kind = LDB_RHS_COLUMN;
      d.rhs_col = resolve(sides, rc->str, "filter rhs");
      return d;
   }
   if (op == LDB_F_LIKE || op == LDB_F_NOT_LIKE) { // StringRuntime::like, evaluated in generated code
      keepStr.push_back(std::make_unique<std::string>(jp.s("value")));
      ldb_filter_desc d;
      memset(&d, 0, sizeof(d));
      d.col = c;
      d.op = op;
      d.rhs_kind = LDB_RHS_STRING;
      d.str = keepStr.back()->data();
      d.str_len = (int32_t) keepStr.back()->size();
      return d;
   }
   if (const J* sc = jp.get("scalar")) { // column OP (scalar subquery result): the constant is read back from the device
      if (rowsOf(sc->s("from")) < 1 || scalarIsNull(sc->s("from"), sc->s("col"))) { // no row, or a NULL (a key-less aggregate over no rows): a comparison with NULL keeps nothing
         ldb_filter_desc d;
         memset(&d, 0, sizeof(d));
         d.col = c;
         d.op = LDB_F_LT;
         d.rhs_kind = LDB_RHS_COLUMN;
         d.rhs_col = c;
         return d;
      }
      __int128 x = readScalar(sc->s("from"), sc->s("col"));
      // the two sides of the comparison are cast to a common decimal type first; with
      // x at scale sx and the column at scale sc <= sx:  col * 10^k OP x  ⇔  col OP' floor-ish(x / 10^k)
      const int64_t k = sc->iOr("div_pow10", 0);
      if (k < 0 || k > 38) throw std::runtime_error("plan: div_pow10 must be in [0, 38]");
      if (k > 0) {
         __int128 m = 1;
         for (int64_t i = 0; i < k; i++) m *= 10;
         const __int128 fl = floorDiv(x, m);
         const bool exact = fl * m == x;
         // col*m > x ⇔ col > floor(x/m);  col*m >= x ⇔ col > floor(x/m) unless exact;  col*m < x ⇔ col <= floor unless exact …
         ldb_filter_desc d;
         memset(&d, 0, sizeof(d));
         d.col = c;
         d.rhs_kind = LDB_RHS_INT;
         int32_t o = op;
         __int128 v = fl;
         switch (op) {
            case LDB_F_GT: o = LDB_F_GT; break;
            case LDB_F_GTE: o = exact ? LDB_F_GTE : LDB_F_GT; break;
            case LDB_F_LT: o = exact ? LDB_F_LT : LDB_F_LTE; break;
            case LDB_F_LTE: o = LDB_F_LTE; break;
            case LDB_F_EQ:
               if (!exact) { // never true: compare with an impossible pair
                  o = LDB_F_LT;
                  v = ((__int128) 1) << 126;
                  v = -v;
               }
               break;
            default: throw std::runtime_error("plan: scalar comparison operator not supported");
         }
         d.op = o;
         d.value_lo = (uint64_t) v;
         d.value_hi = (int64_t) (v >> 64);
         return d;
      }
      ldb_filter_desc d;
      memset(&d, 0, sizeof(d));
      d.col = c;
      d.op = op;
      d.rhs_kind = LDB_RHS_INT;
      d.value_lo = (uint64_t) x;
      d.value_hi = (int64_t) (x >> 64);
      return d;
   }
   // column vs constant: typed by the mirror of Restrictions::create (Restrictions.cpp:392-521)
   FilterDescription fd;
   fd.columnName = colName;
   fd.op = (FilterOp) op;
   if (op == LDB_F_IN) {
      const J& vals = jp.at("values");
      if (vals.kind != J::ARR || vals.arr.empty()) throw std::runtime_error("plan: IN needs a non-empty 'values' array");
      if (vals.arr[0].kind == J::STR) {
         std::vector<std::string> v;
         for (auto& e : vals.arr) v.push_back(e.str);
         fd.values = v;
      } else {
         std::vector<int64_t> v;
         for (auto& e : vals.arr) v.push_back(e.inum);
         fd.values = v;
      }
   } else if (op != LDB_F_NOTNULL) {
      const J& v = jp.at("value");
      if (v.kind == J::STR) fd.value = v.str;
      else if (v.kind == J::NUM && v.isInt) fd.value = v.inum;
      else if (v.kind == J::NUM) fd.value = v.num;
      else throw std::runtime_error("plan: filter constant must be a string or a number");
   }
   keepRestr.push_back(Restrictions::create({fd}, tab, c.side));
   return keepRestr.back()->data()[0];
}
// rows of `cur` whose column d.col is one of d's constants: cur ⋉ (table of the constants).  The table, its relation and the hash table live as hidden
// values until the plan run ends
ldb_rel* Interp::semiJoinConstants(ldb_rel* cur, const ldb_filter_desc& d, const std::vector<const ldb_table*>& sides, const std::string& stem) {
   ldb_coltype ct;
   check(ldb_gpu_table_coltype(sides[(size_t) d.col.side], d.col.col, &ct), "IN list (column type)");
   const size_t w = ct.type == LDB_T_INT32 || ct.type == LDB_T_DATE32 || ct.type == LDB_T_CHAR4 ? 4 : ct.type == LDB_T_INT64 ? 8 : 0;
   if (!w)
      throw std::runtime_error("filter: an IN list of more than " + std::to_string(kMaxInConstants) +
                               " numeric constants over a column that is not a 4- or 8-byte integer / date / char(1) (string lists of any size go to the scan itself)");
   std::vector<uint8_t> buf(w * (size_t) d.n_in);
   for (int32_t k = 0; k < d.n_in; k++) memcpy(buf.data() + w * (size_t) k, &d.in_values[2 * k], w); // (little-endian low word of the 128-bit constant)
   ct.nullable = 0;
   const char* colName = "in_value";
   const std::string tag = "$in_list:" + stem + ":" + std::to_string(env.size());
   OwnedTable ot(ctx);
   check(ldb_gpu_table_alloc(ctx, "in_list", 1, &ct, &colName, d.n_in, nullptr, 0, ot.out()), "IN list (table)");
   ldb_table* t = ot.get();
   putTable(tag, ot);
   check(ldb_gpu_table_write_fixed(ctx, t, 0, buf.data(), (int64_t) buf.size()), "IN list (constants)");
   OwnedRel obr(ctx);
   check(ldb_gpu_rel_from_table(ctx, t, obr.out()), "IN list (relation)");
   ldb_rel* br = obr.get();
   putRel(tag + ":rel", obr, {t});
   const ldb_colref key{0, 0};
   OwnedHt oht(ctx);
   check(ldb_gpu_join_build(ctx, br, &key, 1, 0, oht.out()), "IN list (hash table)");
   ldb_hashtable* ht = oht.get();
   putHt(tag + ":ht", oht, {t});
   ldb_rel* out = nullptr;
   check(ldb_gpu_join_probe(ctx, ht, cur, &d.col, 1, LDB_JOIN_SEMI, &out, nullptr), "IN list (semi join)");
   return out;
}
std::vector<ldb_filter_desc> Interp::preds(const std::vector<const ldb_table*>& sides, const J* list) {
   std::vector<ldb_filter_desc> out;
   if (!list) return out;
   for (auto& jp : list->arr) out.push_back(pred(sides, jp));
   return out;
}

// ------------------------------------------------------------ expressions
static Scalar scalarOfCol(const ldb_coltype& t) {
   Scalar s;
   switch (t.type) {
      case LDB_T_DECIMAL128: s.kind = Scalar::DEC; s.p = t.precision; s.s = t.scale; break;
      case LDB_T_DATE32: s.kind = Scalar::DATE; break;
      case LDB_T_BOOL8: s.kind = Scalar::BOOL; break;
      case LDB_T_INT8:
      case LDB_T_INT16:
      case LDB_T_INT32:
      case LDB_T_INT64:
      case LDB_T_CHAR4: s.kind = Scalar::INT; break;
      case LDB_T_FLOAT32: s.kind = Scalar::F32; break;
      case LDB_T_FLOAT64: s.kind = Scalar::F64; break;
      default: throw std::runtime_error("plan: expression over a non-numeric column");
   }
   return s;
}
static DecimalType asDec(const Scalar& s) { return s.kind == Scalar::DEC ? DecimalType{s.p, s.s} : DecimalType{19, 0}; } // int → decimal(19,0), sql_analyzer.cpp:3125-3141
static Scalar decScalar(DecimalType t) {
   Scalar s;
   s.kind = Scalar::DEC;
   s.p = t.p;
   s.s = t.s;
   return s;
}
// decimal literal "0.2" → decimal(2,1) value 2 (sql_analyzer.cpp:2103-2113: p = digits, s = digits after the point)
bool Interp::decimalLiteral(const std::string& txt, __int128* v, Scalar* t) {
   const auto dot = txt.find('.');
   if (dot == std::string::npos) return false;
   for (size_t i = 0; i < txt.size(); i++)
      if (!(isdigit((unsigned char) txt[i]) || txt[i] == '.' || (i == 0 && txt[i] == '-'))) return false;
   const int32_t s = (int32_t) (txt.size() - dot - 1);
   const bool neg = txt[0] == '-';
   const int32_t p = (int32_t) txt.size() - 1 - (neg ? 1 : 0);
   *v = parseDecimal(txt, s);
   *t = decScalar({p, s});
   return true;
}

static void castTo(XB& b, const Scalar& from, const DecimalType& to) { // db.cast to a decimal of larger-or-equal scale
   const int32_t fs = from.kind == Scalar::DEC ? from.s : 0;
   if (to.s > fs) b.push(LDB_X_MUL_POW10, to.s - fs);
   else if (to.s < fs) b.push(LDB_X_SDIV_POW10, fs - to.s);
}
// ---- floats (the plan is post-frontend: the reference has inserted db.cast, so both sides of an operator have ONE type)
static Scalar floatScalar(int bits) {
   Scalar s;
   s.kind = bits == 32 ? Scalar::F32 : Scalar::F64;
   return s;
}
static int32_t floatBits(const Scalar& s) { return s.kind == Scalar::F32 ? 32 : 64; }
static const char* scalarName(const Scalar& s) {
   switch (s.kind) {
      case Scalar::F32: return "f32";
      case Scalar::F64: return "f64";
      case Scalar::DEC: return "decimal";
      case Scalar::DATE: return "date";
      case Scalar::BOOL: return "bool";
      default: return "integer";
   }
}
// true: a float operator (both sides floats of one width); false: no float involved; anything else needs a cast
static bool floatPair(const std::string& op, const Scalar& l, const Scalar& r) {
   if (!l.isFloat() && !r.isFloat()) return false;
   if (l.kind != r.kind)
      throw std::runtime_error("plan: '" + op + "' over " + scalarName(l) + " and " + scalarName(r) + ": floats do not mix with other types or widths, add an explicit cast ({\"cast\": [\"" +
                               (l.isFloat() ? scalarName(l) : scalarName(r)) + "\", …]})");
   return true;
}
static void pushFConst(XB& b, double v, int32_t bits) {
   int64_t raw;
   memcpy(&raw, &v, 8);
   b.push(LDB_X_FCONST, bits, {0, 0}, (__int128) (uint64_t) raw);
}
// CastOpLowering's decimal scale factor: single-precision powf widened to the target type (LowerToStd.cpp:947-1018)
static double castPow10(int32_t s) { return (double) powf(10.0f, (float) s); }
static Scalar parseCastType(const std::string& t) {
   if (t == "f32") return floatScalar(32);
   if (t == "f64") return floatScalar(64);
   if (t == "i64") return Scalar{};
   int p = 0, sc = 0;
   char tail = 0;
   if (sscanf(t.c_str(), "decimal(%d,%d%c", &p, &sc, &tail) == 3 && tail == ')' && p >= 1 && p <= 38 && sc >= 0 && sc <= p) return decScalar({p, sc});
   throw std::runtime_error("plan: cast target '" + t + "' (f32, f64, i64 or decimal(p,s) expected)");
}
// compile an expression tree into postfix code; returns its type
Scalar Interp::compileX(const std::vector<const ldb_table*>& sides, const J& e, XB& b) {
   if (e.kind == J::NUM) {
      if (!e.isInt) throw std::runtime_error("plan: write decimal literals as strings (\"0.2\")");
      b.push(LDB_X_CONST, 0, {0, 0}, (__int128) e.inum);
      return Scalar{};
   }
   if (e.kind == J::STR) {
      __int128 v;
      Scalar t;
      if (decimalLiteral(e.str, &v, &t)) {
         b.push(LDB_X_CONST, 0, {0, 0}, v);
         return t;
      }
      const ldb_colref c = resolve(sides, e.str, "expression");
      b.push(LDB_X_COL, 0, c);
      return scalarOfCol(typeOf(sides, c));
   }
   if (e.kind != J::OBJ || e.obj.size() != 1) throw std::runtime_error("plan: expression node must be {\"op\": [args]}");
   const std::string& op = e.obj[0].first;
   const J& args = e.obj[0].second;
   auto arity = [&](size_t n) {
      if (args.kind != J::ARR || args.arr.size() != n) throw std::runtime_error("plan: '" + op + "' takes " + std::to_string(n) + " arguments");
   };
   if (op == "datediff") { // DateRuntime::dateDiffDay / Hour / Minute / Second (DateRuntime.cpp:83-98): (end - start) ns sdiv 10^9, then sdiv 60 / 3600 / 86400
      arity(3);
      if (args.arr[0].kind != J::STR) throw std::runtime_error("plan: 'datediff' takes [unit, end, start] with the unit as a string");
      const int32_t unit = datepartOf(args.arr[0].str);
      if (unit < LDB_DP_DAY) throw std::runtime_error("plan: 'datediff' unit '" + args.arr[0].str + "' (day, hour, minute, second)");
      const int64_t perDay = unit == LDB_DP_DAY ? 1 : unit == LDB_DP_HOUR ? 24 : unit == LDB_DP_MINUTE ? 1440 : 86400;
      const Scalar l = compileX(sides, args.arr[1], b), r = compileX(sides, args.arr[2], b);
      if (l.kind != r.kind || (l.kind != Scalar::DATE && l.kind != Scalar::INT))
         throw std::runtime_error(std::string("plan: 'datediff' over ") + scalarName(l) + " and " + scalarName(r) + ": two date32 values or two int64 ns values expected");
      b.push(LDB_X_SUB);
      if (l.kind == Scalar::DATE) { // whole days, multiplied out to the unit
         if (perDay != 1) {
            b.push(LDB_X_CONST, 0, {0, 0}, (__int128) perDay);
            b.push(LDB_X_MUL);
         }
         return Scalar{};
      }
      b.push(LDB_X_CONST, 0, {0, 0}, (__int128) 1000000000);
      b.push(LDB_X_SDIV); // truncating, as the reference's `/`
      if (unit != LDB_DP_SECOND) {
         b.push(LDB_X_CONST, 0, {0, 0}, (__int128) (86400 / perDay));
         b.push(LDB_X_SDIV);
      }
      return Scalar{};
   }
   if (op == "add" || op == "sub") {
      arity(2);
      XB lb, rb;
      const Scalar l = compileX(sides, args.arr[0], lb), r = compileX(sides, args.arr[1], rb);
      if (floatPair(op, l, r)) { // arith.addf / subf
         b.ins.insert(b.ins.end(), lb.ins.begin(), lb.ins.end());
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
         b.push(op == "add" ? LDB_X_FADD : LDB_X_FSUB);
         return l;
      }
      if (l.kind == Scalar::INT && r.kind == Scalar::INT) {
         b.ins.insert(b.ins.end(), lb.ins.begin(), lb.ins.end());
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
         b.push(op == "add" ? LDB_X_ADD : LDB_X_SUB);
         return Scalar{};
      }
      const DecimalType t = higherDecimalType(asDec(l), asDec(r)); // DecimalBinOpLowering after the frontend's casts (LowerToStd.cpp:680-699)
      b.ins.insert(b.ins.end(), lb.ins.begin(), lb.ins.end());
      castTo(b, l, t);
      b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
      castTo(b, r, t);
      b.push(op == "add" ? LDB_X_ADD : LDB_X_SUB);
      return decScalar(t);
   }
   if (op == "mul") {
      arity(2);
      const Scalar l = compileX(sides, args.arr[0], b);
      const Scalar r = compileX(sides, args.arr[1], b);
      if (floatPair(op, l, r)) { // arith.mulf
         b.push(LDB_X_FMUL);
         return l;
      }
      b.push(LDB_X_MUL);
      if (l.kind == Scalar::INT && r.kind == Scalar::INT) return Scalar{};
      const DecimalType dl = asDec(l), dr = asDec(r), t = typeAfterMul(dl, dr); // DecimalMulOpLowering (LowerToStd.cpp:653-677)
      if (dl.s + dr.s > t.s) b.push(LDB_X_SDIV_POW10, dl.s + dr.s - t.s);
      return decScalar(t);
   }
   if (op == "div") {
      arity(2);
      const Scalar l = compileX(sides, args.arr[0], b);
      XB rb;
      const Scalar r = compileX(sides, args.arr[1], rb);
      if (floatPair(op, l, r)) { // arith.divf: IEEE, x / 0 = ±inf / NaN
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
         b.push(LDB_X_FDIV);
         return l;
      }
      const DecimalType dl = asDec(l), dr = asDec(r), t = typeAfterDiv(dl, dr); // DecimalOpScaledLowering (LowerToStd.cpp:631-651)
      const int32_t k = t.s + dr.s - dl.s;
      if (k < 0) throw std::runtime_error("plan: decimal division with a negative scale adjustment");
      b.push(LDB_X_MUL_POW10, k);
      b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
      b.push(LDB_X_SDIV);
      return decScalar(t);
   }
   if (op == "idiv") { // integer division of two integers (arith.divsi: truncating) — the result stays an integer
      arity(2);
      const Scalar l = compileX(sides, args.arr[0], b);
      const Scalar r = compileX(sides, args.arr[1], b);
      if (l.kind != Scalar::INT || r.kind != Scalar::INT) throw std::runtime_error("plan: idiv takes two integers (decimals and floats divide with 'div')");
      b.push(LDB_X_SDIV);
      return Scalar{};
   }
   if (op == "row_number") { // the logical row number of the input relation, 0 … n-1 (a tuple's identity inside nested_map)
      arity(0);
      b.push(LDB_X_ROW);
      return Scalar{};
   }
   if (op == "cmp") { // ["GT", a, b]
      arity(3);
      const int32_t cmp = opOf(args.arr[0].str);
      if (cmp > LDB_F_GTE) throw std::runtime_error("plan: cmp needs EQ/NEQ/LT/LTE/GT/GTE");
      XB lb, rb;
      const Scalar l = compileX(sides, args.arr[1], lb), r = compileX(sides, args.arr[2], rb);
      b.ins.insert(b.ins.end(), lb.ins.begin(), lb.ins.end());
      const bool flt = floatPair(op, l, r); // arith.cmpf, ordered predicates
      if (!flt && (l.kind == Scalar::DEC || r.kind == Scalar::DEC)) {
         const DecimalType t = higherDecimalType(asDec(l), asDec(r));
         castTo(b, l, t);
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
         castTo(b, r, t);
      } else {
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
      }
      b.push(flt ? LDB_X_FCMP : LDB_X_CMP, cmp);
      Scalar s;
      s.kind = Scalar::BOOL;
      return s;
   }
   if (op == "and" || op == "or") {
      arity(2);
      compileX(sides, args.arr[0], b);
      compileX(sides, args.arr[1], b);
      b.push(op == "and" ? LDB_X_AND : LDB_X_OR);
      Scalar s;
      s.kind = Scalar::BOOL;
      return s;
   }
   if (op == "not" || op == "isnull") {
      arity(1);
      compileX(sides, args.arr[0], b);
      b.push(op == "not" ? LDB_X_NOT : LDB_X_ISNULL);
      Scalar s;
      s.kind = Scalar::BOOL;
      return s;
   }
   if (op == "coalesce" || op == "case") { // coalesce(a, b) / case when c then a else b
      const bool isCase = op == "case";
      arity(isCase ? 3 : 2);
      if (isCase) compileX(sides, args.arr[0], b);
      XB lb, rb;
      const Scalar l = compileX(sides, args.arr[isCase ? 1 : 0], lb), r = compileX(sides, args.arr[isCase ? 2 : 1], rb);
      Scalar out = l;
      b.ins.insert(b.ins.end(), lb.ins.begin(), lb.ins.end());
      if (!floatPair(op, l, r) && (l.kind == Scalar::DEC || r.kind == Scalar::DEC)) {
         const DecimalType t = higherDecimalType(asDec(l), asDec(r));
         castTo(b, l, t);
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
         castTo(b, r, t);
         out = decScalar(t);
      } else {
         b.ins.insert(b.ins.end(), rb.ins.begin(), rb.ins.end());
      }
      b.push(isCase ? LDB_X_SELECT : LDB_X_COALESCE);
      return out;
   }
   if (op == "neg") {
      arity(1);
      const Scalar t = compileX(sides, args.arr[0], b);
      if (t.isFloat()) throw std::runtime_error("plan: neg of a float is not built");
      b.push(LDB_X_NEG);
      return t;
   }
   if (op == "f32" || op == "f64") { // float literal: {"f64": "0.85"}
      if (args.kind != J::STR) throw std::runtime_error("plan: a float literal is written {\"" + op + "\": \"0.85\"}");
      char* end = nullptr;
      const double v = strtod(args.str.c_str(), &end);
      if (args.str.empty() || *end) throw std::runtime_error("plan: float literal '" + args.str + "'");
      pushFConst(b, v, op == "f32" ? 32 : 64);
      return floatScalar(op == "f32" ? 32 : 64);
   }
   if (op == "cast") { // {"cast": [T, e]}: db.cast with a float on one side (CastOpLowering, LowerToStd.cpp:947-1018)
      arity(2);
      if (args.arr[0].kind != J::STR) throw std::runtime_error("plan: cast takes [type, expression]");
      const Scalar to = parseCastType(args.arr[0].str);
      const Scalar from = compileX(sides, args.arr[1], b);
      if (to.isFloat() && from.isFloat()) {
         if (to.kind != from.kind) b.push(LDB_X_FCVT, floatBits(to)); // arith.extf / truncf
         return to;
      }
      if (to.isFloat()) { // sitofp; a decimal then divides by (T) powf(10, s)
         b.push(LDB_X_I2F, floatBits(to));
         if (from.kind == Scalar::DEC && from.s > 0) {
            pushFConst(b, castPow10(from.s), floatBits(to));
            b.push(LDB_X_FDIV);
         }
         return to;
      }
      if (from.isFloat()) { // fptosi; a decimal target first multiplies by (T) powf(10, s)
         if (to.kind == Scalar::DEC && to.s > 0) {
            pushFConst(b, castPow10(to.s), floatBits(from));
            b.push(LDB_X_FMUL);
         }
         b.push(LDB_X_F2I);
         return to;
      }
      throw std::runtime_error("plan: cast from " + std::string(scalarName(from)) + " to " + args.arr[0].str + ": only casts with a float on one side are built");
   }
   throw std::runtime_error("plan: unknown expression operator '" + op + "'");
}

// aggregate argument → the sum-of-products normal form of ldb_expr (what the decimal lowerings
// reduce to once the scales are fixed); returns the result type
struct Interp::Factor {
   bool isCol = false, isConst = false;
   ldb_colref col{0, 0};
   __int128 k = 0; // constant (unscaled)
   int sign = 1; // (k + sign * col)
   bool constPlus = false;
   Scalar type;
};
Interp::Factor Interp::factorOf(const std::vector<const ldb_table*>& sides, const J& e) {
   Factor f;
   if (e.kind == J::NUM) {
      f.isConst = true;
      f.k = e.inum;
      return f;
   }
   if (e.kind == J::STR) {
      __int128 v;
      Scalar t;
      if (decimalLiteral(e.str, &v, &t)) {
         f.isConst = true;
         f.k = v;
         f.type = t;
         return f;
      }
      f.isCol = true;
      f.col = resolve(sides, e.str, "aggregate");
      if (typeOf(sides, f.col).type == LDB_T_UTF8) throw std::runtime_error("plan: the string column '" + e.str + "' inside an aggregate expression (only min / max of the bare column)");
      f.type = scalarOfCol(typeOf(sides, f.col));
      if (f.type.isFloat()) throw std::runtime_error("plan: aggregate over a float column is not built in the plan language");
      return f;
   }
   if (e.kind == J::OBJ && e.obj.size() == 1 && (e.obj[0].first == "add" || e.obj[0].first == "sub")) { // (k ± col)
      const J& a = e.obj[0].second;
      if (a.kind == J::ARR && a.arr.size() == 2 && a.arr[0].kind == J::NUM && a.arr[1].kind == J::STR) {
         f.constPlus = true;
         f.col = resolve(sides, a.arr[1].str, "aggregate");
         if (typeOf(sides, f.col).type == LDB_T_UTF8) throw std::runtime_error("plan: the string column '" + a.arr[1].str + "' inside an aggregate expression (only min / max of the bare column)");
         const Scalar ct = scalarOfCol(typeOf(sides, f.col));
         if (ct.isFloat()) throw std::runtime_error("plan: aggregate over a float column is not built in the plan language");
         f.sign = e.obj[0].first == "add" ? 1 : -1;
         if (ct.kind == Scalar::DEC) { // int literal → decimal(19,0) → common scale of the column (sql_analyzer.cpp:3125-3141)
            f.type = decScalar(higherDecimalType({19, 0}, {ct.p, ct.s}));
            f.k = (__int128) a.arr[0].inum * pow10i(ct.s);
         } else {
            f.type = ct;
            f.k = a.arr[0].inum;
         }
         return f;
      }
   }
   throw std::runtime_error("plan: aggregate factors must be a column, a literal or (integer ± column)");
}
Scalar Interp::termOf(const std::vector<const ldb_table*>& sides, const J& e, ldb_term* t) {
   memset(t, 0, sizeof(*t));
   std::vector<const J*> fs;
   if (e.kind == J::OBJ && e.obj.size() == 1 && e.obj[0].first == "mul") {
      for (auto& a : e.obj[0].second.arr) fs.push_back(&a);
   } else {
      fs.push_back(&e);
   }
   if (fs.size() > LDB_MAX_FACTORS) throw std::runtime_error("plan: more than 3 factors in an aggregate product");
   Scalar type;
   bool first = true;
   for (auto* fe : fs) {
      const Factor f = factorOf(sides, *fe);
      ldb_factor& o = t->f[t->n_factors++];
      if (f.isConst) {
         o = {0, {0, 0}, (int64_t) f.k, 0};
      } else if (f.constPlus) {
         o = {1, f.col, (int64_t) f.k, f.sign};
      } else {
         o = {1, f.col, 0, 1};
      }
      if (first) {
         type = f.type;
         first = false;
      } else if (type.kind == Scalar::DEC || f.type.kind == Scalar::DEC) {
         const DecimalType a = asDec(type), b2 = asDec(f.type), r = typeAfterMul(a, b2);
         if (a.s + b2.s != r.s) t->div_pow10 += a.s + b2.s - r.s; // clamped scale: truncating divide (LowerToStd.cpp:653-677)
         type = decScalar(r);
      }
   }
   return type;
}
Scalar Interp::aggExpr(const std::vector<const ldb_table*>& sides, const J& e, ldb_expr* out) {
   memset(out, 0, sizeof(*out));
   if (e.kind == J::OBJ && e.obj.size() == 1 && (e.obj[0].first == "add" || e.obj[0].first == "sub")) {
      const J& a = e.obj[0].second;
      const bool constPlusCol = a.kind == J::ARR && a.arr.size() == 2 && a.arr[0].kind == J::NUM && a.arr[1].kind == J::STR;
      if (!constPlusCol) { // difference / sum of two products (Q9's amount)
         if (a.kind != J::ARR || a.arr.size() != 2) throw std::runtime_error("plan: add/sub take two arguments");
         out->n_terms = 2;
         const Scalar l = termOf(sides, a.arr[0], &out->t[0]), r = termOf(sides, a.arr[1], &out->t[1]);
         out->t[1].negate = e.obj[0].first == "sub";
         if (l.kind != Scalar::DEC && r.kind != Scalar::DEC) return Scalar{};
         const DecimalType dl = asDec(l), dr = asDec(r), t = higherDecimalType(dl, dr);
         // bring both terms to the common scale with one more constant factor
         ldb_term* ts[2] = {&out->t[0], &out->t[1]};
         const DecimalType ds[2] = {dl, dr};
         for (int i = 0; i < 2; i++) {
            if (ds[i].s < t.s) {
               if (ts[i]->n_factors >= LDB_MAX_FACTORS) throw std::runtime_error("plan: no room for the scale factor in an aggregate term");
               ts[i]->f[ts[i]->n_factors++] = {0, {0, 0}, pow10i(t.s - ds[i].s), 0};
            }
         }
         return decScalar(t);
      }
   }
   out->n_terms = 1;
   return termOf(sides, e, &out->t[0]);
}

} // namespace ldbplan
