// ldb_subop_expr.cpp — the sub-operator dump consumer's expressions and restrictions: the dump's expression trees → Expr (convert), Expr → the plan
// language (exprJson), computed columns as map steps (ensureCol), conditions as restrictions (condPreds / applyFilter), and the helpers that
// append steps (emit / flush).  Declarations: ldb_subop_translate.hpp.
#include "ldb_subop_translate.hpp"

namespace ldbsubop {

std::string exprJson(const ExprP& e0) { // the plan language of ldb_plan.cpp (compileX)
   const ExprP e = stripCast(e0); // db.cast is implicit there: operands are typed by the reference's decimal rules
   switch (e->kind) {
      case Expr::COL: return quote(e->name);
      case Expr::CONST_INT: return std::to_string(e->i);
      case Expr::CONST_STR: return quote(e->name);
      case Expr::OP: {
         if (e->name == "cmp") return "{\"cmp\": [" + quote(e->cmp) + ", " + exprJson(e->args[0]) + ", " + exprJson(e->args[1]) + "]}";
         if (e->name == "select") return "{\"case\": [" + exprJson(e->args[0]) + ", " + exprJson(e->args[1]) + ", " + exprJson(e->args[2]) + "]}";
         if (e->name == "add" || e->name == "sub" || e->name == "mul" || e->name == "div" || e->name == "and" || e->name == "or" || e->name == "not" || e->name == "isnull" || e->name == "coalesce") {
            std::string o = "{" + quote(e->name) + ": [";
            if ((e->name == "and" || e->name == "or" || e->name == "mul") && e->args.size() > 2) { // n-ary in the dump, flattened for mul, nested for and/or
               if (e->name == "mul") {
                  for (size_t k = 0; k < e->args.size(); k++) o += (k ? ", " : "") + exprJson(e->args[k]);
                  return o + "]}";
               }
               ExprP acc = e->args[0];
               for (size_t k = 1; k < e->args.size(); k++) {
                  ExprP n = mk(Expr::OP, e->name);
                  n->args = {acc, e->args[k]};
                  acc = n;
               }
               return exprJson(acc);
            }
            for (size_t k = 0; k < e->args.size(); k++) o += (k ? ", " : "") + exprJson(e->args[k]);
            return o + "]}";
         }
         throw Unsupported("expression '" + e->name + "' has no device form");
      }
      default: throw Unsupported("expression leaf without a device form");
   }
}
// (a * b) * c → one n-ary product, the form the aggregate normal form of ldb_plan.cpp recognises
ExprP flattenMul(const ExprP& e) {
   if (e->kind != Expr::OP) return e;
   auto r = std::make_shared<Expr>(*e);
   r->args.clear();
   for (auto& a : e->args) {
      ExprP f = flattenMul(a);
      if (e->name == "mul" && f->kind == Expr::OP && f->name == "mul")
         for (auto& g : f->args) r->args.push_back(g);
      else
         r->args.push_back(f);
   }
   return r;
}

static bool strs(const J& e, std::initializer_list<const char*> want) {
   const J& s = e.at("strings");
   if (s.kind != J::ARR || s.arr.size() != want.size()) return false;
   size_t k = 0;
   for (const char* w : want)
      if (s.arr[k++].str != w) return false;
   return true;
}
ExprP Translator::convert(const J& e, const Stream& st) {
   const std::string& type = e.s("type");
   if (type == "expression_leaf") {
      const std::string& leaf = e.s("leaf_type");
      if (leaf == "column" || leaf == "external_column") {
         auto it = st.cols.find(e.s("displayName"));
         if (it == st.cols.end()) throw Unsupported("column '" + e.s("displayName") + "' is not defined on this stream");
         return it->second;
      }
      if (leaf == "constant") {
         const J& v = e.at("value");
         if (v.kind == J::NUM && v.isInt) {
            ExprP c = mk(Expr::CONST_INT);
            c->i = v.inum;
            c->cmp = e.sOr("data_type", "");
            return c;
         }
         if (v.kind == J::STR) return mk(Expr::CONST_STR, v.str);
         if (v.kind == J::BOOL) {
            ExprP c = mk(Expr::CONST_BOOL);
            c->i = v.b;
            return c;
         }
         throw Unsupported("floating-point constant");
      }
      if (leaf == "member") return mk(Expr::MEMBER, e.s("member"));
      if (leaf == "null") return mk(Expr::NULLV);
      return mk(Expr::UNKNOWN); // "unknown" / "null": only legal inside the recognised aggregate bodies
   }
   if (type != "expression_inner") throw Unsupported("expression node of type '" + type + "'");
   const J& subs = e.at("subExpressions");
   std::vector<ExprP> a;
   for (auto& s : subs.arr) a.push_back(convert(s, st));
   auto op = [&](const char* name, size_t n) {
      if (a.size() != n) throw Unsupported(std::string("malformed '") + name + "' expression");
      ExprP r = mk(Expr::OP, name);
      r->args = a;
      return r;
   };
   const J& ss = e.at("strings");
   const std::string first = ss.arr.empty() ? "" : ss.arr[0].str;
   if (strs(e, {"", " * ", ""})) return op("mul", 2);
   if (strs(e, {"", " + ", ""})) {
      // the unpatched tool prints db.sub with the separator " + " too (mlir-subop-to-json.cpp:315-317): a sum is a sum only from an emitter with E1
      if (!ext.count("E1")) throw Unsupported("' + ' is ambiguous without emitter extension E1: the unpatched tool prints db.sub as ' + ' as well (mlir-subop-to-json.cpp:315-317)");
      return op("add", 2);
   }
   if (strs(e, {"", " - ", ""})) return op("sub", 2); // emitter extension E1
   if (strs(e, {"", " / ", ""})) return op("div", 2);
   if (strs(e, {"cast(", ")"})) return op("cast", 1);
   if (strs(e, {"not ", ""})) return op("not", 1);
   if (strs(e, {"", " is null"})) return op("isnull", 1);
   if (strs(e, {"", " ? ", " : ", ""})) return op("select", 3);
   if (strs(e, {"if ", " then ", " else ", ""})) return op("select", 3);
   if (strs(e, {"", " between ", " and ", ""})) {
      // db.between carries lowerInclusive / upperInclusive (DBOps.td:507); `x >= a and x < b` is canonicalised into a HALF-OPEN one (DBOps.cpp:475-483,
      // lowered at LowerToStd.cpp:1026) and the unpatched tool drops both flags (mlir-subop-to-json.cpp:261-263): only an emitter with E10 says which
      if (a.size() != 3) throw Unsupported("malformed between");
      const J *li = e.get("lowerInclusive"), *ui = e.get("upperInclusive");
      if (!ext.count("E10") || !li || !ui || li->kind != J::BOOL || ui->kind != J::BOOL)
         throw Unsupported("db.between without its lowerInclusive / upperInclusive flags (emitter extension E10): the unpatched tool prints a half-open range like a closed one (mlir-subop-to-json.cpp:261-263)");
      ExprP lo = mk(Expr::OP, "cmp"), hi = mk(Expr::OP, "cmp"), r = mk(Expr::OP, "and");
      lo->cmp = li->b ? "GTE" : "GT", lo->args = {a[0], a[1]};
      hi->cmp = ui->b ? "LTE" : "LT", hi->args = {a[0], a[2]};
      r->args = {lo, hi};
      return r;
   }
   if (first == "hash(") { // hash(x) or hash(pack(x, y, …)): only the hashed columns matter
      ExprP h = mk(Expr::HASH);
      h->args = a.size() == 1 && a[0]->kind == Expr::OP && a[0]->name == "pack" ? a[0]->args : a;
      return h;
   }
   if (first == "pack(") {
      ExprP r = mk(Expr::OP, "pack");
      r->args = a;
      return r;
   }
   if (ss.arr.size() == 3 && ss.arr[0].str.empty() && ss.arr[2].str.empty() && a.size() == 2) { // db.compare: convertCmpPredicate, no spaces
      static const std::pair<const char*, const char*> cmps[] = {{"=", "EQ"}, {"<>", "NEQ"}, {"<", "LT"}, {"<=", "LTE"}, {">", "GT"}, {">=", "GTE"}, {"isa", "EQ"}};
      for (auto& c : cmps)
         if (ss.arr[1].str == c.first) {
            ExprP r = mk(Expr::OP, "cmp");
            r->cmp = c.second;
            r->args = a;
            return r;
         }
   }
   if (ss.arr.size() >= 3 && first.empty() && ss.arr[1].str == " and ") {
      ExprP r = mk(Expr::OP, "and");
      r->args = a;
      return r;
   }
   if (ss.arr.size() >= 3 && first == "(" && ss.arr[1].str == " or ") {
      ExprP r = mk(Expr::OP, "or");
      r->args = a;
      return r;
   }
   if (first.empty() && ss.arr.size() >= 3 && ss.arr[1].str == " in [") {
      ExprP r = mk(Expr::OP, "in");
      r->args = a;
      return r;
   }
   if (first.size() > 1 && first.back() == '(' && isalpha((unsigned char) first[0])) { // db.runtime_call: "Fn(" a ", " b ")" (mlir-subop-to-json.cpp:318-326)
      ExprP r = mk(Expr::OP, "call");
      r->cmp = first.substr(0, first.size() - 1);
      r->args = a;
      return r;
   }
   throw Unsupported("expression '" + first + "…' (operator without a device form)");
}

// ---------------------------------------------------------------- emission helpers
std::string Translator::emit(const char* op, const char* stem, Fields fields) {
   OutStep st;
   st.op = op;
   st.out = fresh(stem);
   st.fields = std::move(fields);
   steps.push_back(st);
   return st.out;
}
void Translator::flush(Stream& s) { // apply pending restrictions as a filter step
   if (!s.preds.empty()) s.rel = emit("filter", "v", {{"in", quote(s.rel)}, {"preds", joined(s.preds)}});
   s.preds.clear();
   s.bareTable = false;
}
void Translator::use(const std::string& col) {
   auto it = aggCol.find(col);
   if (it != aggCol.end()) steps[(size_t) it->second.first].aggs[(size_t) it->second.second].used = true;
}
void Translator::useAll(const ExprP& e) {
   if (e->kind == Expr::COL) use(e->name);
   for (auto& a : e->args) useAll(a);
}
// the runtime calls with a device form: the `fn` of the map step each becomes and, for the calls of DateRuntime::extract*, the date part
// (also the parts DateTrunc may name; the year keeps its own form, extract_year, without a part field)
struct DeviceCall {
   const char* call;
   size_t nargs;
   const char *fn, *part;
};
static const DeviceCall kDeviceCalls[] = {{"ExtractYearFromDate", 1, "extract_year", "year"}, {"ExtractMonthFromDate", 1, "extract", "month"}, {"ExtractDayFromDate", 1, "extract", "day"},
                                          {"ExtractHourFromDate", 1, "extract", "hour"},      {"ExtractMinuteFromDate", 1, "extract", "minute"}, {"ExtractSecondFromDate", 1, "extract", "second"},
                                          {"DateTrunc", 2, "date_trunc", nullptr},             {"Substring", 3, "substr", nullptr},               {"ToUpper", 1, "upper", nullptr},
                                          {"ToLower", 1, "lower", nullptr},                    {"StringLength", 1, "length", nullptr},            {"Concatenate", 2, "concat", nullptr}};
static const DeviceCall* deviceCall(const std::string& call) {
   for (auto& d : kDeviceCalls)
      if (call == d.call) return &d;
   return nullptr;
}
static bool isDatePart(const std::string& part) {
   for (auto& d : kDeviceCalls)
      if (d.part && part == d.part) return true;
   return false;
}
// runtime calls nested inside an expression become columns first (the expression language is arithmetic / boolean only)
ExprP Translator::materializeCalls(Stream& s, const ExprP& e, const std::string& hint) {
   if (e->kind != Expr::OP) return e;
   if (e->name == "call" && deviceCall(e->cmp)) return mk(Expr::COL, ensureCol(s, e, hint + "_f" + std::to_string(++nval)));
   bool changed = false;
   std::vector<ExprP> args;
   for (auto& a : e->args) {
      ExprP n = materializeCalls(s, a, hint);
      changed = changed || n != a;
      args.push_back(n);
   }
   if (!changed) return e;
   auto r = std::make_shared<Expr>(*e);
   r->args = args;
   return r;
}
// the operands of a Concatenate nest, left to right, as the parts of a `concat` map step: string constants, columns, a Substring with
// constant bounds of a column, ToUpper / ToLower of a column or of such a Substring; anything else has no device form
void Translator::concatParts(const ExprP& e, std::vector<std::string>& out) {
   auto isCall = [](const ExprP& x, const char* fn, size_t n) { return x->kind == Expr::OP && x->name == "call" && x->cmp == fn && x->args.size() == n; };
   if (isCall(e, "Concatenate", 2)) {
      concatParts(e->args[0], out);
      concatParts(e->args[1], out);
      return;
   }
   if (e->kind == Expr::CONST_STR) {
      out.push_back("{\"const\": " + quote(e->name) + "}");
      return;
   }
   std::string mapping;
   ExprP x = e;
   if (isCall(x, "ToUpper", 1) || isCall(x, "ToLower", 1)) {
      mapping = x->cmp == "ToUpper" ? ", \"case\": \"upper\"" : ", \"case\": \"lower\"";
      x = x->args[0];
   }
   std::string window;
   if (isCall(x, "Substring", 3) && stripCast(x->args[1])->kind == Expr::CONST_INT && stripCast(x->args[2])->kind == Expr::CONST_INT) {
      window = ", \"from\": " + std::to_string(stripCast(x->args[1])->i) + ", \"for\": " + std::to_string(stripCast(x->args[2])->i);
      x = x->args[0];
   }
   if (x->kind != Expr::COL) throw Unsupported(x->kind == Expr::OP ? "'" + (x->name == "call" ? x->cmp : x->name) + "' inside Concatenate has no device form" : "this operand of Concatenate has no device form");
   use(x->name);
   out.push_back("{\"col\": " + quote(x->name) + mapping + window + "}");
}
// a plain column holding `e` on the stream: a computed expression becomes a `map` step
std::string Translator::ensureCol(Stream& s, const ExprP& e0, const std::string& hint) {
   const ExprP e = stripCast(e0);
   if (e->kind == Expr::COL) {
      use(e->name);
      return e->name;
   }
   const std::string as = sanitize(hint);
   Fields f; // what the map step says between "in" and "as"
   if (e->kind == Expr::OP && e->name == "call") { // the runtime functions with a device kernel
      const DeviceCall* dc = deviceCall(e->cmp);
      if (!dc || e->args.size() != dc->nargs) throw Unsupported("runtime function '" + e->cmp + "' has no device form");
      const ExprP a0 = stripCast(e->args[0]);
      f = {{"fn", quote(dc->fn)}};
      if (e->cmp == "Concatenate") { // StringRuntime::concat, nested left or right: one part list
         std::vector<std::string> parts;
         concatParts(e, parts);
         if (parts.size() > 8) throw Unsupported("a concatenation of " + std::to_string(parts.size()) + " parts (the device form takes 8)");
         f.push_back({"parts", joined(parts)});
      } else if (e->cmp == "DateTrunc") { // DateRuntime::dateTrunc(part, date): the part must be a constant the device form knows
         if (a0->kind != Expr::CONST_STR) throw Unsupported("DateTrunc with a part that is not a string constant has no device form");
         if (!isDatePart(a0->name)) throw Unsupported("DateTrunc part '" + a0->name + "' has no device form");
         const std::string src = ensureCol(s, stripCast(e->args[1]), hint + "_arg");
         f.insert(f.end(), {{"part", quote(a0->name)}, {"col", quote(src)}});
      } else if (e->cmp == "Substring") { // StringRuntime::substr(str, from, len) with constant bounds
         const ExprP from = stripCast(e->args[1]), len = stripCast(e->args[2]);
         if (from->kind != Expr::CONST_INT || len->kind != Expr::CONST_INT) throw Unsupported("runtime function '" + e->cmp + "' has no device form");
         const std::string src = ensureCol(s, a0, hint + "_arg");
         f.insert(f.end(), {{"col", quote(src)}, {"from", std::to_string(from->i)}, {"for", std::to_string(len->i)}});
      } else { // DateRuntime::extractYear … extractSecond, StringRuntime::toUpper / toLower / len over a column
         const std::string src = ensureCol(s, a0, hint + "_arg");
         if (dc->part && std::string(dc->fn) == "extract") f.push_back({"part", quote(dc->part)});
         f.push_back({"col", quote(src)});
      }
      flush(s);
   } else {
      const ExprP x = materializeCalls(s, e, hint);
      flush(s);
      useAll(x);
      f = {{"expr", exprJson(flattenMul(x))}};
   }
   f.insert(f.begin(), {"in", quote(s.rel)});
   f.push_back({"as", quote(as)});
   s.rel = emit("map", "v", f);
   s.names.insert(as);
   ExprP c = mk(Expr::COL, as);
   for (auto& kv : s.cols)
      if (kv.second == e0) kv.second = c;
   return as;
}

// a condition as a conjunction of the plan language's restrictions: column-vs-constant comparisons, AND of such, and an
// OR of equalities on ONE column (→ IN); false when it is anything else
bool Translator::condPreds(const ExprP& c0, std::vector<std::string>& out) {
   const ExprP c = stripCast(c0);
   if (c->kind != Expr::OP) return false;
   auto lit = [](const ExprP& k) { return k->kind == Expr::CONST_INT ? std::to_string(k->i) : quote(k->name); };
   auto isConst = [](const ExprP& k) { return k->kind == Expr::CONST_INT || k->kind == Expr::CONST_STR; };
   if (c->name == "and") {
      for (auto& a : c->args)
         if (!condPreds(a, out)) return false;
      return true;
   }
   if (c->name == "cmp") {
      ExprP l = stripCast(c->args[0]), r = stripCast(c->args[1]);
      std::string op = c->cmp;
      if (l->kind != Expr::COL && r->kind == Expr::COL) {
         std::swap(l, r);
         op = mirrored(op);
      }
      if (l->kind != Expr::COL || !isConst(r)) return false;
      use(l->name);
      out.push_back("{\"col\": " + quote(l->name) + ", \"op\": " + quote(op) + ", \"value\": " + lit(r) + "}");
      return true;
   }
   if (c->name == "in") { // db.oneof: column in [constants]
      const ExprP l = stripCast(c->args[0]);
      if (l->kind != Expr::COL || c->args.size() < 2) return false;
      std::string vals;
      for (size_t k = 1; k < c->args.size(); k++) {
         const ExprP v = stripCast(c->args[k]);
         if (!isConst(v)) return false;
         vals += (vals.empty() ? "" : ", ") + lit(v);
      }
      use(l->name);
      out.push_back("{\"col\": " + quote(l->name) + ", \"op\": \"IN\", \"values\": [" + vals + "]}");
      return true;
   }
   if (c->name == "call" || (c->name == "not" && stripCast(c->args[0])->kind == Expr::OP && stripCast(c->args[0])->name == "call")) { // [not] ConstLike(column, pattern)
      const bool neg = c->name == "not";
      const ExprP f = neg ? stripCast(c->args[0]) : c;
      if ((f->cmp != "ConstLike" && f->cmp != "Like") || f->args.size() != 2) return false;
      const ExprP l = stripCast(f->args[0]), pat = stripCast(f->args[1]);
      if (l->kind != Expr::COL || pat->kind != Expr::CONST_STR) return false;
      use(l->name);
      out.push_back("{\"col\": " + quote(l->name) + ", \"op\": " + (neg ? "\"NOT LIKE\"" : "\"LIKE\"") + ", \"value\": " + quote(pat->name) + "}");
      return true;
   }
   if (c->name == "not" && stripCast(c->args[0])->kind == Expr::OP && stripCast(c->args[0])->name == "isnull") { // not (x is null)
      const ExprP l = stripCast(stripCast(c->args[0])->args[0]);
      if (l->kind != Expr::COL) return false;
      use(l->name);
      out.push_back("{\"col\": " + quote(l->name) + ", \"op\": \"NOTNULL\"}");
      return true;
   }
   if (c->name == "or") {
      std::string col, vals;
      for (auto& a0 : c->args) {
         const ExprP a = stripCast(a0);
         if (!(a->kind == Expr::OP && a->name == "cmp" && a->cmp == "EQ")) return false;
         ExprP l = stripCast(a->args[0]), r = stripCast(a->args[1]);
         if (l->kind != Expr::COL) std::swap(l, r);
         if (l->kind != Expr::COL || !isConst(r) || (!col.empty() && col != l->name)) return false;
         col = l->name;
         vals += (vals.empty() ? "" : ", ") + lit(r);
      }
      if (col.empty()) return false;
      use(col);
      out.push_back("{\"col\": " + quote(col) + ", \"op\": \"IN\", \"values\": [" + vals + "]}");
      return true;
   }
   return false;
}
std::string Translator::predJson(const std::string& col, const std::string& op, const J* value, const J* values) {
   std::string p = "{\"col\": " + quote(col) + ", \"op\": " + quote(op);
   auto lit = [](const J& v) { return v.kind == J::STR ? quote(v.str) : v.kind == J::NUM && v.isInt ? std::to_string(v.inum) : std::to_string(v.num); };
   if (values) {
      p += ", \"values\": [";
      for (size_t k = 0; k < values->arr.size(); k++) p += (k ? ", " : "") + lit(values->arr[k]);
      p += "]";
   } else if (value && op != "NOTNULL") {
      p += ", \"value\": " + lit(*value);
   }
   return p + "}";
}
// a restriction on the rows of a stream: conjunctions of column-vs-constant comparisons / IN / LIKE / NOT NULL, two
// columns of base tables, a disjunction of such conjunctions (→ filter_dnf), or any arithmetic / boolean expression
// (→ a computed boolean column + `= true`)
void Translator::applyFilter(Stream& s, const ExprP& e0) {
   const ExprP e = materializeCalls(s, stripCast(e0), "pred");
   std::vector<std::string> ps;
   if (condPreds(e, ps)) {
      s.preds.insert(s.preds.end(), ps.begin(), ps.end());
      return;
   }
   if (e->kind == Expr::OP && e->name == "cmp") {
      const ExprP l = stripCast(e->args[0]), r = stripCast(e->args[1]);
      if (l->kind == Expr::COL && r->kind == Expr::COL && l->base && r->base) {
         use(l->name), use(r->name);
         s.preds.push_back("{\"col\": " + quote(l->name) + ", \"op\": " + quote(e->cmp) + ", \"rhs_col\": " + quote(r->name) + "}");
         return;
      }
   }
   if (e->kind == Expr::OP && e->name == "or") { // disjunctive normal form
      std::vector<std::string> clauses;
      bool ok = true;
      for (size_t k = 0; k < e->args.size() && ok; k++) {
         std::vector<std::string> cl;
         ok = condPreds(e->args[k], cl);
         clauses.push_back(joined(cl));
      }
      if (ok) {
         flush(s);
         s.rel = emit("filter_dnf", "v", {{"in", quote(s.rel)}, {"clauses", joined(clauses)}});
         return;
      }
   }
   const std::string col = ensureCol(s, e, "pred" + std::to_string(++nval));
   s.preds.push_back("{\"col\": " + quote(col) + ", \"op\": \"EQ\", \"value\": 1}");
}

} // namespace ldbsubop
