// ldb_plan_steps.cpp — the plan interpreter's environment and its steps: one function per step of the plan language,
// nested_map and loop on top of them, and the step table that the interpreter and the structure check both read.
#include "ldb_plan_interp.hpp"
#include <algorithm>
#include <chrono>

namespace ldbplan {

// "case" of a concat part
int32_t strcaseOf(const std::string& c) {
   if (c == "none") return LDB_SC_NONE;
   if (c == "upper") return LDB_SC_UPPER;
   if (c == "lower") return LDB_SC_LOWER;
   throw std::runtime_error("plan: map concat: unknown case '" + c + "' (none, upper, lower)");
}
int32_t datepartOf(const std::string& p) {
   static const char* const names[] = {"year", "month", "day", "hour", "minute", "second"}; // ldb_datepart
   for (int32_t k = 0; k < 6; k++)
      if (p == names[k]) return k;
   return -1;
}

// ================================================================== environment
// the named values (nullptr: all of them) and the hidden tables from index `hiddenFrom` on: hash tables first (they reference relations), then
// relations, then tables
void Interp::releaseValues(const std::vector<std::string>* names, size_t hiddenFrom) {
   auto each = [&](auto&& f) {
      if (names)
         for (auto& n : *names) f(env[n]);
      else
         for (auto& kv : env) f(kv.second);
   };
   each([&](Value& v) {
      if (v.kind == Value::HT && v.owned && v.ht) ldb_gpu_hashtable_release(ctx, v.ht);
   });
   each([&](Value& v) {
      if (v.lazyRel) ldb_gpu_rel_release(ctx, v.lazyRel);
      if (v.kind == Value::REL && v.owned && v.rel) ldb_gpu_rel_release(ctx, v.rel);
   });
   each([&](Value& v) {
      if (v.kind == Value::TABLE && v.owned && v.table) ldb_gpu_table_release(ctx, const_cast<ldb_table*>(v.table));
   });
   if (names)
      for (auto& n : *names) env.erase(n);
   else
      env.clear();
   for (size_t h = hiddenFrom; h < hidden.size(); h++) ldb_gpu_table_release(ctx, hidden[h]);
   hidden.resize(hiddenFrom);
}
Interp::~Interp() { releaseValues(nullptr, 0); }
ldb_table* Interp::takeResult() {
   Value& r = val(result);
   if (r.kind != Value::TABLE || !r.owned) throw std::runtime_error("plan: result '" + result + "' must be a table produced by the plan");
   r.owned = false; // taken: the caller releases it
   return const_cast<ldb_table*>(r.table);
}

Value& Interp::val(const std::string& name) {
   auto it = env.find(name);
   if (it == env.end()) throw std::runtime_error("plan: unknown value '" + name + "'");
   return it->second;
}
// a value as a relation (tables get an identity relation on first use)
ldb_rel* Interp::relOf(const std::string& name, std::vector<const ldb_table*>** sides) {
   Value& v = val(name);
   if (v.kind == Value::HT) throw std::runtime_error("plan: '" + name + "' is a hash table, a relation is expected");
   if (v.kind == Value::TABLE) {
      if (!v.lazyRel) check(ldb_gpu_rel_from_table(ctx, v.table, &v.lazyRel), "scan");
      if (v.sides.empty()) v.sides = {v.table};
      if (sides) *sides = &v.sides;
      return v.lazyRel;
   }
   if (sides) *sides = &v.sides;
   return v.rel;
}
int64_t Interp::rowsOf(const std::string& name) {
   Value& v = val(name);
   if (v.kind == Value::TABLE) return ldb_gpu_table_rows(v.table);
   if (v.kind == Value::REL) return ldb_gpu_rel_rows(ctx, v.rel);
   throw std::runtime_error("plan: '" + name + "' has no row count");
}
void Interp::put(const std::string& name, Value v) {
   if (env.count(name)) throw std::runtime_error("plan: value '" + name + "' defined twice");
   env.emplace(name, std::move(v));
}
// putRel / putTable / putHt / hide take a fresh handle over from its holder — once the environment has it, not before
void Interp::putRel(const std::string& name, OwnedRel& r, std::vector<const ldb_table*> sides) {
   Value v;
   v.kind = Value::REL;
   v.rel = r.get();
   v.owned = true;
   v.sides = std::move(sides);
   put(name, std::move(v));
   r.release();
}
void Interp::putTable(const std::string& name, OwnedTable& t) {
   Value v;
   v.kind = Value::TABLE;
   v.table = t.get();
   v.owned = true;
   put(name, std::move(v));
   t.release();
}
void Interp::putHt(const std::string& name, OwnedHt& ht, std::vector<const ldb_table*> sides) {
   Value v;
   v.kind = Value::HT;
   v.ht = ht.get();
   v.owned = true;
   v.sides = std::move(sides);
   put(name, std::move(v));
   ht.release();
}
void Interp::hide(OwnedTable& t) {
   ldb_table* const p = t.get();
   hidden.push_back(p);
   t.release();
}

// "name" or "side:name" → column reference inside a relation with the given side tables
ldb_colref Interp::resolve(const std::vector<const ldb_table*>& sides, const std::string& ref, const char* what) {
   const auto colon = ref.find(':');
   if (colon != std::string::npos && colon > 0 && isdigit((unsigned char) ref[0])) {
      const int side = std::stoi(ref.substr(0, colon));
      if (side < 0 || (size_t) side >= sides.size()) throw std::runtime_error(std::string(what) + ": side out of range in '" + ref + "'");
      const int32_t c = ldb_gpu_table_col_index(sides[(size_t) side], ref.substr(colon + 1).c_str());
      if (c < 0) throw std::runtime_error(std::string(what) + ": no column '" + ref + "'");
      return {side, c};
   }
   for (size_t s = 0; s < sides.size(); s++) {
      const int32_t c = ldb_gpu_table_col_index(sides[s], ref.c_str());
      if (c >= 0) return {(int32_t) s, c};
   }
   throw std::runtime_error(std::string(what) + ": no column '" + ref + "' in the relation");
}
ldb_coltype Interp::typeOf(const std::vector<const ldb_table*>& sides, ldb_colref c) {
   ldb_coltype t;
   ldb_gpu_table_coltype(sides[(size_t) c.side], c.col, &t);
   return t;
}

// ------------------------------------------------------------ steps
void Interp::run(const J& plan, const char* const* names, const ldb_table* const* tables, int32_t n) {
   for (int32_t i = 0; i < n; i++) {
      Value v;
      v.kind = Value::TABLE;
      v.table = tables[i];
      put(names[i], v);
   }
   const J& steps = plan.at("steps");
   result = plan.sOr("result", "result");
   static const bool stepTrace = getenv("LDB_PLAN_STEP_TRACE") != nullptr; // diagnostics: host time of every step on stderr
   for (auto& st : steps.arr) {
      try {
         const auto t0 = std::chrono::steady_clock::now();
         step(st);
         if (stepTrace)
            fprintf(stderr, "[ldb plan] %s: %s -> %s: %.3f ms host\n", plan.sOr("name", "plan").c_str(), st.sOr("op", "?").c_str(), st.sOr("out", "").c_str(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      } catch (const std::exception& e) {
         throw std::runtime_error(plan.sOr("name", "plan") + ": step '" + st.sOr("op", "?") + "' → '" + st.sOr("out", "") + "': " + e.what());
      }
   }
}

// ---- pieces that several steps share
std::vector<ldb_colref> Interp::cols(const std::vector<const ldb_table*>& sides, const J& list, const char* what) {
   std::vector<ldb_colref> out;
   for (auto& c : list.arr) out.push_back(resolve(sides, c.kind == J::STR ? c.str : c.s("col"), what));
   return out;
}
// the step's "residual" list: column-vs-column conjuncts between the probe and the build side of a join
std::vector<ldb_join_residual> Interp::residuals(const J& st, const Sides& probe, const Sides& build, const char* whatProbe, const char* whatBuild) {
   std::vector<ldb_join_residual> resid;
   if (const J* rs = st.get("residual"))
      for (auto& r : rs->arr) resid.push_back({resolve(probe, r.s("probe"), whatProbe), resolve(build, r.s("build"), whatBuild), opOf(r.s("op")), 0});
   return resid;
}
// "by" / "order_by": column names, or {"col", "desc"}.  A plan states a reference query, and the reference's comparator is total over NULLs
// (SimplifySortComparePattern, PrepareLowering.cpp:106-132): every key orders NULL as the largest value
std::vector<ldb_sort_spec> Interp::sortSpecs(const Sides& sides, const J& by, const char* what) {
   std::vector<ldb_sort_spec> specs;
   for (auto& b : by.arr)
      specs.push_back({resolve(sides, b.kind == J::STR ? b.str : b.s("col"), what), b.kind == J::OBJ && b.bOr("desc", false) ? 1 : 0, LDB_NULLS_LARGEST});
   return specs;
}
// the {"col", "as"} entries of a column list name the columns of the table made from it
static void renameCols(ldb_table* t, const J& cols) {
   size_t i = 0;
   for (auto& c : cols.arr) {
      if (c.kind == J::OBJ)
         if (const J* as = c.get("as")) ldb_gpu_table_rename_col(t, (int32_t) i, as->str.c_str());
      i++;
   }
}
// a conjunction of any length, kMaxConjuncts at a time, over `cur` (over `in`, which is not ours, while `cur` is empty): the next relation is
// made first, the intermediate one released after.  evenIfEmpty: one call with no conjuncts when there are none
void Interp::filterInChunks(ldb_rel* in, OwnedRel& cur, const std::vector<ldb_filter_desc>& fs, bool evenIfEmpty, const char* what, const char* whatRelease) {
   for (size_t at = 0; at < fs.size() || (at == 0 && evenIfEmpty); at += kMaxConjuncts) {
      const size_t n = std::min<size_t>(kMaxConjuncts, fs.size() - at);
      OwnedRel next(ctx);
      check(ldb_gpu_scan_filter(ctx, cur.get() ? cur.get() : in, fs.data() + at, (int32_t) n, next.out()), what);
      check(cur.reset(next.release()), whatRelease);
   }
}

// the join kinds of each family, and which sides the result has
enum JoinSides { PROBE_SIDES, BUILD_SIDES, BOTH_SIDES };
struct JoinKind {
   const char* name;
   int32_t kind;
   JoinSides sides;
};
static const JoinKind kProbeKinds[] = {{"inner", LDB_JOIN_INNER, BOTH_SIDES},           {"semi", LDB_JOIN_SEMI, PROBE_SIDES},
                                       {"anti", LDB_JOIN_ANTI, PROBE_SIDES},            {"left_outer", LDB_JOIN_LEFT_OUTER, BOTH_SIDES},
                                       {"mark", LDB_JOIN_MARK, PROBE_SIDES},            {"single", LDB_JOIN_SINGLE, BOTH_SIDES},
                                       {"semi_build", LDB_JOIN_SEMI_BUILD, BUILD_SIDES}, {"anti_build", LDB_JOIN_ANTI_BUILD, BUILD_SIDES},
                                       {"right_outer", LDB_JOIN_RIGHT_OUTER, BOTH_SIDES}, {"full_outer", LDB_JOIN_FULL_OUTER, BOTH_SIDES}};
static const JoinKind kNlKinds[] = {{"inner", LDB_JOIN_INNER, BOTH_SIDES},           {"semi", LDB_JOIN_SEMI, PROBE_SIDES},
                                    {"anti", LDB_JOIN_ANTI, PROBE_SIDES},            {"left_outer", LDB_JOIN_LEFT_OUTER, BOTH_SIDES},
                                    {"semi_build", LDB_JOIN_SEMI_BUILD, BUILD_SIDES}, {"anti_build", LDB_JOIN_ANTI_BUILD, BUILD_SIDES}};
template <size_t N>
static const JoinKind& joinKindOf(const JoinKind (&kinds)[N], const std::string& name, const char* unknown) {
   for (auto& k : kinds)
      if (name == k.name) return k;
   throw std::runtime_error(unknown);
}
static Sides joinOutSides(const JoinKind& k, const Sides& probe, const Sides& build) {
   if (k.sides == BUILD_SIDES) return build;
   Sides out = probe;
   if (k.sides == BOTH_SIDES) out.insert(out.end(), build.begin(), build.end());
   return out;
}

// ---- the steps
void Interp::stepScan(const J& st) { // subop.scan_refs over a table (get_external)
   Value& t = val(st.s("table"));
   if (t.kind != Value::TABLE) throw std::runtime_error("scan: not a table");
   OwnedRel r(ctx);
   check(ldb_gpu_rel_from_table(ctx, t.table, r.out()), "scan");
   putRel(st.s("out"), r, {t.table});
}

void Interp::stepFilter(const J& st) {
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto ps = preds(*sides, &st.at("preds"));
   // Limits of ONE scan_filter call that the reference's Restrictions do not have (round 6): a conjunction of more than eight conjuncts is applied
   // eight at a time (a conjunction may be evaluated in any order); an integer IN list of more than eight constants — Restrictions.cpp:481-515 keeps
   // a hash set of any size — becomes what it is relationally: a semi join against the table of its constants;
   // a string IN list of any size, and a string constant of any length, go to scan_filter as they are (its string-set kernel)
   std::vector<ldb_filter_desc> plain, longIn;
   for (auto& d : ps) (d.op == LDB_F_IN && d.n_in > kMaxInConstants && d.in_values ? longIn : plain).push_back(d);
   OwnedRel cur(ctx); // empty: still `in`
   filterInChunks(in, cur, plain, longIn.empty(), "filter", "filter (intermediate)");
   for (auto& d : longIn) {
      ldb_rel* next = semiJoinConstants(cur.get() ? cur.get() : in, d, *sides, st.s("out"));
      check(cur.reset(next), "filter (intermediate)");
   }
   putRel(st.s("out"), cur, *sides);
}

void Interp::stepFilterDnf(const J& st) {
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   std::vector<ldb_filter_desc> all;
   std::vector<int32_t> sizes;
   for (auto& cl : st.at("clauses").arr) {
      auto ps = preds(*sides, &cl);
      sizes.push_back((int32_t) ps.size());
      all.insert(all.end(), ps.begin(), ps.end());
   }
   OwnedRel r(ctx);
   check(ldb_gpu_scan_filter_dnf(ctx, in, all.data(), sizes.data(), (int32_t) sizes.size(), r.out()), "filter_dnf");
   putRel(st.s("out"), r, *sides);
}

void Interp::stepJoinBuild(const J& st) {
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto keys = cols(*sides, st.at("keys"), "join_build");
   Value& src = val(st.s("in"));
   if (src.kind == Value::TABLE && st.bOr("unique", false) && st.bOr("index", true)) {
      // a bare base table keyed by its primary key: the table's own (persistent) hash index — the reference's index
      // nested-loop join over LingoDBHashIndex (translateINLJ); built once, reused by every later plan run
      std::vector<int32_t> cs;
      for (auto& k : keys) cs.push_back(k.col);
      Value v;
      v.kind = Value::HT;
      v.owned = false;
      v.sides = *sides;
      check(ldb_gpu_table_index(ctx, const_cast<ldb_table*>(src.table), cs.data(), (int32_t) cs.size(), &v.ht), "join_build (table index)");
      put(st.s("out"), std::move(v));
   } else {
      OwnedHt ht(ctx);
      check(ldb_gpu_join_build(ctx, in, keys.data(), (int32_t) keys.size(), st.bOr("unique", false) ? 1 : 0, ht.out()), "join_build");
      putHt(st.s("out"), ht, *sides);
   }
}

// EXISTS (probe rows) AND NOT EXISTS (probe rows that also pass `anti_preds`) for every build row, one pass over the probe side
// (Q21; the reference lowers the two subqueries to two marker joins, translateHJWithMarker)
void Interp::probeSemiAntiBuild(const J& st, Value& ht, ldb_rel* in, const Sides& sides, const std::vector<ldb_colref>& keys) {
   auto resid = residuals(st, sides, ht.sides, "residual probe", "residual build");
   auto ap = preds(sides, &st.at("anti_preds"));
   OwnedRel r(ctx);
   check(ldb_gpu_join_probe_semi_anti_build(ctx, ht.ht, in, keys.data(), (int32_t) keys.size(), resid.data(), (int32_t) resid.size(), ap.data(), (int32_t) ap.size(), r.out()), "join_probe (semi + anti, build side)");
   putRel(st.s("out"), r, ht.sides);
}

void Interp::stepJoinProbe(const J& st) {
   Value& ht = val(st.s("ht"));
   if (ht.kind != Value::HT) throw std::runtime_error("join_probe: 'ht' is not a hash table");
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto keys = cols(*sides, st.at("keys"), "join_probe");
   if (st.sOr("kind", "inner") == "semi_anti_build") return probeSemiAntiBuild(st, ht, in, *sides, keys);
   const JoinKind& jk = joinKindOf(kProbeKinds, st.sOr("kind", "inner"), "join_probe: unknown kind");
   const int32_t kind = jk.kind;
   auto resid = residuals(st, *sides, ht.sides, "residual probe", "residual build");
   // an INNER join takes any number of residual conjuncts (round 6): the probe kernel checks the first two on the candidate pair, the rest are
   // column-vs-column comparisons over the joined rows — for an inner join the same rows (the reference evaluates the whole non-equality part of
   // the predicate as the filter behind the lookup, SpecializeSubOpPass.cpp:152-205).  The other kinds decide per PROBE row and keep the limit
   std::vector<ldb_filter_desc> later;
   if (kind == LDB_JOIN_INNER && resid.size() > (size_t) kMaxResidual) {
      for (size_t k = (size_t) kMaxResidual; k < resid.size(); k++) {
         const ldb_join_residual& x = resid[k];
         ldb_filter_desc d;
         memset(&d, 0, sizeof(d));
         d.col = x.probe_col;
         d.op = x.op;
         d.rhs_kind = LDB_RHS_COLUMN;
         d.rhs_col = {(int32_t) (x.build_col.side + (int32_t) sides->size()), x.build_col.col}; // (the result's sides: probe sides, then build sides)
         later.push_back(d);
      }
      resid.resize((size_t) kMaxResidual);
   }
   OwnedTable mark(ctx); // (before r: a relation zipped with the mark column goes first)
   OwnedRel r(ctx);
   check(ldb_gpu_join_probe_residual(ctx, ht.ht, in, keys.data(), (int32_t) keys.size(), kind, resid.data(), (int32_t) resid.size(), r.out(), mark.out()), "join_probe");
   filterInChunks(nullptr, r, later, false, "join_probe (further residual conjuncts)", "join_probe (intermediate)");
   std::vector<const ldb_table*> outSides = joinOutSides(jk, *sides, ht.sides);
   if (mark.get() && st.get("mark_as")) { // the mark column as a column of the result relation (MarkJoinLowering: the stream carries the mark attribute)
      ldb_gpu_table_rename_col(mark.get(), 0, st.s("mark_as").c_str());
      OwnedRel z(ctx);
      check(ldb_gpu_rel_zip(ctx, r.get(), mark.get(), z.out()), "join_probe (mark column)");
      outSides.push_back(mark.get());
      r.reset(z.release());
   }
   putRel(st.s("out"), r, std::move(outSides));
   if (mark.get()) {
      if (const J* mo = st.get("mark_out")) putTable(mo->str, mark);
      else hide(mark);
   }
}

void Interp::stepJoinNl(const J& st) { // translateNLJ: no key equality, the predicate is the residual conjuncts (small build sides)
   std::vector<const ldb_table*>*sides, *bsides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   ldb_rel* build = relOf(st.s("build"), &bsides);
   const JoinKind& jk = joinKindOf(kNlKinds, st.sOr("kind", "inner"), "join_nl: unknown kind");
   auto resid = residuals(st, *sides, *bsides, "join_nl probe column", "join_nl build column");
   OwnedRel r(ctx);
   check(ldb_gpu_join_nl(ctx, in, build, jk.kind, resid.data(), (int32_t) resid.size(), r.out(), nullptr), "join_nl");
   putRel(st.s("out"), r, joinOutSides(jk, *sides, *bsides));
}

// one entry of a group-by's "aggs": {"fn", "expr", "as", "when", "count", "type"}
ldb_agg_spec Interp::aggSpec(const Sides& sides, const J& ja) {
   ldb_agg_spec a;
   memset(&a, 0, sizeof(a));
   const std::string fn = ja.s("fn");
   if (const J* when = ja.get("when")) { // sum(case when <conjunction> then x else 0 end)
      auto wp = preds(sides, when);
      if (wp.size() > LDB_MAX_AGG_PREDS) throw std::runtime_error("groupby: more than 3 conjuncts in a conditional aggregate");
      a.n_preds = (int32_t) wp.size();
      for (size_t p = 0; p < wp.size(); p++) a.preds[p] = wp[p];
   }
   if (fn == "count_star") {
      a.fn = LDB_AGG_COUNT_STAR;
      a.out_type = LDB_T_INT64;
      return a;
   }
   // min / max over a utf8 column: the bare column name, a utf8 result (bytewise order, StringRuntime::compareLt / compareGt)
   const J& je = ja.at("expr");
   __int128 litv;
   Scalar litt;
   const bool strArg = je.kind == J::STR && !decimalLiteral(je.str, &litv, &litt) && typeOf(sides, resolve(sides, je.str, "aggregate")).type == LDB_T_UTF8;
   if (strArg) {
      if (fn != "min" && fn != "max") throw std::runtime_error("groupby: '" + fn + "' over the string column '" + je.str + "' (only min / max)");
      if (a.n_preds) throw std::runtime_error("groupby: conditional " + fn + " over the string column '" + je.str + "' is not supported");
      a.fn = fn == "min" ? LDB_AGG_MIN : LDB_AGG_MAX;
      a.arg.n_terms = 1;
      a.arg.t[0].n_factors = 1;
      a.arg.t[0].f[0] = {1, resolve(sides, je.str, "aggregate"), 0, 1};
      a.out_type = LDB_T_UTF8;
      return a;
   }
   const Scalar t = aggExpr(sides, ja.at("expr"), &a.arg);
   if (const J* cnt = ja.get("count")) { // AVG over exchanged partials: SUM(expr) / SUM(count) — the merge of (sum, count) pairs
      if (fn != "avg") throw std::runtime_error("groupby: 'count' belongs to fn avg");
      a.has_count_expr = 1;
      aggExpr(sides, *cnt, &a.count_expr);
   }
   if (fn == "count") {
      a.fn = LDB_AGG_COUNT;
      a.out_type = LDB_T_INT64;
      return a;
   }
   static const std::map<std::string, int32_t> fns = {{"sum", LDB_AGG_SUM}, {"min", LDB_AGG_MIN}, {"max", LDB_AGG_MAX}, {"any", LDB_AGG_ANY}, {"avg", LDB_AGG_AVG}};
   auto fit = fns.find(fn);
   if (fit == fns.end()) throw std::runtime_error("groupby: unknown aggregate '" + fn + "'");
   a.fn = fit->second;
   if (t.kind == Scalar::DEC) { // SUM / MIN / MAX keep the argument type (sql_analyzer.cpp:2631-2632)
      DecimalType dt{t.p, t.s};
      a.wide = dt.wide();
      a.out_type = LDB_T_DECIMAL128;
      a.out_precision = dt.p;
      a.out_scale = dt.s;
      if (a.fn == LDB_AGG_AVG) { // SUM / COUNT with the divisor typed decimal(19,0) (:2636-2642)
         const DecimalType r = avgType(dt);
         a.avg_pow10 = r.s - dt.s;
         a.out_precision = r.p;
         a.out_scale = r.s;
      }
   } else if (t.kind == Scalar::DATE) {
      a.out_type = LDB_T_DATE32;
   } else {
      a.out_type = ja.sOr("type", "int64") == "int32" ? LDB_T_INT32 : LDB_T_INT64;
      if (a.fn == LDB_AGG_AVG) throw std::runtime_error("groupby: avg over integers is not supported (cast to decimal)");
   }
   return a;
}

// expected number of groups (sizes the hash table; a low estimate costs a retry, never a wrong result):
// a number, "est_groups_from": "rows" (the input's row count), or {"rows_of": value, "div": d, "min": m};
// without one, what the prepared plan's previous execution produced (*learn: this execution records it)
int64_t Interp::groupEstimate(const J& st, ldb_rel* in, bool hasKeys, bool* learn) {
   int64_t est = 0;
   if (const J* eg = st.get("est_groups")) {
      if (eg->kind == J::OBJ) {
         est = rowsOf(eg->s("rows_of")) / std::max<int64_t>(1, eg->iOr("div", 1));
         est = std::max<int64_t>(est, eg->iOr("min", 1));
      } else {
         est = eg->inum;
      }
   }
   if (st.sOr("est_groups_from", "") == "rows") est = std::max<int64_t>(1, ldb_gpu_rel_rows(ctx, in));
   *learn = est == 0 && groupsSeen && hasKeys;
   if (*learn) {
      auto seen = groupsSeen->find(st.s("out"));
      if (seen != groupsSeen->end()) est = std::max<int64_t>(1, seen->second);
   }
   return est;
}

void Interp::stepGroupby(const J& st) {
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto ps = preds(*sides, st.get("preds"));
   std::vector<ldb_colref> keys;
   if (const J* k = st.get("keys")) keys = cols(*sides, *k, "groupby key");
   std::vector<ldb_agg_spec> aggs;
   std::vector<std::string> names;
   for (auto& ja : st.at("aggs").arr) {
      const ldb_agg_spec a = aggSpec(*sides, ja);
      aggs.push_back(a);
      names.push_back(ja.sOr("as", ""));
   }
   bool learn = false;
   const int64_t est = groupEstimate(st, in, !keys.empty(), &learn);
   OwnedTable out(ctx);
   check(ldb_gpu_groupby(ctx, in, ps.data(), (int32_t) ps.size(), keys.data(), (int32_t) keys.size(), aggs.data(), (int32_t) aggs.size(), est, out.out()), "groupby");
   if (learn) (*groupsSeen)[st.s("out")] = ldb_gpu_table_rows(out.get());
   for (size_t a = 0; a < names.size(); a++)
      if (!names[a].empty()) ldb_gpu_table_rename_col(out.get(), (int32_t) (keys.size() + a), names[a].c_str());
   if (const J* kn = st.get("key_names"))
      for (size_t k = 0; k < kn->arr.size() && k < keys.size(); k++) ldb_gpu_table_rename_col(out.get(), (int32_t) k, kn->arr[k].str.c_str());
   putTable(st.s("out"), out);
}

// ---- map: the `fn` forms.  Each makes the computed column `as` over `in`
ldb_table* Interp::mapExtractYear(const J& st, ldb_rel* in, const Sides& sides) {
   ldb_table* t = nullptr;
   check(ldb_gpu_map_column(ctx, in, resolve(sides, st.s("col"), "map"), LDB_FN_EXTRACT_YEAR, st.s("as").c_str(), &t), "map extract_year");
   return t;
}
ldb_table* Interp::mapDatefn(const J& st, ldb_rel* in, const Sides& sides) { // Extract…FromDate / DateTrunc / DateAdd, DateSubtract (months)
   const std::string& fn = st.s("fn");
   const int32_t f = fn == "extract" ? LDB_DF_EXTRACT : fn == "date_trunc" ? LDB_DF_TRUNC : LDB_DF_ADD_MONTHS;
   int32_t part = 0;
   if (f != LDB_DF_ADD_MONTHS && (part = datepartOf(st.s("part"))) < 0) throw std::runtime_error("map " + fn + ": unknown part '" + st.s("part") + "'");
   ldb_colref mc = {0, 0};
   const bool perRow = f == LDB_DF_ADD_MONTHS && st.get("months_col");
   if (perRow) mc = resolve(sides, st.s("months_col"), "map add_months");
   ldb_table* t = nullptr;
   check(ldb_gpu_map_datefn(ctx, in, resolve(sides, st.s("col"), "map"), f, part, f == LDB_DF_ADD_MONTHS && !perRow ? st.iOr("months", 0) : 0, perRow ? &mc : nullptr, st.s("as").c_str(), &t), ("map " + fn).c_str());
   return t;
}
ldb_table* Interp::mapSubstr(const J& st, ldb_rel* in, const Sides& sides) {
   ldb_table* t = nullptr;
   check(ldb_gpu_map_substr(ctx, in, resolve(sides, st.s("col"), "map"), st.iOr("from", 1), st.iOr("for", 1 << 30), st.s("as").c_str(), &t), "map substr");
   return t;
}
ldb_table* Interp::mapCase(const J& st, ldb_rel* in, const Sides& sides) { // ToUpper / ToLower: one column part under a case mapping
   const std::string& fn = st.s("fn");
   ldb_strpart p = {LDB_SP_COL, fn == "upper" ? LDB_SC_UPPER : LDB_SC_LOWER, resolve(sides, st.s("col"), "map"), nullptr, 0, 1, LDB_STR_WHOLE};
   ldb_table* t = nullptr;
   check(ldb_gpu_map_strcat(ctx, in, &p, 1, st.s("as").c_str(), &t), ("map " + fn).c_str());
   return t;
}
ldb_table* Interp::mapLength(const J& st, ldb_rel* in, const Sides& sides) { // StringLength: UTF-8 characters
   ldb_table* t = nullptr;
   check(ldb_gpu_map_strlen(ctx, in, resolve(sides, st.s("col"), "map"), st.s("as").c_str(), &t), "map length");
   return t;
}
ldb_table* Interp::mapConcat(const J& st, ldb_rel* in, const Sides& sides) { // Concatenate (flattened): constants, columns (window, case mapping), integers / decimals / dates as text
   std::vector<ldb_strpart> ps;
   for (auto& e : st.at("parts").arr) {
      ldb_strpart p = {LDB_SP_CONST, LDB_SC_NONE, {0, 0}, nullptr, 0, 1, LDB_STR_WHOLE};
      if (const J* c = e.get("const")) {
         p.str = c->str.data(); // (the plan outlives the call)
         p.str_len = (int64_t) c->str.size();
      } else if (e.get("int")) {
         p.kind = LDB_SP_INT;
         p.col = resolve(sides, e.s("int"), "map concat");
      } else if (e.get("dec")) {
         p.kind = LDB_SP_DECIMAL;
         p.col = resolve(sides, e.s("dec"), "map concat");
      } else if (e.get("date")) {
         p.kind = LDB_SP_DATE;
         p.col = resolve(sides, e.s("date"), "map concat");
      } else {
         p.kind = LDB_SP_COL;
         p.col = resolve(sides, e.s("col"), "map concat");
         p.strcase = strcaseOf(e.sOr("case", "none"));
         p.from = e.iOr("from", 1);
         p.for_len = e.iOr("for", LDB_STR_WHOLE);
      }
      ps.push_back(p);
   }
   ldb_table* t = nullptr;
   check(ldb_gpu_map_strcat(ctx, in, ps.data(), (int32_t) ps.size(), st.s("as").c_str(), &t), "map concat");
   return t;
}
ldb_table* Interp::mapToVarchar(const J& st, ldb_rel* in, const Sides& sides) { // fromInt / fromDecimal / fromDate: a one-part concat whose kind follows the column's type
   ldb_strpart p = {LDB_SP_INT, LDB_SC_NONE, resolve(sides, st.s("col"), "map to_varchar"), nullptr, 0, 1, LDB_STR_WHOLE};
   ldb_coltype ct = {0, 0, 0, 0};
   ldb_gpu_table_coltype(sides[(size_t) p.col.side], p.col.col, &ct);
   if (ct.type == LDB_T_DECIMAL128) p.kind = LDB_SP_DECIMAL;
   else if (ct.type == LDB_T_DATE32) p.kind = LDB_SP_DATE;
   else if (ct.type != LDB_T_INT32 && ct.type != LDB_T_INT64)
      throw std::runtime_error("map to_varchar: column '" + st.s("col") + "' of type " + std::to_string(ct.type) + " (int32 / int64, decimal128 or date32 expected)");
   ldb_table* t = nullptr;
   check(ldb_gpu_map_strcat(ctx, in, &p, 1, st.s("as").c_str(), &t), "map to_varchar");
   return t;
}
ldb_table* Interp::mapParse(const J& st, ldb_rel* in, const Sides& sides) { // toInt / toDecimal / toDate
   const std::string& fn = st.s("fn");
   const int32_t kind = fn == "to_int" ? LDB_PARSE_INT64 : fn == "to_decimal" ? LDB_PARSE_DECIMAL : LDB_PARSE_DATE;
   const bool fail = st.sOr("on_error", "fail") == "fail"; // as the reference's throw; "null": bad rows are NULL, nothing is read back
   int64_t bad = 0;
   OwnedTable t(ctx);
   check(ldb_gpu_map_strparse(ctx, in, resolve(sides, st.s("col"), "map"), kind, (int32_t) st.iOr("precision", 0), (int32_t) st.iOr("scale", 0), st.s("as").c_str(), t.out(), fail ? &bad : nullptr),
         ("map " + fn).c_str());
   if (bad) throw std::runtime_error("map " + fn + ": " + std::to_string(bad) + " bad row" + (bad == 1 ? "" : "s") + " in column '" + st.s("col") + "' (on_error: \"null\" makes them NULL)");
   return t.release();
}
ldb_table* Interp::mapExpr(const J& st, ldb_rel* in, const Sides& sides) {
   XB b;
   const Scalar ty = compileX(sides, st.at("expr"), b);
   ldb_coltype ct = {LDB_T_INT64, 0, 0, 1};
   if (ty.kind == Scalar::DEC) ct = {LDB_T_DECIMAL128, ty.p, ty.s, 1};
   else if (ty.kind == Scalar::BOOL) ct = {LDB_T_BOOL8, 0, 0, 1};
   else if (ty.kind == Scalar::DATE) ct = {LDB_T_DATE32, 0, 0, 1};
   else if (ty.kind == Scalar::F32) ct = {LDB_T_FLOAT32, 0, 0, 1};
   else if (ty.kind == Scalar::F64) ct = {LDB_T_FLOAT64, 0, 0, 1};
   ldb_table* t = nullptr;
   check(ldb_gpu_map_expr(ctx, in, b.ins.data(), (int32_t) b.ins.size(), ct, st.s("as").c_str(), &t), "map expr");
   return t;
}

void Interp::stepMap(const J& st) { // subop.map: one computed column, attached as a new last side
   static const struct {
      const char* fn;
      ldb_table* (Interp::*make)(const J&, ldb_rel*, const Sides&);
   } forms[] = {{"extract_year", &Interp::mapExtractYear}, {"substr", &Interp::mapSubstr},       {"upper", &Interp::mapCase},      {"lower", &Interp::mapCase},
                {"length", &Interp::mapLength},            {"concat", &Interp::mapConcat},       {"to_varchar", &Interp::mapToVarchar},
                {"to_int", &Interp::mapParse},             {"to_decimal", &Interp::mapParse},    {"to_date", &Interp::mapParse},
                {"extract", &Interp::mapDatefn},           {"date_trunc", &Interp::mapDatefn},   {"add_months", &Interp::mapDatefn}};
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   (void) st.s("as");
   const std::string fn = st.sOr("fn", "");
   auto make = &Interp::mapExpr; // no fn, or none of the above: "expr"
   for (auto& f : forms)
      if (fn == f.fn) make = f.make;
   OwnedTable t(ctx, (this->*make)(st, in, *sides));
   ldb_table* col = t.get();
   hide(t);
   OwnedRel r(ctx);
   check(ldb_gpu_rel_zip(ctx, in, col, r.out()), "map zip");
   auto outSides = *sides;
   outSides.push_back(col);
   putRel(st.s("out"), r, std::move(outSides));
}

void Interp::stepSort(const J& st) { // sort and topk
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto specs = sortSpecs(*sides, st.at("by"), "sort");
   OwnedRel r(ctx);
   if (st.s("op") == "sort") check(ldb_gpu_sort(ctx, in, specs.data(), (int32_t) specs.size(), r.out()), "sort");
   else check(ldb_gpu_topk(ctx, in, specs.data(), (int32_t) specs.size(), st.at("k").inum, r.out()), "topk");
   putRel(st.s("out"), r, *sides);
}

void Interp::stepMaterialize(const J& st) { // MaterializeTableLowering: gather the listed columns
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto cs = cols(*sides, st.at("cols"), "materialize");
   OwnedTable t(ctx);
   check(ldb_gpu_materialize(ctx, in, cs.data(), (int32_t) cs.size(), t.out()), "materialize");
   renameCols(t.get(), st.at("cols"));
   putTable(st.s("out"), t);
}

void Interp::stepSetOp(const J& st) { // UnionAll / UnionDistinct / CountingSetOperation lowerings: two relations, column lists of pairwise equal types
   std::vector<const ldb_table*>*ls, *rs;
   ldb_rel* left = relOf(st.s("left"), &ls);
   ldb_rel* right = relOf(st.s("right"), &rs);
   auto lc = cols(*ls, st.at("left_cols"), "set_op (left)");
   auto rc = cols(*rs, st.at("right_cols"), "set_op (right)");
   if (lc.size() != rc.size() || lc.empty()) throw std::runtime_error("set_op: the two column lists must have the same, non-zero length");
   static const std::map<std::string, int32_t> kinds = {{"union_all", LDB_SET_UNION_ALL}, {"union", LDB_SET_UNION},   {"intersect", LDB_SET_INTERSECT},
                                                       {"intersect_all", LDB_SET_INTERSECT_ALL}, {"except", LDB_SET_EXCEPT}, {"except_all", LDB_SET_EXCEPT_ALL}};
   auto kit = kinds.find(st.s("kind"));
   if (kit == kinds.end()) throw std::runtime_error("set_op: unknown kind '" + st.s("kind") + "'");
   OwnedTable t(ctx);
   check(ldb_gpu_set_op(ctx, left, lc.data(), right, rc.data(), (int32_t) lc.size(), kit->second, t.out()), "set_op");
   if (const J* as = st.get("as"))
      for (size_t k = 0; k < as->arr.size() && k < lc.size(); k++) ldb_gpu_table_rename_col(t.get(), (int32_t) k, as->arr[k].str.c_str());
   putTable(st.s("out"), t);
}

// "frame_from" / "frame_to" of a window step: a row offset, or one of three names
static int64_t frameEnd(const J& st, const char* key, int64_t dflt) {
   const J* f = st.get(key);
   if (!f) return dflt;
   if (f->kind == J::STR) {
      if (f->str == "unbounded_preceding") return LDB_FRAME_UNBOUNDED_PRECEDING;
      if (f->str == "unbounded_following") return LDB_FRAME_UNBOUNDED_FOLLOWING;
      if (f->str == "current_row") return 0;
      throw std::runtime_error("window: frame end '" + f->str + "'");
   }
   return f->inum;
}

void Interp::stepWindow(const J& st) { // WindowLowering: partition + order, one frame for all functions; the function results are attached as new columns
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   std::vector<ldb_colref> part;
   if (const J* pk = st.get("partition_by")) part = cols(*sides, *pk, "window partition key");
   std::vector<ldb_sort_spec> order;
   if (const J* ob = st.get("order_by")) order = sortSpecs(*sides, *ob, "window order");
   const int64_t from = frameEnd(st, "frame_from", LDB_FRAME_UNBOUNDED_PRECEDING), to = frameEnd(st, "frame_to", 0);
   static const std::map<std::string, int32_t> fns = {{"rank", LDB_WIN_RANK}, {"sum", LDB_WIN_SUM}, {"min", LDB_WIN_MIN}, {"max", LDB_WIN_MAX}, {"count", LDB_WIN_COUNT}, {"count_star", LDB_WIN_COUNT_STAR}};
   std::vector<ldb_window_fn> wf;
   std::vector<std::string> names;
   for (auto& f : st.at("fns").arr) {
      auto fit = fns.find(f.s("fn"));
      if (fit == fns.end()) throw std::runtime_error("window: unknown function '" + f.s("fn") + "'");
      ldb_window_fn w;
      memset(&w, 0, sizeof(w));
      w.fn = fit->second;
      if (const J* c = f.get("col")) w.col = resolve(*sides, c->str, "window argument");
      wf.push_back(w);
      names.push_back(f.s("as"));
   }
   if (wf.empty()) throw std::runtime_error("window: no functions");
   OwnedTable t(ctx); // (before r and z: the relations over the function columns go first)
   OwnedRel r(ctx);
   check(ldb_gpu_window(ctx, in, part.data(), (int32_t) part.size(), order.data(), (int32_t) order.size(), from, to, wf.data(), (int32_t) wf.size(), r.out(), t.out()), "window");
   ldb_table* fcols = t.get();
   for (size_t k = 0; k < names.size(); k++) ldb_gpu_table_rename_col(fcols, (int32_t) k, names[k].c_str());
   hide(t);
   OwnedRel z(ctx);
   check(ldb_gpu_rel_zip(ctx, r.get(), fcols, z.out()), "window zip");
   r.reset();
   auto outSides = *sides;
   outSides.push_back(fcols);
   putRel(st.s("out"), z, std::move(outSides));
}

void Interp::stepAllgather(const J& st) { // every rank's rows of a (small) table, concatenated in rank order on every rank
   Value& t = val(st.s("in"));
   if (t.kind != Value::TABLE) throw std::runtime_error("allgather: 'in' must be a table (materialize first)");
   OwnedTable out(ctx);
   if (comm) {
      check(ldb_gpu_allgather(ctx, comm, t.table, st.s("out").c_str(), out.out()), "allgather");
   } else { // one rank: a copy
      std::vector<const ldb_table*>* sides;
      ldb_rel* in = relOf(st.s("in"), &sides);
      std::vector<ldb_colref> all;
      for (int32_t c = 0; c < ldb_gpu_table_cols(t.table); c++) all.push_back({0, c});
      check(ldb_gpu_materialize(ctx, in, all.data(), (int32_t) all.size(), out.out()), "allgather (one rank)");
   }
   putTable(st.s("out"), out);
}

void Interp::stepShuffle(const J& st) { // hash-radix re-partition on db.hash(keys): afterwards equal keys are on one rank
   std::vector<const ldb_table*>* sides;
   ldb_rel* in = relOf(st.s("in"), &sides);
   auto keys = cols(*sides, st.at("keys"), "shuffle key");
   auto cs = cols(*sides, st.at("cols"), "shuffle");
   OwnedTable out(ctx);
   if (comm) check(ldb_gpu_shuffle(ctx, comm, in, keys.data(), (int32_t) keys.size(), cs.data(), (int32_t) cs.size(), st.s("out").c_str(), out.out()), "shuffle");
   else check(ldb_gpu_materialize(ctx, in, cs.data(), (int32_t) cs.size(), out.out()), "shuffle (one rank)");
   renameCols(out.get(), st.at("cols"));
   putTable(st.s("out"), out);
}

// ------------------------------------------------------------ the step table
static const StepRow kSteps[] = {{"scan", {"table"}, {}, &Interp::stepScan},
                                 {"filter", {"in"}, {"preds"}, &Interp::stepFilter},
                                 {"filter_dnf", {"in"}, {"clauses"}, &Interp::stepFilterDnf},
                                 {"join_build", {"in"}, {"keys"}, &Interp::stepJoinBuild},
                                 {"join_probe", {"ht", "in"}, {"keys"}, &Interp::stepJoinProbe},
                                 {"groupby", {"in"}, {"aggs"}, &Interp::stepGroupby},
                                 {"map", {"in"}, {"as"}, &Interp::stepMap},
                                 {"sort", {"in"}, {"by"}, &Interp::stepSort},
                                 {"topk", {"in"}, {"by", "k"}, &Interp::stepSort},
                                 {"materialize", {"in"}, {"cols"}, &Interp::stepMaterialize},
                                 {"join_nl", {"in", "build"}, {}, &Interp::stepJoinNl},
                                 {"allgather", {"in"}, {}, &Interp::stepAllgather},
                                 {"shuffle", {"in"}, {"keys", "cols"}, &Interp::stepShuffle},
                                 {"nested_map", {"in", "scan"}, {}, &Interp::nestedMap},
                                 {"set_op", {"left", "right"}, {"left_cols", "right_cols", "kind"}, &Interp::stepSetOp},
                                 {"window", {"in"}, {"fns"}, &Interp::stepWindow},
                                 {"loop", {}, {}, &Interp::loop}}; // (the structure check gives a loop its own scope)
const StepRow* findStep(const std::string& op) {
   for (auto& row : kSteps)
      if (op == row.op) return &row;
   return nullptr;
}
void Interp::step(const J& st) {
   const StepRow* row = findStep(st.s("op"));
   if (!row) throw std::runtime_error("unknown step");
   (this->*row->fn)(st);
}

// ------------------------------------------------------------ nested_map / loop
static J jStr(const std::string& s) {
   J j;
   j.kind = J::STR;
   j.str = s;
   return j;
}
static J jObj(std::vector<std::pair<std::string, J>> fields) {
   J j;
   j.kind = J::OBJ;
   j.obj = std::move(fields);
   return j;
}
static J jArr(std::vector<J> items) {
   J j;
   j.kind = J::ARR;
   j.arr = std::move(items);
   return j;
}
// subop.nested_map (NestedMapLowering, SubOpToControlFlow.cpp:3996-4048): for every tuple of the outer stream the nested steps
// run with the tuple's columns as parameters — in kmeans.mlir / pagerank.mlir: scan a state, map over (outer tuple, scanned
// tuple), reduce into a per-tuple simple_state, scan that state.  On the device the correlation is removed: the outer tuples get
// their row number as identity, the nested scan becomes a nested-loop join (outer x scanned state, optional residual conjuncts),
// the nested maps run over the pairs, and the per-tuple state is a group-by on the identity.  Without "reduce" the pairs
// themselves are the result (the nested stream returned as it is).
//   {"op": "nested_map", "in": outer, "scan": inner, "residual": [...], "map": [{"as", "expr"} …],
//    "reduce": {"aggs": [...], "keep": [outer columns]}, "out": name}
void Interp::nestedMap(const J& st) {
   const std::string base = "__nm" + std::to_string(tmpCounter++) + "_";
   const std::string& out = st.s("out");
   const J* red = st.get("reduce");
   std::string cur = st.s("in");
   if (red) {
      step(jObj({{"op", jStr("map")}, {"in", jStr(cur)}, {"as", jStr("__tuple")}, {"expr", jObj({{"row_number", jArr({})}})}, {"out", jStr(base + "id")}}));
      cur = base + "id";
   }
   {
      std::vector<std::pair<std::string, J>> f = {{"op", jStr("join_nl")}, {"in", jStr(cur)}, {"build", jStr(st.s("scan"))}, {"kind", jStr("inner")}, {"out", jStr(base + "pairs")}};
      if (const J* rs = st.get("residual")) f.push_back({"residual", *rs});
      step(jObj(std::move(f)));
      cur = base + "pairs";
   }
   int k = 0;
   if (const J* maps = st.get("map"))
      for (auto& m : maps->arr) {
         const std::string nm = base + "m" + std::to_string(k++);
         step(jObj({{"op", jStr("map")}, {"in", jStr(cur)}, {"as", jStr(m.s("as"))}, {"expr", m.at("expr")}, {"out", jStr(nm)}}));
         cur = nm;
      }
   if (!red) { // the nested stream itself: the last value under the step's name
      put(out, env.find(cur)->second);
      env.erase(cur);
      return;
   }
   std::vector<J> aggs = red->at("aggs").arr;
   if (const J* keep = red->get("keep"))
      for (auto& c : keep->arr) aggs.push_back(jObj({{"fn", jStr("any")}, {"expr", jStr(c.str)}, {"as", jStr(c.str)}}));
   step(jObj({{"op", jStr("groupby")}, {"in", jStr(cur)}, {"keys", jArr({jStr("__tuple")})}, {"aggs", jArr(std::move(aggs))}, {"est_groups", jObj({{"rows_of", jStr(st.s("in"))}})}, {"out", jStr(out)}}));
}

// subop.loop (LoopLowering, SubOpToControlFlow.cpp:4058-4120: an scf.while over (condition, loop-carried states)): the body's
// steps run once per iteration with the loop variables bound to the current states; loop_continue names the condition (a member
// of a simple_state, here: column `col` of the one-row table `from`) and the states of the next iteration.  As in the
// reference the loop's results are the states handed to the LAST loop_continue (the one whose condition was false).
//   {"op": "loop", "vars": [{"name", "init"}], "body": [steps], "continue": {"from", "col"}, "next": [{"var", "from"}],
//    "results": [{"name", "var"}], "max_iterations": 1000}
// Loop-carried values are tables (materialised states: buffers, simple states, hash-map contents).
void Interp::loop(const J& st) {
   struct Var {
      std::string name, next, result;
      const ldb_table* cur; // the current state: the initial table, later what `own` holds
      OwnedTable own; // a state produced by an iteration belongs to the loop
   };
   std::vector<Var> vars;
   for (auto& jv : st.at("vars").arr) {
      Value& init = val(jv.s("init"));
      if (init.kind != Value::TABLE) throw std::runtime_error("loop: the initial value of '" + jv.s("name") + "' must be a table (materialize first)");
      vars.push_back(Var{jv.s("name"), "", "", init.table, OwnedTable(ctx)});
   }
   for (auto& jn : st.at("next").arr) {
      bool found = false;
      for (auto& v : vars)
         if (v.name == jn.s("var")) v.next = jn.s("from"), found = true;
      if (!found) throw std::runtime_error("loop: next names the unknown variable '" + jn.s("var") + "'");
   }
   for (auto& v : vars)
      if (v.next.empty()) throw std::runtime_error("loop: no next value for '" + v.name + "'");
   for (auto& jr : st.at("results").arr)
      for (auto& v : vars)
         if (v.name == jr.s("var")) v.result = jr.s("name");
   const J& body = st.at("body");
   const J& cont = st.at("continue");
   const int64_t maxIter = st.iOr("max_iterations", 1000);
   for (int64_t iter = 0;; iter++) {
      if (iter >= maxIter) throw std::runtime_error("loop: no fixpoint after " + std::to_string(maxIter) + " iterations");
      std::vector<std::string> before;
      for (auto& kv : env) before.push_back(kv.first);
      const size_t hiddenBefore = hidden.size();
      for (auto& v : vars) {
         Value b;
         b.kind = Value::TABLE;
         b.table = v.cur;
         b.owned = false; // the loop owns it
         put(v.name, std::move(b));
      }
      for (auto& s : body.arr) step(s);
      // the condition and the next states, read before the iteration's values go away
      bool again = false;
      if (rowsOf(cont.s("from")) >= 1 && !scalarIsNull(cont.s("from"), cont.s("col"))) again = readScalar(cont.s("from"), cont.s("col")) != 0;
      std::vector<const ldb_table*> nexts;
      for (auto& v : vars) { // (a table that an earlier variable takes is no longer the body's: the same refusal)
         Value& nv = val(v.next);
         if (nv.kind != Value::TABLE || !nv.owned || std::find(nexts.begin(), nexts.end(), nv.table) != nexts.end())
            throw std::runtime_error("loop: the next value '" + v.next + "' must be a table produced inside the body");
         nexts.push_back(nv.table);
      }
      // everything else the body defined dies with the iteration
      std::vector<std::string> mine;
      for (auto& kv : env)
         if (!std::binary_search(before.begin(), before.end(), kv.first)) mine.push_back(kv.first);
      for (auto& v : vars) val(v.next).owned = false; // taken over by the loop, only now that nothing can fail before the variables hold them
      releaseValues(&mine, hiddenBefore);
      for (size_t i = 0; i < vars.size(); i++) {
         vars[i].own.reset(const_cast<ldb_table*>(nexts[i]));
         vars[i].cur = nexts[i];
      }
      if (!again) break;
   }
   for (auto& v : vars) {
      if (v.result.empty()) v.own.reset();
      else putTable(v.result, v.own);
   }
}

} // namespace ldbplan

