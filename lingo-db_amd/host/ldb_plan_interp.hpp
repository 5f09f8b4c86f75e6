// ldb_plan_interp.hpp — what the parts of the plan interpreter share: ldb_plan.cpp (entry points, structure check),
// ldb_plan_expr.cpp (predicates and expressions), ldb_plan_steps.cpp (environment, steps, step table).
// Internal to libldb_host.so: everything here has hidden visibility.
#pragma once
#include "ldb_host.hpp"
#include "ldb_json.hpp"
#include <cstring>
#include <map>
#include <utility>

namespace ldbplan __attribute__((visibility("hidden"))) {
using namespace lingodb::runtime::gpu;
using ldbjson::J;

// a fresh handle between the C-ABI call that made it and the environment taking it over: released unless release() was called
template <class T, int32_t (*Release)(ldb_ctx*, T*)>
struct Owned {
   ldb_ctx* ctx;
   T* h;
   explicit Owned(ldb_ctx* c, T* p = nullptr) : ctx(c), h(p) {}
   Owned(Owned&& o) noexcept : ctx(o.ctx), h(o.release()) {}
   ~Owned() { reset(); } // (the move constructor makes it move-only)
   T* get() const { return h; }
   T** out() { return &h; } // for the C-ABI's out parameters
   T* release() { return std::exchange(h, nullptr); }
   int32_t reset(T* p = nullptr) { // releases what it held, then holds p; the status of the release
      const int32_t st = h ? Release(ctx, h) : LDB_OK;
      h = p;
      return st;
   }
};
using OwnedRel = Owned<ldb_rel, ldb_gpu_rel_release>;
using OwnedTable = Owned<ldb_table, ldb_gpu_table_release>;
using OwnedHt = Owned<ldb_hashtable, ldb_gpu_hashtable_release>;

// ================================================================== environment
struct Value {
   enum Kind { TABLE, REL, HT } kind = TABLE;
   const ldb_table* table = nullptr;
   ldb_rel* rel = nullptr;
   ldb_hashtable* ht = nullptr;
   bool owned = false;
   std::vector<const ldb_table*> sides; // REL: the table behind each side; HT: the sides of its build relation
   ldb_rel* lazyRel = nullptr; // TABLE used as a relation
};

struct Scalar { // expression type: integer (p = 0) or decimal(p, s), date, bool, f32 / f64
   enum Kind { INT, DEC, DATE, BOOL, F32, F64 } kind = INT;
   int32_t p = 0, s = 0;
   bool isFloat() const { return kind == F32 || kind == F64; }
};

struct XB { // postfix program under construction
   std::vector<ldb_xinstr> ins;
   void push(int32_t op, int32_t arg = 0, ldb_colref c = {0, 0}, __int128 k = 0) {
      ldb_xinstr x;
      memset(&x, 0, sizeof(x));
      x.op = op;
      x.arg = arg;
      x.col = c;
      x.lo = (int64_t) (uint64_t) k;
      x.hi = (int64_t) (k >> 64);
      ins.push_back(x);
   }
};

using Sides = std::vector<const ldb_table*>;

struct Interp {
   ldb_ctx* ctx;
   ldb_comm* comm = nullptr; // exchange steps: NULL = one rank (allgather is a copy, shuffle a materialize)
   std::map<std::string, Value> env;
   std::vector<ldb_table*> hidden; // computed-column tables that live as long as the plan run
   std::vector<std::unique_ptr<Restrictions>> keepRestr; // constant storage the descriptors point into
   std::vector<std::unique_ptr<std::string>> keepStr;
   std::string result;
   // a prepared plan remembers how many groups each group-by WITHOUT an estimate produced (by its `out` name): the next execution sizes the
   // table from that instead of paying an overflowing attempt again (plans translated from the reference's dumps carry no cardinalities)
   std::map<std::string, int64_t>* groupsSeen = nullptr;
   int tmpCounter = 0;
   explicit Interp(ldb_ctx* c) : ctx(c) {}
   ~Interp();
   void run(const J& plan, const char* const* names, const ldb_table* const* tables, int32_t n);
   ldb_table* takeResult(); // the result table, from now on the caller's: ~Interp skips exactly this table

   // ---- environment (ldb_plan_steps.cpp)
   void releaseValues(const std::vector<std::string>* names, size_t hiddenFrom); // names == nullptr: every value
   Value& val(const std::string& name);
   ldb_rel* relOf(const std::string& name, Sides** sides = nullptr);
   int64_t rowsOf(const std::string& name);
   void put(const std::string& name, Value v);
   void putRel(const std::string& name, OwnedRel& r, Sides sides);
   void putTable(const std::string& name, OwnedTable& t);
   void putHt(const std::string& name, OwnedHt& ht, Sides sides);
   void hide(OwnedTable& t);
   static ldb_colref resolve(const Sides& sides, const std::string& ref, const char* what);
   static ldb_coltype typeOf(const Sides& sides, ldb_colref c);

   // ---- predicates and expressions (ldb_plan_expr.cpp)
   static constexpr int kMaxInConstants = 8, kMaxConjuncts = 8, kMaxResidual = 2; // what one scan_filter call takes (LDB_MAX_IN / LDB_MAX_PREDS of the kernels' descriptors)
   static int32_t opOf(const std::string& op);
   __int128 readScalar(const std::string& table, const std::string& col);
   bool scalarIsNull(const std::string& table, const std::string& col);
   ldb_filter_desc pred(const Sides& sides, const J& jp);
   std::vector<ldb_filter_desc> preds(const Sides& sides, const J* list);
   ldb_rel* semiJoinConstants(ldb_rel* cur, const ldb_filter_desc& d, const Sides& sides, const std::string& stem);
   static bool decimalLiteral(const std::string& txt, __int128* v, Scalar* t);
   Scalar compileX(const Sides& sides, const J& e, XB& b);
   struct Factor;
   Factor factorOf(const Sides& sides, const J& e);
   Scalar termOf(const Sides& sides, const J& e, ldb_term* t);
   Scalar aggExpr(const Sides& sides, const J& e, ldb_expr* out);

   // ---- steps (ldb_plan_steps.cpp)
   void step(const J& st);
   void stepScan(const J& st);
   void stepFilter(const J& st);
   void stepFilterDnf(const J& st);
   void stepJoinBuild(const J& st);
   void stepJoinProbe(const J& st);
   void stepJoinNl(const J& st);
   void stepGroupby(const J& st);
   void stepMap(const J& st);
   void stepSort(const J& st); // sort and topk
   void stepMaterialize(const J& st);
   void stepSetOp(const J& st);
   void stepWindow(const J& st);
   void stepAllgather(const J& st);
   void stepShuffle(const J& st);
   void nestedMap(const J& st);
   void loop(const J& st);
   // pieces of the steps
   std::vector<ldb_colref> cols(const Sides& sides, const J& list, const char* what);
   std::vector<ldb_join_residual> residuals(const J& st, const Sides& probe, const Sides& build, const char* whatProbe, const char* whatBuild);
   std::vector<ldb_sort_spec> sortSpecs(const Sides& sides, const J& by, const char* what);
   void filterInChunks(ldb_rel* in, OwnedRel& cur, const std::vector<ldb_filter_desc>& fs, bool evenIfEmpty, const char* what, const char* whatRelease);
   void probeSemiAntiBuild(const J& st, Value& ht, ldb_rel* in, const Sides& sides, const std::vector<ldb_colref>& keys);
   ldb_agg_spec aggSpec(const Sides& sides, const J& ja);
   int64_t groupEstimate(const J& st, ldb_rel* in, bool hasKeys, bool* learn);
   // the `fn` forms of map: each returns the computed column
   ldb_table* mapExtractYear(const J& st, ldb_rel* in, const Sides& sides);
   ldb_table* mapDatefn(const J& st, ldb_rel* in, const Sides& sides); // extract, date_trunc, add_months
   ldb_table* mapSubstr(const J& st, ldb_rel* in, const Sides& sides);
   ldb_table* mapCase(const J& st, ldb_rel* in, const Sides& sides); // upper, lower
   ldb_table* mapLength(const J& st, ldb_rel* in, const Sides& sides);
   ldb_table* mapConcat(const J& st, ldb_rel* in, const Sides& sides);
   ldb_table* mapToVarchar(const J& st, ldb_rel* in, const Sides& sides);
   ldb_table* mapParse(const J& st, ldb_rel* in, const Sides& sides); // to_int, to_decimal, to_date
   ldb_table* mapExpr(const J& st, ldb_rel* in, const Sides& sides);
};

// one row per step of the plan language: the fields that name values the step reads, the fields it must have, and its function
struct StepRow {
   const char* op;
   const char* reads[3]; // (both lists end with a nullptr)
   const char* needs[4];
   void (Interp::*fn)(const J&);
};
const StepRow* findStep(const std::string& op); // nullptr: unknown step

int32_t strcaseOf(const std::string& c); // "case" of a concat part
int32_t datepartOf(const std::string& p); // "part" of extract / date_trunc and the unit of datediff as ldb_datepart, -1: unknown

} // namespace ldbplan
