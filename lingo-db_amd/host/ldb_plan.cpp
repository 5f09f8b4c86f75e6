// ldb_plan.cpp — plans as DATA: a JSON list of execution steps interpreted over the C-ABI.
//
// LingoDB hands a query to its backend as `subop.execution_step`s (one per pipeline,
// src/compiler/Dialect/SubOperator/Transforms/OrganizeExecutionStepsPass.cpp; walked by
// handleExecutionStepCPU, SubOpToControlFlow.cpp:4363-4395) and can dump them as JSON
// (tools/ct/mlir-subop-to-json.cpp: {"type":"execution_step","subops":[{"subop":"scan", …}]}).
// This file is the receiving end a GPU `ExecutionBackend` needs: a step list with the same
// vocabulary, at the granularity of the C-ABI (scan + filter, lookup + scan_list = join_probe,
// reduce + merge = groupby, …), each step's callbacks replaced by declarative descriptors.  The
// plan text is data — the TPC-H plans under lingo-db_amd/plans/ are JSON files, not C++ functions;
// INTEGRATION.md shows the LingoDB-side emitter that would produce the same documents.
//
// Column references are NAMES, resolved against the tables a relation was built from; constants
// are SQL literals typed against the column by the mirror of Restrictions::create; scalar
// expressions are trees typed by the reference's decimal rules (sql_analyzer.cpp:3058-3159) and
// compiled either into the aggregate normal form (ldb_expr) or into a postfix program (ldb_xinstr).
#include "ldb_plan_interp.hpp"
#include <algorithm>
#include <chrono>
#include <functional>

using namespace ldbplan;
using ldbjson::JParser;

namespace {
thread_local std::string g_plan_json_err;
} // namespace

// ================================================================== prepared plans
// A plan is static data, yet ldb_plan_run_json parses it, resolves every name and waits for the device after every
// operator whose output size decides the next allocation.  ldb_plan_prepare parses once; ldb_plan_execute brackets the
// interpretation with a read-back trace (lingodb_gpu.h, ldb_gpu_trace_*): the first execution over a set of input tables
// records every count the operators read back, the following ones — same tables (ldb_gpu_table_stamp), same options
// (ldb_gpu_option_epoch) — replay them, so that the whole plan is issued without one wait and checked once at the end.  A
// check that fails (LDB_TRACE_MISSED / LDB_ERR_RETRY: something the key does not cover changed) discards the execution and
// repeats it recording.  The descriptors of a repeated execution are byte-identical to the previous one's and are served
// from the context's descriptor cache (no upload).  Reference shape: the query is compiled once and run as one main()
// (src/execution/LLVMBackends.cpp:856-865), a pipeline never returns to the driver between its operators
// (SubOpToControlFlow.cpp:1123-1202).
struct ldb_plan {
   ldb_ctx* ctx = nullptr;
   J doc;
   ldb_trace* trace = nullptr;
   std::vector<uint64_t> key; // what the trace was recorded under: per input (stamp, rows), option epoch, exchange or not
   std::map<std::string, int64_t> groupsSeen; // Interp::groupsSeen
   int64_t executions = 0, replays = 0, misses = 0, peerMisses = 0; // peerMisses: executions repeated because ANOTHER rank's replay failed
   double issue_ms = 0, wait_ms = 0; // over the replayed executions: host time to issue the whole plan / time spent in the one wait at its end
};

namespace {
int32_t runParsed(ldb_ctx* ctx, ldb_comm* comm, const J& plan, const char* const* table_names, const ldb_table* const* tables, int32_t n_tables, ldb_table** result,
                  std::map<std::string, int64_t>* groupsSeen = nullptr) {
   try {
      Interp in(ctx);
      in.comm = comm;
      in.groupsSeen = groupsSeen;
      in.run(plan, table_names, tables, n_tables);
      *result = in.takeResult();
      return LDB_OK;
   } catch (const std::exception& e) { // (an operator that met a wrong replayed count fails with LDB_ERR_RETRY: the trace's end reports it)
      g_plan_json_err = e.what();
      return LDB_ERR_INVALID;
   }
}
} // namespace

// Run a JSON plan over the named input tables; *result = the table named by the plan's "result".
extern "C" int32_t ldb_plan_run_json(ldb_ctx* ctx, const char* plan_json, const char* const* table_names, const ldb_table* const* tables, int32_t n_tables, ldb_table** result) {
   return ldb_plan_run_json_comm(ctx, nullptr, plan_json, table_names, tables, n_tables, result);
}
// the same with a communicator: the plan's `allgather` / `shuffle` steps exchange rows with the other ranks
// (every rank runs the same plan text over its shard)
extern "C" int32_t ldb_plan_run_json_comm(ldb_ctx* ctx, ldb_comm* comm, const char* plan_json, const char* const* table_names, const ldb_table* const* tables, int32_t n_tables,
                                          ldb_table** result) {
   if (!ctx || !plan_json || !result || n_tables < 0) {
      g_plan_json_err = "plan_run_json: bad argument";
      return LDB_ERR_INVALID;
   }
   try {
      JParser parser(plan_json);
      const J plan = parser.value();
      // a one-off execution is bracketed like a prepared one (recording only): the context's counter arena restarts at the plan's
      // first operator, so that a text that is run again builds the descriptors the descriptor cache already holds
      ldb_trace* tr = nullptr;
      const bool bracket = ldb_gpu_trace_create(ctx, &tr) == LDB_OK && ldb_gpu_trace_begin(ctx, tr, 0) == LDB_OK;
      const int32_t st = runParsed(ctx, comm, plan, table_names, tables, n_tables, result);
      if (bracket) {
         int32_t status = 0;
         (void) ldb_gpu_trace_end(ctx, &status);
      }
      if (tr) ldb_gpu_trace_destroy(ctx, tr);
      return st;
   } catch (const std::exception& e) {
      g_plan_json_err = e.what();
      return LDB_ERR_INVALID;
   }
}
extern "C" int32_t ldb_plan_prepare(ldb_ctx* ctx, const char* plan_json, ldb_plan** out) {
   if (!ctx || !plan_json || !out) {
      g_plan_json_err = "plan_prepare: bad argument";
      return LDB_ERR_INVALID;
   }
   try {
      auto p = std::make_unique<ldb_plan>();
      p->ctx = ctx;
      JParser parser(plan_json);
      p->doc = parser.value();
      if (p->doc.kind != J::OBJ) throw std::runtime_error("plan: the top level must be an object");
      (void) p->doc.at("steps");
      if (ldb_gpu_trace_create(ctx, &p->trace) != LDB_OK) throw std::runtime_error(ldb_gpu_last_error());
      *out = p.release();
      return LDB_OK;
   } catch (const std::exception& e) {
      g_plan_json_err = e.what();
      return LDB_ERR_INVALID;
   }
}
extern "C" int32_t ldb_plan_release(ldb_plan* p) {
   if (!p) return LDB_OK;
   if (p->trace) ldb_gpu_trace_destroy(p->ctx, p->trace);
   delete p;
   return LDB_OK;
}
extern "C" int32_t ldb_plan_execute(ldb_plan* p, ldb_comm* comm, const char* const* table_names, const ldb_table* const* tables, int32_t n_tables, ldb_table** result) {
   if (!p || !result || n_tables < 0 || (n_tables && (!table_names || !tables))) {
      g_plan_json_err = "plan_execute: bad argument";
      return LDB_ERR_INVALID;
   }
   std::vector<uint64_t> key;
   for (int32_t i = 0; i < n_tables; i++) {
      key.push_back(ldb_gpu_table_stamp(tables[i]));
      key.push_back((uint64_t) ldb_gpu_table_rows(tables[i]));
   }
   key.push_back((uint64_t) ldb_gpu_option_epoch());
   key.push_back(comm ? 1 : 0);
   // replay only over the very inputs the trace was recorded on.  With a communicator the ranks replay TOGETHER or not at all (a replaying rank
   // queues its transfers with the recorded sizes, so its peers must do the same): they agree on the minimum of "I could replay" before the
   // execution and on the minimum of their verdicts after it; a miss on any rank makes every rank repeat the execution recording.  Two small
   // collectives per execution instead of a wait at every operator (ldb_gpu_comm_agree); the plan itself is issued without a host wait.
   bool replay = key == p->key;
   if (comm) {
      int32_t all = 0;
      if (ldb_gpu_comm_agree(p->ctx, comm, replay && ldb_gpu_trace_replayable(p->trace) ? 1 : 0, &all) != LDB_OK) {
         g_plan_json_err = ldb_gpu_last_error();
         return LDB_ERR_HIP;
      }
      replay = all == 1;
   }
   const int32_t collective = comm ? LDB_TRACE_COLLECTIVE : 0;
   for (int attempt = 0; attempt < 2; attempt++) {
      if (ldb_gpu_trace_begin(p->ctx, p->trace, (replay && attempt == 0 ? 1 : 0) | collective) != LDB_OK) {
         g_plan_json_err = ldb_gpu_last_error();
         return LDB_ERR_INVALID;
      }
      ldb_table* out = nullptr;
      const auto t0 = std::chrono::steady_clock::now();
      int32_t st = runParsed(p->ctx, comm, p->doc, table_names, tables, n_tables, &out, &p->groupsSeen);
      const auto t1 = std::chrono::steady_clock::now();
      int32_t status = LDB_TRACE_OFF;
      if (ldb_gpu_trace_end(p->ctx, &status) != LDB_OK) {
         if (out) ldb_gpu_table_release(p->ctx, out);
         g_plan_json_err = ldb_gpu_last_error();
         return LDB_ERR_HIP;
      }
      p->executions++;
      if (comm && replay && attempt == 0) { // did every rank's replay hold?  (only asked where a replay was attempted: all ranks take this branch together)
         int32_t all_ok = 0;
         if (ldb_gpu_comm_agree(p->ctx, comm, status == LDB_TRACE_MISSED ? 0 : 1, &all_ok) != LDB_OK) {
            if (out) ldb_gpu_table_release(p->ctx, out);
            g_plan_json_err = ldb_gpu_last_error();
            return LDB_ERR_HIP;
         }
         if (!all_ok && status != LDB_TRACE_MISSED) { // a peer mis-speculated: what it sent here is void too
            status = LDB_TRACE_MISSED;
            p->peerMisses++;
         }
      }
      if (status == LDB_TRACE_MISSED) { // a replayed count was wrong: everything computed from it is void
         if (out) ldb_gpu_table_release(p->ctx, out);
         p->misses++;
         p->key.clear();
         continue;
      }
      if (st != LDB_OK) {
         p->key.clear();
         return st;
      }
      if (status == LDB_TRACE_REPLAYED) {
         p->replays++;
         p->issue_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
         p->wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
      }
      p->key = key;
      *result = out;
      return LDB_OK;
   }
   g_plan_json_err = "plan_execute: the execution could not be completed after a failed replay";
   return LDB_ERR_INVALID;
}
extern "C" int32_t ldb_plan_times(const ldb_plan* p, double* issue_ms, double* wait_ms) {
   if (!p) return LDB_ERR_INVALID;
   if (issue_ms) *issue_ms = p->issue_ms;
   if (wait_ms) *wait_ms = p->wait_ms;
   return LDB_OK;
}
extern "C" int32_t ldb_plan_stats(const ldb_plan* p, int64_t* executions, int64_t* replays, int64_t* misses, int64_t* readbacks) {
   if (!p) return LDB_ERR_INVALID;
   if (executions) *executions = p->executions;
   if (replays) *replays = p->replays;
   if (misses) *misses = p->misses;
   if (readbacks) ldb_gpu_trace_stats(p->trace, readbacks, nullptr, nullptr, nullptr);
   return LDB_OK;
}
extern "C" const char* ldb_plan_json_last_error(void) { return g_plan_json_err.c_str(); }

// the `fn` forms of a map step: extract_year / substr / upper / lower / length / to_varchar over "col", to_int / to_decimal
// (with "precision" and "scale") / to_date over "col" with an optional "on_error", concat over "parts", extract / date_trunc
// over "col" with a "part", add_months over "col" with exactly one of "months" (a number) and "months_col"
static void checkMapFn(const J& st, const std::string& out) {
   const std::string& fn = st.s("fn");
   if (fn == "extract_year" || fn == "substr" || fn == "upper" || fn == "lower" || fn == "length" || fn == "to_varchar") {
      (void) st.s("col");
      return;
   }
   if (fn == "to_int" || fn == "to_decimal" || fn == "to_date") { // precision and scale belong to to_decimal, and it needs both
      const std::string where = "plan: map → '" + out + "': " + fn;
      (void) st.s("col");
      for (const char* f : {"precision", "scale"}) {
         const J* v = st.get(f);
         if (fn == "to_decimal" && (!v || v->kind != J::NUM)) throw std::runtime_error(where + " needs a number '" + f + "'");
         if (fn != "to_decimal" && v) throw std::runtime_error(where + " takes no '" + f + "' (to_decimal only)");
      }
      if (const J* oe = st.get("on_error"))
         if (oe->kind != J::STR || (oe->str != "fail" && oe->str != "null")) throw std::runtime_error(where + ": 'on_error' must be \"fail\" or \"null\"" + (oe->kind == J::STR ? ", not '" + oe->str + "'" : ""));
      return;
   }
   if (fn == "extract" || fn == "date_trunc" || fn == "add_months") {
      const std::string where = "plan: map → '" + out + "': " + fn;
      (void) st.s("col");
      if (fn == "add_months") {
         const J *m = st.get("months"), *mc = st.get("months_col");
         if (m && mc) throw std::runtime_error(where + " takes 'months' or 'months_col', not both");
         if (!m && !mc) throw std::runtime_error(where + " needs 'months' (a number) or 'months_col'");
         if (m && m->kind != J::NUM) throw std::runtime_error(where + ": 'months' must be a number");
         if (mc) (void) st.s("months_col");
         return;
      }
      const J* part = st.get("part");
      if (!part || part->kind != J::STR) throw std::runtime_error(where + " needs a 'part' (year, month, day, hour, minute, second)");
      if (datepartOf(part->str) < 0) throw std::runtime_error(where + ": unknown part '" + part->str + "' (year, month, day, hour, minute, second)");
      return;
   }
   if (fn != "concat") {
      if (!st.get("expr")) throw std::runtime_error("plan: map → '" + out + "': unknown fn '" + fn + "'");
      return;
   }
   const J* parts = st.get("parts");
   if (!parts || parts->kind != J::ARR) throw std::runtime_error("plan: map → '" + out + "': concat needs an array 'parts'");
   if (parts->arr.empty() || parts->arr.size() > LDB_MAX_STRPARTS)
      throw std::runtime_error("plan: map → '" + out + "': concat of " + std::to_string(parts->arr.size()) + " parts (1 to " + std::to_string(LDB_MAX_STRPARTS) + ")");
   size_t k = 0;
   for (auto& e : parts->arr) {
      const std::string where = "plan: map → '" + out + "': concat part " + std::to_string(k++);
      if (e.kind != J::OBJ) throw std::runtime_error(where + " must be an object");
      int given = 0;
      for (const char* f : {"const", "col", "int", "dec", "date"})
         if (e.get(f)) {
            given++;
            (void) e.s(f);
         }
      if (given != 1) throw std::runtime_error(where + " needs exactly one of 'const', 'col', 'int', 'dec', 'date'");
      if (const J* c = e.get("case")) {
         if (c->kind != J::STR) throw std::runtime_error(where + ": 'case' must be a string");
         (void) strcaseOf(c->str);
         if (!e.get("col") && c->str != "none") throw std::runtime_error(where + ": 'case' belongs to a 'col' part");
      }
      if ((e.get("from") || e.get("for")) && !e.get("col")) throw std::runtime_error(where + ": 'from' / 'for' belong to a 'col' part");
   }
}

// Device-less check of a plan's structure (what an emitter can verify before shipping a plan): the text
// parses, every step has a known "op" with its required fields, every value a step reads was named as an
// input or produced by an earlier step, no value is produced twice, and the result is produced by a step.
// Column names and types are only known at run time (ldb_plan_run_json).
extern "C" int32_t ldb_plan_json_check(const char* plan_json, const char* const* input_names, int32_t n_inputs) {
   if (!plan_json || n_inputs < 0) {
      g_plan_json_err = "plan_json_check: bad argument";
      return LDB_ERR_INVALID;
   }
   try {
      JParser parser(plan_json);
      const J plan = parser.value();
      if (plan.kind != J::OBJ) throw std::runtime_error("plan: the top level must be an object");
      std::map<std::string, bool> known; // name → produced by a step (false: an input)
      for (int32_t i = 0; i < n_inputs; i++) known[input_names[i]] = false;
      if (const J* in = plan.get("inputs"))
         for (auto& e : in->arr)
            if (!known.count(e.str)) {
               if (n_inputs > 0) throw std::runtime_error("plan: input '" + e.str + "' is not provided");
               known[e.str] = false;
            }
      const J& steps = plan.at("steps");
      if (steps.kind != J::ARR) throw std::runtime_error("plan: 'steps' must be an array");
      std::function<void(const J&, std::map<std::string, bool>&)> checkSteps = [&](const J& list, std::map<std::string, bool>& known) {
      for (auto& st : list.arr) {
         const std::string& op = st.s("op");
         const StepRow* sh = findStep(op); // the interpreter's own step table
         if (!sh) throw std::runtime_error("plan: unknown step '" + op + "'");
         if (op == "loop") { // variables bound from existing tables, a body with its own scope, results defined afterwards
            std::map<std::string, bool> inner = known;
            std::vector<std::string> vars;
            for (auto& v : st.at("vars").arr) {
               if (!known.count(v.s("init"))) throw std::runtime_error("plan: loop variable '" + v.s("name") + "' starts from '" + v.s("init") + "' before it exists");
               if (inner.count(v.s("name"))) throw std::runtime_error("plan: value '" + v.s("name") + "' defined twice");
               inner[v.s("name")] = true;
               vars.push_back(v.s("name"));
            }
            if (st.at("body").kind != J::ARR) throw std::runtime_error("plan: loop 'body' must be an array of steps");
            checkSteps(st.at("body"), inner);
            if (!inner.count(st.at("continue").s("from"))) throw std::runtime_error("plan: loop condition reads '" + st.at("continue").s("from") + "' before it exists");
            (void) st.at("continue").s("col");
            for (auto& n : st.at("next").arr) {
               if (std::find(vars.begin(), vars.end(), n.s("var")) == vars.end()) throw std::runtime_error("plan: loop 'next' names the unknown variable '" + n.s("var") + "'");
               auto it = inner.find(n.s("from"));
               if (it == inner.end() || known.count(n.s("from"))) throw std::runtime_error("plan: loop 'next' value '" + n.s("from") + "' is not produced by the body");
            }
            for (auto& r : st.at("results").arr) {
               if (std::find(vars.begin(), vars.end(), r.s("var")) == vars.end()) throw std::runtime_error("plan: loop result names the unknown variable '" + r.s("var") + "'");
               if (known.count(r.s("name"))) throw std::runtime_error("plan: value '" + r.s("name") + "' defined twice");
               known[r.s("name")] = true;
            }
            continue;
         }
         const std::string& out = st.s("out");
         for (const char* const* r = sh->reads; *r; r++)
            if (!known.count(st.s(*r))) throw std::runtime_error("plan: step '" + op + "' → '" + out + "' reads '" + st.s(*r) + "' before it exists");
         for (const char* const* f = sh->needs; *f; f++) (void) st.at(*f);
         if (op == "map" && !st.get("expr") && !st.get("fn")) throw std::runtime_error("plan: map → '" + out + "' needs 'expr' or 'fn'");
         if (op == "map" && st.get("fn")) checkMapFn(st, out);
         if (known.count(out)) throw std::runtime_error("plan: value '" + out + "' defined twice");
         known[out] = true;
         if (const J* mo = st.get("mark_out")) known[mo->str] = true;
      }
      };
      checkSteps(steps, known);
      const std::string result = plan.sOr("result", "result");
      auto it = known.find(result);
      if (it == known.end() || !it->second) throw std::runtime_error("plan: result '" + result + "' is not produced by a step");
      return LDB_OK;
   } catch (const std::exception& e) {
      g_plan_json_err = e.what();
      return LDB_ERR_INVALID;
   }
}
