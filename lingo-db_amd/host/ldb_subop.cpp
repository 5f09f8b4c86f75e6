// ldb_subop.cpp — consumer of the reference's OWN sub-operator dump.
//
// LingoDB's CPU backend walks `subop.execution_step`s (handleExecutionStepCPU, SubOpToControlFlow.cpp:4363-4395;
// the GPU stub handleExecutionStepGPU, :4512-4548, is where a device backend plugs in) and the repository ships a
// tool that prints exactly that IR as JSON: tools/ct/mlir-subop-to-json.cpp (`[{"type":"execution_step",
// "subops":[{"subop":"get_external","meta":{tableName,mapping,filters}}, {"subop":"scan","mapping":[…]}, …],
// "inputs","results","outerEdges","innerEdges"}]`, :434-560 and the sub-operator cases :560-850).  This file
// reads that document and pattern-matches the sub-operator sequences the reference's lowerings produce onto
// the C-ABI's operator-level steps (the step list ldb_plan.cpp interprets):
//
//   get_external + scan                         → a base table relation; meta.filters → restrictions
//   map                                         → column bindings (expressions are inlined into their consumers; runtime calls
//                                                 ExtractYearFromDate / Extract{Month … Second}FromDate / DateTrunc / Substring / ToUpper / ToLower / StringLength → map fn, a Concatenate
//                                                 nest → map fn concat with its parts, ConstLike → LIKE restrictions)
//   filter all_true                             → restrictions (conjunctions, IN, LIKE, DNF → filter_dnf, anything else → a computed
//                                                 boolean column + `= true`) / the conjuncts of a hash join (keys, residuals, post-join filters)
//   lookup(SimpleState) | lookup_or_insert(HashMap) + reduce [+ create_thread_local / merge]
//                                               → groupby (sum / count / count(*) / min / max / any, the nullable bodies; sum ÷ count → avg;
//                                                 an empty reduce → distinct)
//   materialize(Buffer) + create_hash_indexed_view + lookup(HashIndexedView) + nested_map{scan_list, gather,
//     combine_tuple, map, filter …}             → join_build + join_probe: inner; anyTuple + marker filter → semi / anti, read as a value →
//                                                 mark; flag member + scatter → semi_build / anti_build; + null / as-nullable maps + union →
//                                                 left_outer, right_outer (reverseSides), full_outer
//   create_simple_state + scatter / lookup + gather → the cross product with a one-row side (constant single join)
//   lookup(HashMap) + unwrap_optional_ref + … + reduce into another input's map → group join
//   two inputs counting into one map / two maps + union → set_op (UNION [ALL], INTERSECT [ALL], EXCEPT [ALL])
//   sorted / continuous / segment-tree views + scan_ref, frame references, entries_between, lookup(SegmentTreeView) → window
//   a buffer scanned inside a nested_map body   → join_nl
//   materialize(Buffer) + create_sorted_view    → sort          materialize(Heap) + scan → topk
//   materialize(ResultTable)                    → materialize (the query result)
// (INTEGRATION.md §1b has the table with the lowering each row comes from.)
//
// Everything else is reported per execution step as "cpu" with the reason (the reference would run such a step on
// its CPU backend; there is none here, so the translation as a whole fails with LDB_ERR_UNSUPPORTED and the report
// says which step).  The dump loses a few facts a backend needs; the consumer relies on small emitter additions, listed in
// INTEGRATION.md §1b and in tools/write_subop_dumps.py / tools/subop_lower.py (E1 " - " for db.sub, E4 sortBy / maxRows on
// create_sorted_view / create_heap, E5 primaryKey, E6 combine_tuple, E7 the arith.* ops of the nullable aggregate bodies / set-operation
// counters / rank, E8 the aggregates of create_segment_tree_view and the keys of lookup, E9 the materialize inside the reduce that
// fills a window partition's buffer).  Group-by keys need no
// extension: performAggregation names key members "keyval$n" and the later scan of the map re-defines the SAME
// columns (RelAlgToSubOp.cpp:2158-2166, test/lit/RelAlg/lowering.mlir:37), so keys are read off that scan.
#include "ldb_subop_translate.hpp"
#include <cstring>

namespace ldbsubop {

// ------------------------------------------------------------------ the sub-operator table
static const OpRow kOps[] = {{"get_external", &Translator::opGetExternal},
                             {"create_thread_local", &Translator::opCreateState},
                             {"create_simple_state", &Translator::opCreateState},
                             {"generic_create", &Translator::opCreateState},
                             {"create_array", &Translator::opCreateState},
                             {"create_from", &Translator::opCreateState},
                             {"create_heap", &Translator::opCreateHeap},
                             {"merge", &Translator::opMerge},
                             {"create_hash_indexed_view", &Translator::opCreateHashIndexedView},
                             {"create_sorted_view", &Translator::opCreateSortedView},
                             {"create_continuous_view", &Translator::opCreateContinuousView},
                             {"create_segment_tree_view", &Translator::opCreateSegmentTreeView},
                             {"scan_ref", &Translator::opScanRef},
                             {"get_begin_reference", &Translator::opFrameReference},
                             {"get_end_reference", &Translator::opFrameReference},
                             {"offset_reference_by", &Translator::opOffsetReferenceBy},
                             {"entries_between", &Translator::opEntriesBetween},
                             {"scan", &Translator::opScan},
                             {"nested_map", &Translator::opNestedMap},
                             {"scan_list", &Translator::opScanList},
                             {"unwrap_optional_ref", &Translator::opUnwrapOptionalRef},
                             {"gather", &Translator::opGather},
                             {"combine_tuple", &Translator::opCombineTuple},
                             {"renaming", &Translator::opRenaming},
                             {"map", &Translator::opMap},
                             {"filter", &Translator::opFilter},
                             {"union", &Translator::opUnion},
                             {"lookup", &Translator::opLookup},
                             {"lookup_or_insert", &Translator::opLookup},
                             {"reduce", &Translator::opReduce},
                             {"materialize", &Translator::opMaterialize},
                             {"scatter", &Translator::opScatter}};
const OpRow* findOp(const std::string& subop) {
   for (auto& row : kOps)
      if (subop == row.subop) return &row;
   return nullptr;
}
void Translator::handle(const J& op, StepCtx& c) {
   const J* kind = op.get("subop");
   if (!kind) throw Unsupported("a sub-operator the dump tool has no case for (\"operator\": \"unknown\")");
   const std::string& ref = op.s("ref");
   const OpRow* row = findOp(kind->str);
   if (!row) throw Unsupported("sub-operator '" + kind->str + "' has no device pattern");
   (this->*row->fn)(op, ref, c);
}

// ------------------------------------------------------------------ states and streams of one execution step
StateP Translator::newState(State::Kind k, const std::string& ref, StepCtx& c) {
   auto s = std::make_shared<State>();
   s->kind = k;
   c.local[stateKey(ref, 0)] = s;
   return s;
}
StateP Translator::resolve(const J& acc, StepCtx& c) {
   const std::string& t = acc.s("type");
   if (t == "parentArg") {
      const int64_t n = acc.iOr("argnr", -1);
      if (n < 0 || (size_t) n >= c.args.size() || !c.args[(size_t) n]) throw Unsupported("state argument " + std::to_string(n) + " is not available");
      return c.args[(size_t) n];
   }
   if (t == "node") {
      const std::string id = stateKey(acc);
      auto it = c.local.find(id);
      if (it != c.local.end()) return it->second;
      auto jt = states.find(id);
      if (jt != states.end()) return jt->second;
      throw Unsupported("state '" + id + "' is produced by a sub-operator this consumer does not know");
   }
   if (t == "nested_map_arg" && c.nested && !c.nested->partState.empty()) return states.at(c.nested->partState); // the per-partition buffer of a window
   throw Unsupported("state access of type '" + t + "'");
}
Stream& Translator::input(const J& op, StepCtx& c) {
   for (auto& e : op.at("outerEdges").arr)
      if (e.s("type") == "stream") {
         auto it = c.streams.find(e.at("input").s("ref"));
         if (it == c.streams.end()) throw Unsupported("stream input '" + e.at("input").s("ref") + "' is not produced in this step");
         return it->second;
      }
   if (c.nested) return *c.nested;
   throw Unsupported("sub-operator without a stream input");
}
std::string Translator::idOf(const StateP& st, StepCtx& c) {
   for (auto& kv : states)
      if (kv.second == st) return kv.first;
   for (auto& kv : c.local)
      if (kv.second == st) {
         states[kv.first] = st;
         return kv.first;
      }
   throw Unsupported("state without an identity");
}

void Translator::opGetExternal(const J& op, const std::string& ref, StepCtx& c) {
   const J& meta = op.at("meta");
   StateP s = newState(State::TABLE, ref, c);
   s->table = meta.s("tableName");
   inputs.insert(s->table);
   for (auto& m : meta.at("mapping").arr) s->memberToIdent[m.s("memberName")] = m.s("identifier");
   if (const J* fs = meta.get("filters"))
      for (auto& f : fs->arr) {
         const std::string& fop = f.s("op");
         if (fop == "UNKNOWN") throw Unsupported("restriction with an unknown FilterOp");
         s->filters.push_back(predJson(f.s("columnName"), fop, f.get("value"), f.get("values")));
      }
   if (const J* pk = meta.get("primaryKey")) // emitter extension E5
      for (auto& k : pk->arr) s->pkey.push_back(k.str);
   if (meta.get("index")) throw Unsupported("get_external over an external hash index");
}
void Translator::opCreateState(const J&, const std::string& ref, StepCtx& c) {
   newState(State::UNKNOWN, ref, c);
}
void Translator::opCreateHeap(const J& op, const std::string& ref, StepCtx& c) {
   StateP s = newState(State::HEAP, ref, c);
   s->maxRows = op.iOr("maxRows", -1); // emitter extension E4
   if (const J* sb = op.get("sortBy"))
      for (auto& k : sb->arr) s->sortBy.push_back({k.s("member"), k.sOr("direction", "asc") == "desc"});
   if (s->maxRows < 0 || s->sortBy.empty()) throw Unsupported("create_heap without maxRows / sortBy (emitter extension E4)");
}
void Translator::opMerge(const J& op, const std::string& ref, StepCtx& c) { // the thread-local instances merged into one state: there is one state on a GPU (a thread-local step input is the state itself)
   c.local[stateKey(ref, 0)] = resolve(op.at("accesses").arr.at(0), c);
}
void Translator::opCreateHashIndexedView(const J& op, const std::string& ref, StepCtx& c) {
   StateP src = resolve(op.at("accesses").arr.at(0), c);
   if (src->kind != State::BUFFER) throw Unsupported("hash-indexed view over a state that is not a materialised buffer");
   StateP s = newState(State::HIV, ref, c);
   s->source = src;
}
void Translator::opCreateSortedView(const J& op, const std::string& ref, StepCtx& c) {
   StateP src = resolve(op.at("accesses").arr.at(0), c);
   if (src->kind != State::BUFFER) throw Unsupported("sorted view over a state that is not a materialised buffer");
   const J* sb = op.get("sortBy"); // emitter extension E4
   if (!sb || sb->arr.empty()) throw Unsupported("create_sorted_view without sortBy (emitter extension E4)");
   StateP s = newState(State::SORTED, ref, c);
   s->source = src;
   s->in = src->in;
   s->members = src->members;
   if (!src->partPending) flush(s->in);
   std::vector<std::string> by;
   for (auto& key : sb->arr) {
      auto it = s->members.find(key.s("member"));
      if (it == s->members.end()) throw Unsupported("sort key '" + key.s("member") + "' is not a member of the buffer");
      const std::string col = ensureCol(s->in, it->second, stripSuffix(it->first));
      it->second = mk(Expr::COL, col);
      s->sortCols.push_back({col, key.sOr("direction", "asc") == "desc"});
      by.push_back(sortKey(col, s->sortCols.back().second));
   }
   s->partCols = src->partCols;
   if (src->partPending) { // one partition's buffer of a window: the window step orders the rows inside their partitions itself
      if (s->in.rel != src->in.rel) throw Unsupported("window ordered by a computed column inside a partition");
      return;
   }
   s->in.rel = emit("sort", "s", {{"in", quote(s->in.rel)}, {"by", joined(by)}});
}
void Translator::opCreateContinuousView(const J& op, const std::string& ref, StepCtx& c) { // the rows of a (sorted) buffer addressable by position: the input of a window evaluation
   StateP src = resolve(op.at("accesses").arr.at(0), c);
   if (src->kind != State::SORTED && src->kind != State::BUFFER) throw Unsupported("continuous view over a state that is neither a buffer nor a sorted view");
   StateP v = newState(State::CONTVIEW, ref, c);
   v->source = src;
   v->in = src->in;
   v->members = src->members;
   v->sortCols = src->sortCols;
   v->partCols = src->partCols;
}
void Translator::opCreateSegmentTreeView(const J& op, const std::string& ref, StepCtx& c) {
   StateP src = resolve(op.at("accesses").arr.at(0), c);
   if (src->kind != State::CONTVIEW) throw Unsupported("segment tree over a state that is not a continuous view");
   const J* ag = op.get("aggregates"); // emitter extension E8: the tool prints neither the functions nor their source members
   if (!ag || ag->arr.empty()) throw Unsupported("create_segment_tree_view without its aggregates (emitter extension E8)");
   StateP t = newState(State::SEGTREE, ref, c);
   t->source = src;
   for (auto& a : ag->arr) t->winAggs.push_back({a.s("member"), a.s("fn"), a.sOr("source", "")});
}

void Translator::addReport(const std::string& ref, bool gpu, const std::string& reason, size_t nSubops) {
   if (!report.empty()) report += ", ";
   report += "{\"ref\": " + quote(ref) + ", \"subops\": " + std::to_string(nSubops) + ", \"target\": " + (gpu ? "\"gpu\"" : "\"cpu\"") + (reason.empty() ? "" : ", \"reason\": " + quote(reason)) + "}";
}

bool Translator::run(const J& plan, std::string* err) {
   if (plan.kind != J::ARR) throw std::runtime_error("subop dump: the document must be the array ToJson::run prints");
   // the manifest of the patched emitter (integration/mlir-subop-to-json.patch, --gpu-manifest): which of the extensions E1 … E10 produced this
   // document.  A dump without one comes from the unpatched tool, whose output this consumer would MIS-translate silently in two places (db.sub
   // printed as " + ", db.between without its inclusivity flags) — refused as a whole
   bool manifest = false;
   for (auto& node : plan.arr)
      if (node.kind == J::OBJ && node.sOr("type", "") == "emitter_manifest") {
         manifest = true;
         if (const J* x = node.get("extensions"))
            for (auto& v : x->arr) ext.insert(v.str);
      }
   if (!manifest) {
      *err = "the dump carries no emitter manifest ({\"type\": \"emitter_manifest\", \"extensions\": [...]}, written by the patched tool: "
             "integration/mlir-subop-to-json.patch): the unpatched mlir-subop-to-json prints db.sub as ' + ' (needs E1) and drops the inclusivity flags of "
             "db.between (needs E10) — refusing the document instead of mis-translating it";
      addReport("", false, *err, 0);
      return false;
   }
   bool ok = true;
   for (auto& node : plan.arr) {
      if (node.sOr("type", "") == "emitter_manifest") continue;
      const std::string& ref = node.s("ref");
      StepCtx c;
      const bool isStep = node.sOr("type", "") == "execution_step";
      size_t nSub = isStep ? node.at("subops").arr.size() : 1;
      if (!ok) { // after the first unsupported step nothing downstream can be placed
         addReport(ref, false, "depends on a step that stays on the CPU", nSub);
         continue;
      }
      try {
         if (isStep) {
            for (auto& e : node.at("outerEdges").arr) {
               if (e.s("type") != "requiredInput") continue;
               const std::string id = stateKey(e.at("input"));
               const size_t argnr = (size_t) e.at("output").iOr("argnr", 0);
               if (c.args.size() <= argnr) c.args.resize(argnr + 1);
               auto it = states.find(id);
               c.args[argnr] = it == states.end() ? nullptr : it->second;
            }
            for (auto& op : node.at("subops").arr) c.outerStep = c.outerStep || (op.get("subop") && op.s("subop") == "union");
            for (auto& op : node.at("subops").arr) handle(op, c);
            if (const J* ie = node.get("innerEdges"))
               for (auto& e : ie->arr) {
                  if (e.s("type") != "resultEdge") continue;
                  const std::string id = stateKey(e.at("input"));
                  auto it = c.local.find(id);
                  if (it == c.local.end()) throw Unsupported("step result '" + id + "' is not a state this consumer tracks");
                  states[stateKey(ref, e.at("output").iOr("resnr", 0))] = it->second;
               }
         } else {
            handle(node, c);
            for (auto& kv : c.local) states[kv.first] = kv.second;
         }
         addReport(ref, true, "", nSub);
      } catch (const Unsupported& u) {
         ok = false;
         addReport(ref, false, u.what(), nSub);
         if (err->empty()) *err = "step " + ref + ": " + u.what();
      }
   }
   if (ok && result.empty()) {
      ok = false;
      *err = "the dump never materialises into a ResultTable";
   }
   return ok;
}

std::string Translator::planJson(const std::string& name) const {
   std::string o = "{\"name\": " + quote(name) + ", \"doc\": \"translated from a mlir-subop-to-json dump by ldb_subop_translate\", \"inputs\": [";
   size_t k = 0;
   for (auto& t : inputs) o += (k++ ? ", " : "") + quote(t);
   o += "],\n \"steps\": [\n";
   for (size_t s = 0; s < steps.size(); s++) {
      const OutStep& st = steps[s];
      o += "  {\"op\": " + quote(st.op);
      for (auto& f : st.fields) o += ", " + quote(f.first) + ": " + f.second;
      if (st.op == "groupby") {
         o += ", \"aggs\": [";
         bool first = true;
         for (auto& a : st.aggs) {
            if (!a.used) continue; // aggregates nothing downstream reads (the sum / count halves of an avg)
            o += std::string(first ? "" : ", ") + "{\"fn\": " + quote(a.fn) + (a.expr.empty() ? "" : ", \"expr\": " + a.expr) + (a.when.empty() ? "" : ", \"when\": " + a.when) +
                 (a.type.empty() ? "" : ", \"type\": " + quote(a.type)) + ", \"as\": " + quote(a.as) + "}";
            first = false;
         }
         o += "]";
      }
      o += ", \"out\": " + quote(st.out) + "}" + (s + 1 < steps.size() ? ",\n" : "\n");
   }
   return o + " ], \"result\": " + quote(result) + "}\n";
}

static std::string g_subop_err, g_subop_report;

} // namespace ldbsubop

using namespace ldbsubop;
using ldbjson::JParser;

// the translation of one dump: LDB_OK and the plan text (NUL-terminated) in plan_out; LDB_ERR_UNSUPPORTED when a step has
// no device pattern (ldb_subop_report() says which); LDB_ERR_INVALID for a malformed document or a too-small buffer
// (*needed receives the size to retry with)
extern "C" int32_t ldb_subop_translate(const char* dump_json, const char* name, char* plan_out, int64_t cap, int64_t* needed) {
   g_subop_err.clear();
   g_subop_report = "[]";
   if (needed) *needed = 0;
   if (!dump_json) {
      g_subop_err = "null dump";
      return LDB_ERR_INVALID;
   }
   try {
      JParser jp(dump_json);
      const J doc = jp.value();
      Translator t;
      const bool ok = t.run(doc, &g_subop_err);
      g_subop_report = "[" + t.report + "]";
      if (!ok) return LDB_ERR_UNSUPPORTED;
      const std::string text = t.planJson(name ? name : "subop_dump");
      if (needed) *needed = (int64_t) text.size() + 1;
      if (!plan_out || cap < (int64_t) text.size() + 1) {
         g_subop_err = "output buffer too small";
         return LDB_ERR_INVALID;
      }
      memcpy(plan_out, text.c_str(), text.size() + 1);
      return LDB_OK;
   } catch (const std::exception& e) {
      g_subop_err = e.what();
      return LDB_ERR_INVALID;
   }
}
extern "C" const char* ldb_subop_last_error(void) { return g_subop_err.c_str(); }
// per execution step: {"ref", "subops", "target": "gpu" | "cpu", "reason"} — the placement handleExecutionStepGPU would make
extern "C" const char* ldb_subop_report(void) { return g_subop_report.c_str(); }
