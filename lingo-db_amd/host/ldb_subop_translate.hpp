// ldb_subop_translate.hpp — what the units of the sub-operator dump consumer share: ldb_subop.cpp (the sub-operator table, the walk
// over the document, the state-creating sub-operators, the C entry points), ldb_subop_expr.cpp (expressions and restrictions),
// ldb_subop_stream.cpp (the sub-operators of one tuple stream and the aggregation they feed) and ldb_subop_join.cpp (hash / nested-loop /
// group joins, set operations, windows).  Internal to libldb_host.so; the pattern list is the header comment of ldb_subop.cpp.
#pragma once
#include "ldb_host.hpp"
#include "ldb_json.hpp"
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace ldbsubop __attribute__((visibility("hidden"))) {
using ldbjson::J;
using ldbjson::quote;

struct Unsupported : std::runtime_error {
   using std::runtime_error::runtime_error;
};

// ------------------------------------------------------------------ expressions (the tool's expression_leaf / expression_inner)
struct Expr;
using ExprP = std::shared_ptr<Expr>;
struct Expr {
   enum Kind { COL, CONST_INT, CONST_STR, CONST_BOOL, MEMBER, REF, HASH, MARKER, FLAG, NULLV, SETCNT, UNKNOWN, OP } kind = UNKNOWN; // SETCNT: one of the two counters of INTERSECT / EXCEPT (i = 1 | 2) // MARKER: "a partner exists" of a probe row; FLAG: of a build row; NULLV: db.null
   std::string name; // COL: column name in the plan language; MEMBER: member; OP: add sub mul div cast cmp and or not isnull select between in call (cmp = the runtime function)
   std::string cmp; // OP cmp: EQ NEQ LT LTE GT GTE; constants: the dump's data_type
   int64_t i = 0;
   bool build = false; // COL gathered from the build side of the hash join being matched
   bool base = false; // COL of a scanned base table (its type is the table's: column-vs-column restrictions compare like with like)
   std::string dtype; // COL: the dump's datatype of the column it was first defined as ("decimal(12,2)", "int32", …; may be empty)
   std::vector<ExprP> args;
};
inline ExprP mk(Expr::Kind k, const std::string& name = "") {
   auto e = std::make_shared<Expr>();
   e->kind = k;
   e->name = name;
   return e;
}
inline ExprP stripCast(ExprP e) {
   while (e->kind == Expr::OP && e->name == "cast") e = e->args[0];
   return e;
}
std::string exprJson(const ExprP& e); // the plan language of ldb_plan.cpp (compileX)
ExprP flattenMul(const ExprP& e);
std::string classifySet(const ExprP& e0); // what a map over the two counters of a set operation computes ("" when nothing known)
inline std::string mirrored(const std::string& op) { return op == "LT" ? "GT" : op == "GT" ? "LT" : op == "LTE" ? "GTE" : op == "GTE" ? "LTE" : op; } // a comparison with its sides swapped
inline std::string joined(const std::vector<std::string>& items) { // a JSON array of raw JSON items
   std::string o = "[";
   for (size_t k = 0; k < items.size(); k++) o += (k ? ", " : "") + items[k];
   return o + "]";
}
inline std::string nameList(const std::vector<std::string>& v) { // a JSON array of strings
   std::string o = "[";
   for (size_t k = 0; k < v.size(); k++) o += (k ? ", " : "") + quote(v[k]);
   return o + "]";
}
inline std::string sortKey(const std::string& col, bool desc) { return desc ? "{\"col\": " + quote(col) + ", \"desc\": true}" : quote(col); } // one entry of "by" / "order_by"

// ------------------------------------------------------------------ what the walk keeps
struct Stream {
   std::string rel; // plan value holding the rows
   bool bareTable = false; // `rel` is an input table nothing has been applied to yet (its restrictions are in `preds`)
   std::vector<std::string> preds; // restrictions not yet applied (JSON objects of the plan language)
   std::map<std::string, ExprP> cols; // column displayName ("lineitem::l_quantity") → what it is
   std::set<std::string> names; // every column name the relation physically has (the plan language resolves columns by name)
   std::vector<std::set<std::string>> unique; // column sets known to identify a row
   std::string aggState; // the state being reduced into
   // the hash join being matched: its equalities are known, the join kind is not yet: inner unless the marker idiom of a
   // semi / anti join follows (RelAlgToSubOp.cpp:1296-1375).  Emitting the join resets all of it with one assignment.
   struct JoinMatch {
      bool pending = false;
      bool inJoinBody = false; // between the gather of a hash join and the end of its nested_map: filters are conjuncts of the join predicate
      std::string probeHiv; // the hash-indexed view being probed
      std::vector<std::string> probeKeys, buildKeys;
      std::vector<bool> keyDecimal; // per key pair: a decimal column is involved (kept as a residual equality when an integer key exists)
      std::vector<std::string> residual; // non-equality conjuncts relating the two sides ({"probe", "op", "build"})
   } join;
   std::vector<ExprP> postJoin; // conjuncts of the join predicate that do not relate one probe with one build column: applied to the joined rows (inner joins only; NOT reset with `join`)
   std::string flagState; // scan of a build buffer whose flag member a semi / anti join with reversed sides has set
   std::string nlBuild; // nested-loop join (translateNLJ): the buffer being scanned once per tuple of this stream
   bool flagAntiPending = false; // a flagged buffer scanned for its UNflagged rows in a step that also has a union: the unmatched half of a reversed outer join (when a map of NULLs follows) or an ordinary anti join of the build side (anything else)
   bool fullOuter = false; // the matches and the partner-less probe rows of a FULL outer join: united with the unmatched build rows after the probe pipeline
   bool antiBranch = false; // outer / single join: the branch of the probe rows WITHOUT a partner (filter none_true on the marker)
   std::string constState; // constant single join: the one-row state this stream looked up
   std::vector<std::string> lastMapped; // the columns the most recent map defined (UNION ALL maps both inputs to the result columns)
   // a window being evaluated on this stream: the continuous view it scans, the functions collected so far and their common frame
   struct WinFn {
      std::string fn, col, as;
   };
   struct Window {
      std::string view, lookup, staticView; // staticView: a plain scan of the view feeding the whole-partition aggregation of a frame unbounded on both sides
      std::vector<WinFn> fns;
      bool frame = false, hasTo = false;
      int64_t from = 0, to = 0;
   } win;
   std::string partState; // scan of the map of per-partition buffers: the buffer column stands for this state inside the nested_map
   std::string gjState; // group join: this stream probes the map the other input created (GroupJoinLowering, RelAlgToSubOp.cpp:2682-2950)
   std::string setState; // scan of the counting map of INTERSECT / EXCEPT: the set operation is emitted when its predicate / repeat count is consumed
};
struct AggSpec {
   std::string member, fn;
   ExprP arg; // null for count(*)
};
struct OutAgg {
   std::string fn, expr, as;
   std::string when, type; // conditional aggregate: sum(case when <conjunction> then x else 0 end); result type override
   bool used = false;
};
using Fields = std::vector<std::pair<std::string, std::string>>; // key → raw JSON, in order
struct OutStep {
   std::string op, out;
   Fields fields;
   std::vector<OutAgg> aggs; // groupby
};
struct State {
   enum Kind { UNKNOWN, TABLE, AGG, BUFFER, HIV, SORTED, HEAP, RESULT, MARKER, CONST1, CONTVIEW, SEGTREE } kind = UNKNOWN; // CONST1: the scattered one-row state of a constant single join; CONTVIEW / SEGTREE: the views of a window
   std::string table; // TABLE
   std::map<std::string, std::string> memberToIdent;
   std::vector<std::string> filters, pkey;
   Stream in; // AGG: the reduced stream; BUFFER/HEAP/RESULT/SORTED: the materialised one
   std::vector<AggSpec> aggs;
   int groupbyStep = -1; // AGG: index of the emitted groupby (emitted when the state is first scanned)
   std::map<std::string, std::string> aggOut; // AGG: member → output column
   std::map<std::string, ExprP> members; // BUFFER …: member → what was stored
   std::shared_ptr<State> source; // HIV / SORTED: the buffer underneath
   std::string ht; // HIV: the plan value of the built table
   std::vector<std::string> htKeys;
   bool htUnique = false;
   std::vector<std::pair<std::string, bool>> sortBy; // member, descending
   int64_t maxRows = -1;
   bool emitted = false; // SORTED / HEAP: the sort / topk step exists and in.rel names its output
   // BUFFER that is the build side of a semi / anti join with reversed sides: the flag member, the probing stream (kept
   // for the anti form, which is emitted when the flag filter says all_false) and the build rows with a partner
   std::string flagMember, semiRel, antiRel;
   std::shared_ptr<Stream> flagProbe;
   std::shared_ptr<State> flagHiv;
   // AGG reduced by TWO pipelines with nothing but row counters: the map of a UNION (distinct) / INTERSECT / EXCEPT
   // windows (WindowLowering, RelAlgToSubOp.cpp:2193-2553): SORTED remembers its order, a BUFFER filled inside the reduce of a map keyed by the
   // PARTITION BY columns remembers them, a SEGTREE its aggregates (emitter extension E8)
   std::vector<std::pair<std::string, bool>> sortCols; // column, descending
   std::vector<std::string> partCols;
   bool partPending = false; // BUFFER filled per partition: the keys are named by the scan of the map
   struct WinAgg {
      std::string member, fn, source;
   };
   std::vector<WinAgg> winAggs;
   // AGG whose map a second stream looks up and aggregates into: a group join
   std::shared_ptr<Stream> gjRight;
   std::vector<AggSpec> gjAggs;
   std::vector<ExprP> gjFilters;
   std::vector<std::pair<std::string, ExprP>> gjPairs, gjStored; // (left key column, the right column renamed to it); (gjval member, placeholder of the stored left column)
   bool gjInner = false;
   std::shared_ptr<Stream> setRight;
   std::string setLeftCounter, setRightCounter;
   std::vector<std::string> setLeftCols, setRightCols;
};
using StateP = std::shared_ptr<State>;

// ------------------------------------------------------------------ one execution step
struct StepCtx {
   std::vector<StateP> args;
   std::map<std::string, StateP> local; // "<ref>#<resnr>" of states created inside the step
   std::map<std::string, Stream> streams; // by producing sub-operator
   Stream* nested = nullptr; // the stream a nested_map hands to its body
   bool outerBody = false; // the nested_map body being walked ends in a union: an outer / single join (RelAlgToSubOp.cpp:1486-1587)
   bool outerStep = false; // the step itself has a union: an outer join with reverseSides unites the matches with the unmatched build rows
};

struct Translator {
   std::vector<OutStep> steps;
   std::map<std::string, StateP> states; // "<step ref>#<resnr>" → state
   std::map<std::string, std::pair<int, int>> aggCol; // output column name → (groupby step, agg index)
   std::set<std::string> inputs;
   std::string result;
   std::string markName; // the column a mark join about to be emitted adds
   std::string report; // JSON array body
   std::set<std::string> ext; // the emitter extensions the dump's manifest declares (integration/mlir-subop-to-json.patch)
   int nval = 0;

   std::string fresh(const char* stem) { return std::string(stem) + std::to_string(++nval); }
   static std::string sanitize(std::string s) {
      for (size_t p; (p = s.find("::")) != std::string::npos;) s.replace(p, 2, ".");
      return s;
   }
   static std::string stripSuffix(const std::string& m) { // "revenue$4" → "revenue"
      const size_t p = m.rfind('$');
      return p == std::string::npos ? m : m.substr(0, p);
   }
   static bool isKeyMember(const std::string& m) { return m.rfind("keyval", 0) == 0 || m.rfind("gjkeyval", 0) == 0; } // performAggregation / GroupJoinLowering member names
   static std::string stateKey(const std::string& ref, int64_t resnr) { return ref + "#" + std::to_string(resnr); } // the key of `states` / StepCtx::local
   static std::string stateKey(const J& edge) { return stateKey(edge.s("ref"), edge.iOr("resnr", 0)); }

   // ---------------------------------------------------------------- ldb_subop.cpp: the document, the table, states
   bool run(const J& plan, std::string* err);
   std::string planJson(const std::string& name) const;
   void addReport(const std::string& ref, bool gpu, const std::string& reason, size_t nSubops);
   void handle(const J& op, StepCtx& c);
   StateP newState(State::Kind k, const std::string& ref, StepCtx& c);
   StateP resolve(const J& acc, StepCtx& c);
   Stream& input(const J& op, StepCtx& c);
   std::string idOf(const StateP& st, StepCtx& c);
   void opGetExternal(const J& op, const std::string& ref, StepCtx& c);
   void opCreateState(const J& op, const std::string& ref, StepCtx& c); // create_thread_local, create_simple_state, generic_create, create_array, create_from
   void opCreateHeap(const J& op, const std::string& ref, StepCtx& c);
   void opMerge(const J& op, const std::string& ref, StepCtx& c);
   void opCreateHashIndexedView(const J& op, const std::string& ref, StepCtx& c);
   void opCreateSortedView(const J& op, const std::string& ref, StepCtx& c);
   void opCreateContinuousView(const J& op, const std::string& ref, StepCtx& c);
   void opCreateSegmentTreeView(const J& op, const std::string& ref, StepCtx& c);

   // ---------------------------------------------------------------- ldb_subop_expr.cpp: expressions, restrictions, emission helpers
   ExprP convert(const J& e, const Stream& st);
   std::string emit(const char* op, const char* stem, Fields fields); // appends a step writing a fresh value `stem<n>`; returns that name
   void flush(Stream& s);
   void use(const std::string& col);
   void useAll(const ExprP& e);
   ExprP materializeCalls(Stream& s, const ExprP& e, const std::string& hint);
   void concatParts(const ExprP& e, std::vector<std::string>& out);
   std::string ensureCol(Stream& s, const ExprP& e0, const std::string& hint);
   bool condPreds(const ExprP& c0, std::vector<std::string>& out);
   void applyFilter(Stream& s, const ExprP& e0);
   static std::string predJson(const std::string& col, const std::string& op, const J* value, const J* values);

   // ---------------------------------------------------------------- ldb_subop_stream.cpp: the sub-operators of one stream, aggregation
   StateP emitGroupBy(const StateP& st, const J& mapping);
   void opScan(const J& op, const std::string& ref, StepCtx& c);
   Stream scanTable(const StateP& st, const J& mapping);
   Stream scanAggregate(const StateP& st, const J& mapping);
   Stream scanMarker(const StateP& st, const J& mapping);
   Stream scanBuffer(const StateP& st, const J& mapping, StepCtx& c); // buffer / sorted view / heap / result table
   void emitTopK(const StateP& heap);
   Stream scanNestedBuffer(const StateP& st, const J& mapping, StepCtx& c);
   void opNestedMap(const J& op, const std::string& ref, StepCtx& c);
   void opCombineTuple(const J& op, const std::string& ref, StepCtx& c);
   void opRenaming(const J& op, const std::string& ref, StepCtx& c);
   void opMap(const J& op, const std::string& ref, StepCtx& c);
   void mapConsumes(Stream& s, const J& computed);
   void mapAverage(const std::string& name, ExprP& e);
   void opFilter(const J& op, const std::string& ref, StepCtx& c);
   void filterNoneTrue(Stream& s, const J& columns, StepCtx& c);
   void opLookup(const J& op, const std::string& ref, StepCtx& c); // lookup, lookup_or_insert
   void opReduce(const J& op, const std::string& ref, StepCtx& c);
   void aggOfBody(AggSpec& a, const ExprP& e);
   void opMaterialize(const J& op, const std::string& ref, StepCtx& c);

   // ---------------------------------------------------------------- ldb_subop_join.cpp: joins, group joins, set operations, windows
   void addJoinConjunct(Stream& s, const ExprP& pred);
   void separateNames(const Stream& s, const StateP& buf, bool built);
   std::string emitJoin(Stream& s, const std::string& kind);
   void takeFlagRows(Stream& s, bool anti);
   void realiseFlag(Stream& s);
   void settle(Stream& s);
   void clearJoin(Stream& s);
   void finishProbeSide(Stream& s, bool anti);
   void emitNestedLoop(Stream& s, const ExprP& pred);
   void opScanList(const J& op, const std::string& ref, StepCtx& c);
   void opGather(const J& op, const std::string& ref, StepCtx& c);
   void gatherWindow(Stream& s, const J& op);
   void gatherGroupJoin(Stream& s, const J& op);
   void gatherConstJoin(Stream& s, const J& op);
   void gatherHashJoin(Stream& s, const J& op);
   void opUnion(const J& op, const std::string& ref, StepCtx& c);
   void opScatter(const J& op, const std::string& ref, StepCtx& c);
   void opUnwrapOptionalRef(const J& op, const std::string& ref, StepCtx& c);
   struct GroupJoin; // what the pieces of scanGroupJoin hand on
   Stream scanGroupJoin(const StateP& st, const J& mapping);
   void groupJoinLeft(GroupJoin& g);
   void groupJoinProbe(GroupJoin& g);
   void groupJoinAggregate(GroupJoin& g);
   Stream groupJoinOuter(GroupJoin& g);
   Stream groupJoinInner(GroupJoin& g);
   void emitSetOp(Stream& s, const std::string& kind);
   Stream scanSetOp(const StateP& st, const J& mapping, StepCtx& c);
   void setFrame(Stream& s, int64_t from, int64_t to, bool haveTo);
   void flushWindow(Stream& s);
   void opScanRef(const J& op, const std::string& ref, StepCtx& c);
   void opFrameReference(const J& op, const std::string& ref, StepCtx& c); // get_begin_reference, get_end_reference
   void opOffsetReferenceBy(const J& op, const std::string& ref, StepCtx& c);
   void opEntriesBetween(const J& op, const std::string& ref, StepCtx& c);
   bool lookupWindow(Stream& s, const StateP& st, const std::string& id, const J& op);
   Stream scanContinuousView(const StateP& st, const J& mapping, StepCtx& c);
   Stream scanPartitionMap(const StateP& st, const J& mapping, StepCtx& c);
};

// one row of the sub-operator table (ldb_subop.cpp): the dump's "subop" name and the handler of its pattern; several names may share one
struct OpRow {
   const char* subop;
   void (Translator::*fn)(const J& op, const std::string& ref, StepCtx& c);
};
const OpRow* findOp(const std::string& subop);

} // namespace ldbsubop
