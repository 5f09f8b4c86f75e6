// ldb_subop_stream.cpp — the sub-operator dump consumer's handlers for the sub-operators of one tuple stream: scan (by what the scanned state has
// become), nested_map, map, filter, renaming, lookup, reduce, materialize, and the groupby step an aggregation state becomes when it is
// scanned.  What a pending join, a group join, a set operation or a window needs is in ldb_subop_join.cpp.  Declarations: ldb_subop_translate.hpp.
#include "ldb_subop_translate.hpp"

namespace ldbsubop {

// ---------------------------------------------------------------- states
StateP Translator::emitGroupBy(const StateP& st, const J& mapping) {
   if (st->groupbyStep >= 0) return st;
   Stream& in = st->in;
   OutStep g;
   g.op = "groupby";
   g.out = fresh("g");
   std::vector<std::string> keys;
   for (auto& m : mapping.arr) {
      const std::string& member = m.s("member");
      if (!isKeyMember(member)) continue;
      // the scan re-defines the grouped column itself: its binding on the reduced stream is the key
      auto it = in.cols.find(m.at("column").s("displayName"));
      if (it == in.cols.end()) throw Unsupported("group key '" + m.at("column").s("displayName") + "' is not a column of the aggregated stream");
      keys.push_back(ensureCol(in, it->second, m.at("column").s("displayName")));
   }
   for (auto& a : st->aggs) {
      OutAgg o;
      o.fn = a.fn;
      if (a.arg) {
         const ExprP sel = stripCast(a.arg);
         std::vector<std::string> when;
         // sum(case when c then x else 0 end): a conditional aggregate (the reference computes the case in a map before the reduce)
         if (a.fn == "sum" && sel->kind == Expr::OP && sel->name == "select" && stripCast(sel->args[2])->kind == Expr::CONST_INT && stripCast(sel->args[2])->i == 0 &&
             condPreds(sel->args[0], when)) {
            const ExprP then = stripCast(sel->args[1]);
            useAll(then);
            o.expr = exprJson(flattenMul(then));
            o.when = joined(when);
            if (then->kind == Expr::CONST_INT && then->cmp == "int32") o.type = "int32"; // integer literals are int32 and SUM keeps the type
         } else {
            useAll(a.arg);
            o.expr = exprJson(flattenMul(a.arg));
         }
      }
      std::string as;
      for (auto& m : mapping.arr)
         if (m.s("member") == a.member) as = sanitize(m.at("column").s("displayName"));
      o.as = as.empty() ? sanitize(st->in.rel + "." + a.member) : as;
      o.used = a.member == "distinct$count"; // (a distinct projection reads no aggregate: its group-by keeps the row count)
      st->aggOut[a.member] = o.as;
      g.aggs.push_back(o);
   }
   g.fields = {{"in", quote(in.rel)}, {"keys", nameList(keys)}};
   if (keys.empty()) g.fields.push_back({"est_groups", "1"});
   if (!in.preds.empty()) {
      if (!in.bareTable) {
         flush(in);
         g.fields[0].second = quote(in.rel);
      } else { // restrictions of the scanned table fuse into the aggregation kernel (scan → filter → aggregate in one pass)
         g.fields.push_back({"preds", joined(in.preds)});
      }
   }
   st->groupbyStep = (int) steps.size();
   for (size_t k = 0; k < g.aggs.size(); k++) aggCol[g.aggs[k].as] = {st->groupbyStep, (int) k};
   steps.push_back(g);
   Stream out;
   out.rel = g.out;
   out.names.insert(keys.begin(), keys.end());
   for (auto& a : g.aggs) out.names.insert(a.as);
   if (!keys.empty()) out.unique.push_back(std::set<std::string>(keys.begin(), keys.end()));
   size_t kk = 0;
   for (auto& m : mapping.arr) {
      const std::string& member = m.s("member");
      if (isKeyMember(member)) st->aggOut[member] = keys[kk++];
   }
   st->in = out; // from here on the state IS the aggregated table
   return st;
}

// ---------------------------------------------------------------- scan: what comes out depends on what the state has become
void Translator::opScan(const J& op, const std::string& ref, StepCtx& c) {
   StateP st = resolve(op.at("accesses").arr.at(0), c);
   const J& mapping = op.at("mapping");
   if (st->kind == State::TABLE) c.streams[ref] = scanTable(st, mapping);
   else if (st->kind == State::AGG && st->gjRight) c.streams[ref] = scanGroupJoin(st, mapping);
   else if (st->kind == State::AGG && st->setRight) c.streams[ref] = scanSetOp(st, mapping, c);
   else if (st->kind == State::AGG) c.streams[ref] = scanAggregate(st, mapping);
   else if (st->kind == State::MARKER) c.streams[ref] = scanMarker(st, mapping);
   else if (st->kind == State::CONTVIEW) c.streams[ref] = scanContinuousView(st, mapping, c);
   else if (st->kind == State::BUFFER && st->partPending) c.streams[ref] = scanPartitionMap(st, mapping, c);
   else if (st->kind == State::BUFFER && c.nested) c.streams[ref] = scanNestedBuffer(st, mapping, c);
   else if (st->kind == State::BUFFER || st->kind == State::SORTED || st->kind == State::HEAP || st->kind == State::RESULT) c.streams[ref] = scanBuffer(st, mapping, c);
   else throw Unsupported("scan of a state nothing was written to");
}
Stream Translator::scanTable(const StateP& st, const J& mapping) {
   Stream s;
   s.rel = st->table;
   s.bareTable = true;
   s.preds = st->filters;
   if (!st->pkey.empty()) s.unique.push_back(std::set<std::string>(st->pkey.begin(), st->pkey.end()));
   for (auto& kv : st->memberToIdent) s.names.insert(kv.second);
   for (auto& m : mapping.arr) {
      auto it = st->memberToIdent.find(m.s("member"));
      if (it == st->memberToIdent.end()) throw Unsupported("scan of member '" + m.s("member") + "' that get_external does not map");
      ExprP c = mk(Expr::COL, it->second);
      c->base = true;
      c->dtype = m.at("column").sOr("datatype", "");
      s.cols[m.at("column").s("displayName")] = c;
   }
   return s;
}
Stream Translator::scanAggregate(const StateP& st, const J& mapping) {
   emitGroupBy(st, mapping);
   Stream s = st->in;
   for (auto& m : mapping.arr) {
      auto it = st->aggOut.find(m.s("member"));
      if (it == st->aggOut.end()) throw Unsupported("scan of member '" + m.s("member") + "' the aggregation does not produce");
      ExprP c = mk(Expr::COL, it->second);
      c->dtype = m.at("column").sOr("datatype", "");
      s.cols[m.at("column").s("displayName")] = c;
   }
   return s;
}
Stream Translator::scanMarker(const StateP& st, const J& mapping) { // the per-row marker of anyTuple: the pending join continues on the probe stream
   Stream s = st->in;
   for (auto& m : mapping.arr) s.cols[m.at("column").s("displayName")] = mk(Expr::MARKER);
   return s;
}
// the heap keeps the best maxRows rows: a top-k over what was materialised (emitted once, when the heap is first scanned)
void Translator::emitTopK(const StateP& st) {
   if (st->kind != State::HEAP || st->emitted) return;
   flush(st->in);
   std::vector<std::string> by;
   for (auto& key : st->sortBy) {
      auto it = st->members.find(key.first);
      if (it == st->members.end()) throw Unsupported("heap sort key '" + key.first + "' was not materialised");
      const std::string col = ensureCol(st->in, it->second, stripSuffix(it->first));
      it->second = mk(Expr::COL, col);
      by.push_back(sortKey(col, key.second));
   }
   st->in.rel = emit("topk", "t", {{"in", quote(st->in.rel)}, {"by", joined(by)}, {"k", std::to_string(st->maxRows)}});
   st->emitted = true;
}
// translateNLJ: the buffer is scanned once per tuple of the outer stream
Stream Translator::scanNestedBuffer(const StateP& st, const J& mapping, StepCtx& c) {
   Stream s = *c.nested;
   settle(s);
   if (!s.nlBuild.empty()) throw Unsupported("two nested scans in one nested_map body");
   s.nlBuild = idOf(st, c);
   separateNames(s, st, false);
   for (auto& m : mapping.arr) {
      auto it = st->members.find(m.s("member"));
      if (it == st->members.end()) throw Unsupported("scan of member '" + m.s("member") + "' that was never materialised");
      auto e = std::make_shared<Expr>(*stripCast(it->second));
      if (e->kind != Expr::COL) {
         const std::string colname = ensureCol(st->in, it->second, stripSuffix(it->first));
         it->second = mk(Expr::COL, colname);
         e = std::make_shared<Expr>(*it->second);
      }
      e->build = true;
      s.cols[m.at("column").s("displayName")] = e;
   }
   return s;
}
Stream Translator::scanBuffer(const StateP& st, const J& mapping, StepCtx& c) {
   emitTopK(st);
   Stream s;
   s.rel = st->in.rel;
   s.preds = st->in.preds;
   s.unique = st->in.unique;
   s.names = st->in.names;
   s.bareTable = st->in.bareTable;
   for (auto& m : mapping.arr) {
      auto it = st->members.find(m.s("member"));
      if (it == st->members.end()) throw Unsupported("scan of member '" + m.s("member") + "' that was never materialised");
      s.cols[m.at("column").s("displayName")] = it->second;
      if (!st->flagMember.empty() && m.s("member") == st->flagMember) { // the flag a reversed semi / anti join has set
         s.cols[m.at("column").s("displayName")] = mk(Expr::FLAG);
         s.flagState = idOf(st, c);
      }
   }
   return s;
}
void Translator::opNestedMap(const J& op, const std::string& ref, StepCtx& c) { // the body runs once per tuple of the input stream: inline it
   Stream s = input(op, c);
   if (!s.setState.empty()) { // INTERSECT ALL / EXCEPT ALL: the body generates `repeat` copies of the key (generate + scf.for, :893-911)
      std::string kind;
      for (auto& kv : s.cols)
         if (kv.second->kind == Expr::OP && kv.second->name == "setop") kind = kv.second->cmp;
      if (kind != "intersect_all" && kind != "except_all") throw Unsupported("nested_map over the counters of a set operation without a repeat count");
      emitSetOp(s, kind);
      c.streams[ref] = s;
      return;
   }
   Stream* outer = c.nested;
   const bool outerWas = c.outerBody;
   c.nested = &s;
   c.outerBody = false;
   std::string last;
   if (const J* body = op.get("subops")) {
      for (auto& b : body->arr) c.outerBody = c.outerBody || (b.get("subop") && b.s("subop") == "union");
      for (auto& b : body->arr) {
         handle(b, c);
         if (b.get("subop") && c.streams.count(b.s("ref"))) last = b.s("ref");
      }
   }
   c.nested = outer;
   c.outerBody = outerWas;
   c.streams[ref] = last.empty() ? s : c.streams[last];
   c.streams[ref].join.inJoinBody = false;
   flushWindow(c.streams[ref]); // a window evaluated per partition inside the body
   if (!c.streams[ref].nlBuild.empty()) emitNestedLoop(c.streams[ref], nullptr); // no predicate in the body: a cross product
}
void Translator::opCombineTuple(const J& op, const std::string& ref, StepCtx& c) { // emitter extension E6: a no-op for column bindings
   c.streams[ref] = input(op, c);
}
void Translator::opRenaming(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   for (auto& r : op.at("renamed").arr) {
      auto it = s.cols.find(r.at("old").s("displayName"));
      if (it == s.cols.end()) throw Unsupported("renaming of an undefined column");
      s.cols[r.at("new").s("displayName")] = it->second;
      if (!s.gjState.empty()) states.at(s.gjState)->gjPairs.push_back({r.at("new").s("displayName"), it->second}); // left key := the right key it equals
   }
   c.streams[ref] = s;
}
// what a map decides before it binds its columns: whether it consumes the matched pairs of a pending join, the unflagged rows of a build
// buffer or the results of a window (and so makes them steps), or is part of the idiom that is still being matched
void Translator::mapConsumes(Stream& s, const J& computed) {
   if (s.join.pending && !s.join.inJoinBody) { // `map … = true` is the first sub-operator of the marker idioms; anything else consumes the pairs
      bool marker = true;
      for (auto& cm : computed.arr) marker = marker && convert(cm.at("expression"), s)->kind == Expr::CONST_BOOL;
      if (!marker) settle(s);
   }
   if (s.flagAntiPending) {
      bool nulls = true, copies = true;
      for (auto& cm : computed.arr) {
         const Expr::Kind k = stripCast(convert(cm.at("expression"), s))->kind;
         nulls = nulls && k == Expr::NULLV;
         copies = copies && k == Expr::COL;
      }
      if (nulls) { // the unmatched BUILD rows of an outer join with reverseSides: null-extended and united with the matches below
         s.flagAntiPending = false;
         s.antiBranch = true;
      } else if (!copies) { // (as-nullable copies of the build columns precede the NULLs of a full outer join: still undecided)
         realiseFlag(s);
      }
   }
   if (!s.win.fns.empty() || !s.win.view.empty()) { // a map that is not part of the window evaluation consumes its results
      bool part = true;
      for (auto& cm : computed.arr) {
         const ExprP e = stripCast(convert(cm.at("expression"), s));
         part = part && (e->kind == Expr::CONST_INT || (e->kind == Expr::OP && e->name == "add" && stripCast(e->args[0])->kind == Expr::OP && stripCast(e->args[0])->name == "wbetween"));
      }
      if (!part) flushWindow(s);
   }
}
// sum(x) / count(x) over one aggregation = avg(x) (the frontend's expansion of avg): a further aggregate of that groupby, `e` becomes its column
void Translator::mapAverage(const std::string& name, ExprP& e) {
   const ExprP d = stripCast(e);
   if (d->kind != Expr::OP || d->name != "div") return;
   const ExprP n = stripCast(d->args[0]), m = stripCast(d->args[1]);
   auto a = n->kind == Expr::COL ? aggCol.find(n->name) : aggCol.end();
   auto b = m->kind == Expr::COL ? aggCol.find(m->name) : aggCol.end();
   if (a == aggCol.end() || b == aggCol.end() || a->second.first != b->second.first) return;
   OutStep& g = steps[(size_t) a->second.first];
   const OutAgg& sum = g.aggs[(size_t) a->second.second];
   const OutAgg& cnt = g.aggs[(size_t) b->second.second];
   if (sum.fn != "sum" || !(cnt.fn == "count_star" || (cnt.fn == "count" && cnt.expr == sum.expr))) return;
   OutAgg avg;
   avg.fn = "avg";
   avg.expr = sum.expr;
   avg.as = sanitize(name);
   aggCol[avg.as] = {a->second.first, (int) g.aggs.size()};
   g.aggs.push_back(avg);
   e = mk(Expr::COL, avg.as);
}
void Translator::opMap(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   mapConsumes(s, op.at("computed"));
   s.lastMapped.clear();
   for (auto& cm : op.at("computed").arr) {
      const std::string& name = cm.at("computed").s("displayName");
      ExprP e = convert(cm.at("expression"), s);
      s.lastMapped.push_back(name);
      if (!s.win.view.empty() && stripCast(e)->kind == Expr::OP && stripCast(e)->name == "add" && stripCast(stripCast(e)->args[0])->kind == Expr::OP &&
          stripCast(stripCast(e)->args[0])->name == "wbetween" && stripCast(stripCast(e)->args[1])->kind == Expr::CONST_INT && stripCast(stripCast(e)->args[1])->i == 1) {
         // rank = entries between the frame begin and the current row + 1 (arith.addi: emitter extension E7)
         setFrame(s, stripCast(stripCast(e)->args[0])->i, 0, false);
         Stream::WinFn f;
         f.fn = "rank";
         f.as = sanitize(name);
         s.win.fns.push_back(f);
         s.cols[name] = mk(Expr::COL, f.as);
         continue;
      }
      if (!s.setState.empty()) { // the predicate / repeat count over the counters of INTERSECT / EXCEPT
         const std::string kind = classifySet(e);
         if (kind.empty()) throw Unsupported("expression over the counters of a set operation that is neither INTERSECT nor EXCEPT");
         ExprP r = mk(Expr::OP, "setop");
         r->cmp = kind;
         s.cols[name] = r;
         continue;
      }
      mapAverage(name, e);
      s.cols[name] = e;
   }
   c.streams[ref] = s;
}
// none of the columns true: only the anti forms of the marker idioms
void Translator::filterNoneTrue(Stream& s, const J& columns, StepCtx& c) {
   for (auto& col : columns.arr) {
      auto it = s.cols.find(col.s("displayName"));
      if (it == s.cols.end()) throw Unsupported("filter on an undefined column");
      const Expr::Kind k = stripCast(it->second)->kind;
      if (k == Expr::MARKER && s.join.pending) {
         if (c.outerBody) s.antiBranch = true; // outer / single join: the partner-less rows are null-extended and united with the matches
         else finishProbeSide(s, true);
      } else if (k == Expr::FLAG && c.outerStep) {
         s.flagAntiPending = true; // decided by what consumes the rows (realiseFlag)
      } else if (k == Expr::FLAG) {
         takeFlagRows(s, true);
      } else throw Unsupported("filter with all_false semantic on a computed predicate");
   }
}
void Translator::opFilter(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   if (op.sOr("semantic", "all_true") != "all_true") {
      filterNoneTrue(s, op.at("columns"), c);
      c.streams[ref] = s;
      return;
   }
   for (auto& col : op.at("columns").arr) {
      auto it = s.cols.find(col.s("displayName"));
      if (it == s.cols.end()) throw Unsupported("filter on an undefined column");
      const ExprP e = it->second;
      const ExprP p = stripCast(e);
      if (p->kind == Expr::MARKER) { // anyTuple's marker: the probe row has (all_true) / lacks (all_false) a partner
         if (!s.join.pending) throw Unsupported("marker filter without a pending hash join");
         finishProbeSide(s, false);
         continue;
      }
      if (p->kind == Expr::OP && p->name == "not" && stripCast(p->args[0])->kind == Expr::MARKER) { // `not mark` of a mark join
         if (!s.join.pending) throw Unsupported("marker filter without a pending hash join");
         finishProbeSide(s, true);
         continue;
      }
      if (p->kind == Expr::FLAG) { // flag member of a build buffer: build rows with a partner
         takeFlagRows(s, false);
         continue;
      }
      if (p->kind == Expr::CONST_BOOL && p->i) continue; // (the `matched` marker of an inner group join: true for every group the join produced)
      if (!s.gjState.empty()) { // the group join's predicate: applied to the joined rows before they are aggregated
         states.at(s.gjState)->gjFilters.push_back(e);
         continue;
      }
      if (p->kind == Expr::OP && p->name == "setop") { // INTERSECT / EXCEPT (distinct): keep the keys whose counters satisfy the predicate
         if (s.setState.empty() || (p->cmp != "intersect" && p->cmp != "except")) throw Unsupported("filter on the counters of a set operation that is not INTERSECT / EXCEPT (distinct)");
         emitSetOp(s, p->cmp);
         continue;
      }
      if (s.join.inJoinBody && !s.join.probeHiv.empty()) {
         addJoinConjunct(s, e);
         continue;
      }
      if (!s.nlBuild.empty()) {
         emitNestedLoop(s, e);
         continue;
      }
      settle(s);
      applyFilter(s, e);
   }
   c.streams[ref] = s;
}
void Translator::opLookup(const J& op, const std::string& ref, StepCtx& c) {
   const std::string& kind = op.s("subop"); // lookup | lookup_or_insert
   Stream s = input(op, c);
   StateP st = resolve(op.at("accesses").arr.at(0), c);
   const std::string stateType = op.sOr("stateType", "");
   std::string id;
   for (auto& kv : c.local)
      if (kv.second == st) id = kv.first;
   if (id.empty())
      for (auto& kv : states)
         if (kv.second == st) id = kv.first;
   if (kind == "lookup" && lookupWindow(s, st, id, op)) { // the aggregates of a window's frame
      c.streams[ref] = s;
      return;
   }
   if (!(stateType == "SimpleState" && kind == "lookup")) settle(s);
   if (stateType == "HashIndexedView" && kind == "lookup") {
      if (st->kind != State::HIV) throw Unsupported("lookup into a hash-indexed view that was not created from a buffer");
      if (!s.join.probeHiv.empty()) throw Unsupported("nested hash-indexed-view lookups");
      states[id] = st;
      s.join.probeHiv = id;
   } else if (stateType == "HashMap" && kind == "lookup") { // the second input of a group join looks its group up (an optional reference)
      if (st->kind != State::AGG || st->gjRight) throw Unsupported("lookup into a hash map that no other pipeline has filled");
      states[id] = st;
      s.gjState = id;
   } else if (stateType == "SimpleState" && kind == "lookup" && st->kind == State::CONST1) {
      states[id] = st;
      s.constState = id;
   } else if ((stateType == "SimpleState" && kind == "lookup") || (stateType == "HashMap" && kind == "lookup_or_insert")) {
      if (st->kind != State::UNKNOWN && !(st->kind == State::AGG && kind == "lookup_or_insert" && !st->setRight)) throw Unsupported("aggregation into a state that is already in use");
      states[id] = st;
      s.aggState = id;
   } else {
      throw Unsupported(kind + " on a " + (stateType.empty() ? "state" : stateType));
   }
   s.cols[op.at("reference").s("displayName")] = mk(Expr::REF);
   c.streams[ref] = s;
}
// the function and the argument of one updated member of a reduce, read off its body
void Translator::aggOfBody(AggSpec& a, const ExprP& e) {
   auto isMember = [&](const ExprP& x) { return x->kind == Expr::MEMBER && x->name == a.member; };
   // SumAggrFunc / CountAggrFunc / CountStarAggrFunc / Min / Max bodies (RelAlgToSubOp.cpp:1805-2020)
   if (e->kind == Expr::OP && e->name == "select" && e->args[0]->kind == Expr::OP && e->args[0]->name == "isnull" && isMember(e->args[0]->args[0]) &&
       e->args[2]->kind == Expr::OP && e->args[2]->name == "add") { // nullable state: isnull(state) ? arg : state + arg
      a.fn = "sum";
      a.arg = e->args[1];
   } else if (e->kind == Expr::OP && e->name == "add" && isMember(e->args[0])) {
      if (e->args[1]->kind == Expr::CONST_INT && e->args[1]->i == 1) a.fn = "count_star";
      else {
         a.fn = "sum";
         a.arg = e->args[1];
      }
   } else if (e->kind == Expr::OP && e->name == "add" && e->args[0]->kind == Expr::OP && e->args[0]->name == "select" && e->args[0]->args[0]->kind == Expr::OP &&
              e->args[0]->args[0]->name == "isnull" && isMember(e->args[0]->args[0]->args[0]) && e->args[1]->kind == Expr::OP && e->args[1]->name == "select" &&
              e->args[1]->args[0]->kind == Expr::OP && e->args[1]->args[0]->name == "isnull") {
      // nullable state, nullable argument: (isnull(state) ? 0 : val(state)) + (isnull(arg) ? 0 : val(arg)) — NULLs do not count
      a.fn = "sum";
      a.arg = e->args[1]->args[0]->args[0];
   } else if (e->kind == Expr::OP && e->name == "select" && e->args[0]->kind == Expr::OP && e->args[0]->name == "isnull" && !isMember(e->args[0]->args[0]) && isMember(e->args[1]) &&
              e->args[2]->kind == Expr::OP && e->args[2]->name == "add" && isMember(e->args[2]->args[0])) { // CountAggrFunc over a nullable argument: isnull(arg) ? state : state + 1
      a.fn = "count";
      a.arg = e->args[0]->args[0];
   } else if (e->kind == Expr::OP && e->name == "select" && isMember(e->args[2]) && e->args[0]->kind == Expr::OP && (e->args[0]->name == "cmp" || e->args[0]->name == "or")) {
      // Min / Max: state > arg ? arg : state; with a nullable state the condition is (state > arg) or isnull(state) (arith.ori, emitter extension E7)
      ExprP cmp = e->args[0];
      if (cmp->name == "or") {
         ExprP found;
         for (auto& x : cmp->args)
            if (x->kind == Expr::OP && x->name == "cmp") found = x;
         if (!found) throw Unsupported("aggregate body with an unrecognised condition");
         cmp = found;
      }
      if (!isMember(cmp->args[0])) throw Unsupported("aggregate body with an unrecognised comparison");
      a.fn = cmp->cmp == "GT" ? "min" : cmp->cmp == "LT" ? "max" : "";
      a.arg = e->args[1];
      if (a.fn.empty()) throw Unsupported("aggregate body with an unrecognised comparison");
   } else if (e->kind == Expr::COL || (e->kind == Expr::OP && e->name == "cast" && stripCast(e)->kind == Expr::COL)) { // AnyAggrFunc: the state becomes the argument
      a.fn = "any";
      a.arg = e;
   } else {
      throw Unsupported("aggregate body of member '" + a.member + "' is not sum / count / min / max");
   }
}
void Translator::opReduce(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   settle(s);
   if (const J* mat = op.get("materialized")) { // WindowLowering with PARTITION BY: the reduce appends the tuple to its partition's buffer (emitter extension E9)
      if (s.aggState.empty()) throw Unsupported("reduce without a preceding lookup into an aggregation state");
      StateP st = states.at(s.aggState);
      if (st->kind != State::UNKNOWN) throw Unsupported("two pipelines reduce into one state");
      st->kind = State::BUFFER;
      st->partPending = true;
      for (auto& m : mat->arr) {
         auto it = s.cols.find(m.at("column").s("displayName"));
         if (it == s.cols.end()) throw Unsupported("materialize of an undefined column '" + m.at("column").s("displayName") + "'");
         st->members[m.s("member")] = it->second;
      }
      s.aggState.clear();
      st->in = s;
      c.streams[ref] = s;
      return;
   }
   if (s.aggState.empty() && s.gjState.empty()) throw Unsupported("reduce without a preceding lookup into an aggregation state");
   const bool gj = s.aggState.empty();
   StateP st = states.at(gj ? s.gjState : s.aggState);
   std::vector<AggSpec> mine;
   for (auto& u : op.at("updated").arr) {
      AggSpec a;
      a.member = u.s("member");
      ExprP e = convert(u.at("expression"), s);
      if (e->kind == Expr::MEMBER && e->name == a.member) continue; // a member returned unchanged (the other input's counter of a set operation)
      aggOfBody(a, e);
      if (a.arg && (a.arg->kind == Expr::UNKNOWN || a.arg->kind == Expr::MEMBER)) throw Unsupported("aggregate argument without a device form");
      mine.push_back(a);
   }
   if (gj) { // the aggregates of a group join, over the tuples of this input that found their group
      st->gjAggs = mine;
      st->gjRight = std::make_shared<Stream>(s);
      st->gjRight->gjState.clear();
      c.streams[ref] = s;
      return;
   }
   if (st->kind == State::AGG) { // the second input of UnionDistinctLowering / CountingSetOperationLowering (:636-915) counts into the same map
      bool counters = !st->setRight && mine.size() <= 1 && st->aggs.size() == 1 && st->aggs[0].fn == "count_star" && (mine.empty() || mine[0].fn == "count_star");
      if (!counters || (mine.empty() != (st->aggs[0].member == "distinct$count"))) throw Unsupported("two pipelines reduce into one state");
      st->setRight = std::make_shared<Stream>(s);
      st->setRight->aggState.clear();
      st->setLeftCounter = mine.empty() ? "" : st->aggs[0].member;
      st->setRightCounter = mine.empty() ? "" : mine[0].member;
      s.aggState.clear();
      c.streams[ref] = s;
      return;
   }
   if (st->kind != State::UNKNOWN) throw Unsupported("two pipelines reduce into one state");
   st->aggs = mine;
   if (st->aggs.empty()) { // ProjectionDistinctLowering: a map of keys only
      AggSpec a;
      a.member = "distinct$count";
      a.fn = "count_star";
      st->aggs.push_back(a);
   }
   st->kind = State::AGG;
   s.aggState.clear();
   st->in = s;
   c.streams[ref] = s;
}
void Translator::opMaterialize(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   StateP st = resolve(op.at("accesses").arr.at(0), c);
   const std::string stateType = op.sOr("stateType", "");
   settle(s);
   if (!s.join.probeHiv.empty()) throw Unsupported("materialize between a lookup and its join predicate");
   if (stateType == "Heap") {
      if (st->kind != State::HEAP) throw Unsupported("materialize into a heap create_heap did not describe");
   } else if (stateType == "Buffer" || stateType == "ResultTable") {
      if (st->kind != State::UNKNOWN) throw Unsupported("two pipelines materialise into one " + stateType);
      st->kind = stateType == "Buffer" ? State::BUFFER : State::RESULT;
   } else {
      throw Unsupported("materialize into a " + stateType);
   }
   std::vector<std::string> order;
   for (auto& m : op.at("mapping").arr) {
      auto it = s.cols.find(m.at("column").s("displayName"));
      if (it == s.cols.end()) throw Unsupported("materialize of an undefined column '" + m.at("column").s("displayName") + "'");
      st->members[m.s("member")] = it->second;
      order.push_back(m.s("member"));
   }
   st->in = s;
   if (st->kind == State::RESULT) {
      flush(st->in);
      std::vector<std::string> cols;
      for (auto& member : order) {
         ExprP& e = st->members[member];
         if (stripCast(e)->kind == Expr::HASH || stripCast(e)->kind == Expr::REF) throw Unsupported("result column that is a hash or a reference");
         cols.push_back(ensureCol(st->in, e, stripSuffix(member)));
         e = mk(Expr::COL, cols.back());
      }
      OutStep m; // (the one step whose value has a fixed name)
      m.op = "materialize";
      m.out = result = "result";
      m.fields = {{"in", quote(st->in.rel)}, {"cols", nameList(cols)}};
      steps.push_back(m);
   }
   c.streams[ref] = s;
}

} // namespace ldbsubop
