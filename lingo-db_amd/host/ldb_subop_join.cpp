// ldb_subop_join.cpp — the sub-operator dump consumer's patterns that span more than one stream: the hash join being matched on a stream
// (its conjuncts, its kind, join_build / join_probe), nested-loop and constant single joins, group joins, set operations, windows, and the
// handlers of the sub-operators that belong to them (scan_list, gather, union, scatter, the reference sub-operators of a window).
// Declarations: ldb_subop_translate.hpp.
#include "ldb_subop_translate.hpp"
#include <algorithm>
#include <functional>

namespace ldbsubop {

static std::string residualJson(const std::string& probe, const std::string& op, const std::string& build) { // one comparison between the sides of a join
   return "{\"probe\": " + quote(probe) + ", \"op\": " + quote(op) + ", \"build\": " + quote(build) + "}";
}
// which side of the hash join being matched an expression reads: 0 nothing, 1 probe, 2 build, 3 both
static int sideOf(const ExprP& e) {
   int r = e->kind == Expr::COL ? (e->build ? 2 : 1) : 0;
   for (auto& a : e->args) r |= sideOf(a);
   return r;
}
// one filter inside the nested_map body of a hash join = conjunct(s) of the join predicate (translateSelection emits one
// map + filter per conjunct, RelAlgToSubOp.cpp:173-258): probe = build equalities are the keys, other comparisons
// between the sides the residual of the probe, anything else is applied to the joined rows
void Translator::addJoinConjunct(Stream& s, const ExprP& pred) {
   StateP hiv = states.at(s.join.probeHiv);
   std::vector<ExprP> conj;
   std::function<void(const ExprP&)> split = [&](const ExprP& e0) {
      const ExprP e = stripCast(e0);
      if (e->kind == Expr::OP && e->name == "and")
         for (auto& a : e->args) split(a);
      else
         conj.push_back(e);
   };
   split(pred);
   Stream& b = hiv->source->in;
   for (auto& e : conj) {
      if (e->kind == Expr::OP && e->name == "cmp") {
         ExprP l = stripCast(e->args[0]), r = stripCast(e->args[1]);
         std::string op = e->cmp;
         if (sideOf(l) == 2 && sideOf(r) == 1) {
            std::swap(l, r);
            op = mirrored(op);
         }
         if (sideOf(l) == 1 && sideOf(r) == 2) {
            const std::string bc = ensureCol(b, r, "build_key"), pc = ensureCol(s, l, "probe_key");
            if (op == "EQ") {
               s.join.buildKeys.push_back(bc);
               s.join.probeKeys.push_back(pc);
               s.join.keyDecimal.push_back(l->dtype.find("decimal") != std::string::npos || r->dtype.find("decimal") != std::string::npos);
            } else {
               s.join.residual.push_back(residualJson(pc, op, bc));
            }
            continue;
         }
      }
      s.postJoin.push_back(e);
   }
   s.join.pending = true;
}
// the plan language resolves columns by name: when the rows of `buf` are about to be joined to a stream that already has
// columns of the same names (self joins, the same table inside a subquery, a group key named like its input column), the
// buffer's columns are re-materialised under fresh names first
void Translator::separateNames(const Stream& s, const StateP& buf, bool built) {
   Stream& b = buf->in;
   bool clash = false;
   for (auto& n : b.names) clash = clash || s.names.count(n);
   if (!clash) return;
   if (built) throw Unsupported("column names of the two join sides collide and the hash table is already built");
   std::vector<std::pair<std::string, std::string>> cols; // member → current column
   for (auto& kv : buf->members) {
      const Expr::Kind k = stripCast(kv.second)->kind;
      if (k == Expr::HASH || k == Expr::REF || k == Expr::CONST_BOOL || k == Expr::FLAG || k == Expr::MARKER || k == Expr::NULLV) continue;
      cols.push_back({kv.first, ensureCol(b, kv.second, stripSuffix(kv.first))});
   }
   flush(b);
   std::map<std::string, std::string> renamed;
   std::string list = "[";
   for (auto& mc : cols) {
      if (renamed.count(mc.second)) continue;
      const std::string to = s.names.count(mc.second) ? mc.second + "_" + std::to_string(++nval) : mc.second;
      renamed[mc.second] = to;
      list += std::string(list.size() > 1 ? ", " : "") + (to == mc.second ? quote(to) : "{\"col\": " + quote(mc.second) + ", \"as\": " + quote(to) + "}");
   }
   b.rel = emit("materialize", "v", {{"in", quote(b.rel)}, {"cols", list + "]"}});
   b.bareTable = false;
   b.names.clear();
   for (auto& r : renamed) b.names.insert(r.second);
   for (auto& mc : cols) buf->members[mc.first] = mk(Expr::COL, renamed[mc.second]);
   std::vector<std::set<std::string>> uniq;
   for (auto& u : b.unique) {
      std::set<std::string> r;
      bool all = true;
      for (auto& k : u) {
         auto it = renamed.find(k);
         all = all && it != renamed.end();
         if (it != renamed.end()) r.insert(it->second);
      }
      if (all) uniq.push_back(r);
   }
   b.unique = uniq;
}
// join_build (once per view) + join_probe of the pending join with the given kind; returns the output relation
std::string Translator::emitJoin(Stream& s, const std::string& kind) {
   StateP hiv = states.at(s.join.probeHiv);
   Stream& b = hiv->source->in;
   if (s.join.probeKeys.empty()) throw Unsupported("hash join without an equality between the sides");
   if (s.join.keyDecimal.size() == s.join.probeKeys.size() && std::count(s.join.keyDecimal.begin(), s.join.keyDecimal.end(), false) > 0 && std::count(s.join.keyDecimal.begin(), s.join.keyDecimal.end(), true) > 0) {
      // integer keys hash; an equality of decimals (a correlated MIN / MAX joined back, Q2) stays a residual comparison of the pair
      std::vector<std::string> pk, bk;
      for (size_t k = 0; k < s.join.probeKeys.size(); k++) {
         if (!s.join.keyDecimal[k]) {
            pk.push_back(s.join.probeKeys[k]);
            bk.push_back(s.join.buildKeys[k]);
         } else {
            s.join.residual.push_back(residualJson(s.join.probeKeys[k], "EQ", s.join.buildKeys[k]));
         }
      }
      s.join.probeKeys = pk;
      s.join.buildKeys = bk;
      s.join.keyDecimal.assign(pk.size(), false);
   }
   if (hiv->ht.empty()) {
      flush(b);
      bool uniq = false;
      const std::set<std::string> ks(s.join.buildKeys.begin(), s.join.buildKeys.end());
      for (auto& u : b.unique) {
         bool sub = !u.empty();
         for (auto& c : u) sub = sub && ks.count(c);
         uniq = uniq || sub;
      }
      hiv->ht = emit("join_build", "h", {{"in", quote(b.rel)}, {"keys", nameList(s.join.buildKeys)}, {"unique", uniq ? "true" : "false"}});
      hiv->htKeys = s.join.buildKeys;
      hiv->htUnique = uniq;
   } else if (hiv->htKeys != s.join.buildKeys) {
      throw Unsupported("one hash-indexed view probed on two different key lists");
   }
   flush(s);
   Fields probe = {{"ht", quote(hiv->ht)}, {"in", quote(s.rel)}, {"keys", nameList(s.join.probeKeys)}, {"kind", quote(kind)}};
   if (!s.join.residual.empty()) probe.push_back({"residual", joined(s.join.residual)});
   if (kind == "mark") probe.push_back({"mark_as", quote(markName)});
   if (kind != "inner" && !s.postJoin.empty()) throw Unsupported("a " + kind + " join whose predicate has a conjunct on one side only");
   return emit("join_probe", "j", probe);
}

// the rows of a flagged build buffer as rows: those with a partner (semi_build) or without (anti_build), emitted once per buffer
// (the build side's restrictions were applied when its hash table was built)
void Translator::takeFlagRows(Stream& s, bool anti) {
   StateP buf = states.at(s.flagState);
   std::string& rel = anti ? buf->antiRel : buf->semiRel;
   if (rel.empty()) rel = emitJoin(*buf->flagProbe, anti ? "anti_build" : "semi_build");
   s.rel = rel;
   s.preds.clear();
   s.bareTable = false;
   s.flagState.clear();
}
// the unflagged rows of a build buffer are consumed as rows: an anti join keeping the build side
void Translator::realiseFlag(Stream& s) {
   if (!s.flagAntiPending) return;
   s.flagAntiPending = false;
   takeFlagRows(s, true);
}
// the pending join turns out to be an ordinary (inner) one: some other sub-operator consumes the matched pairs
void Translator::settle(Stream& s) {
   realiseFlag(s);
   flushWindow(s);
   if (!s.join.pending) return;
   StateP hiv = states.at(s.join.probeHiv);
   bool marked = false;
   for (auto& kv : s.cols) marked = marked || kv.second->kind == Expr::MARKER;
   if (marked) { // MarkJoinLowering (RelAlgToSubOp.cpp:1376-1408): the marker is read as a value (mark or …), not filtered on: every probe row + a boolean column
      markName = "mark" + std::to_string(++nval);
      s.rel = emitJoin(s, "mark");
      ExprP m = mk(Expr::COL, markName);
      s.names.insert(markName);
      s.join = Stream::JoinMatch();
      for (auto it = s.cols.begin(); it != s.cols.end();) {
         if (it->second->kind == Expr::MARKER) it->second = m;
         it = it->second->build ? s.cols.erase(it) : std::next(it);
      }
      return;
   }
   s.rel = emitJoin(s, "inner");
   s.names.insert(hiv->source->in.names.begin(), hiv->source->in.names.end());
   clearJoin(s);
   if (!hiv->htUnique) s.unique.clear(); // probe rows may repeat
   const std::vector<ExprP> post = s.postJoin;
   s.postJoin.clear();
   for (auto& e : post) applyFilter(s, e);
}
// the columns gathered from the build side are columns of the stream itself from here on
static void adoptBuildCols(Stream& s) {
   for (auto& kv : s.cols)
      if (kv.second->build) {
         auto c = std::make_shared<Expr>(*kv.second);
         c->build = false;
         kv.second = c;
      }
}
// the join has been emitted: its build columns are columns of the stream now
void Translator::clearJoin(Stream& s) {
   s.join = Stream::JoinMatch();
   adoptBuildCols(s);
}
// semi / anti join keeping the PROBE rows: the build columns are gone afterwards
void Translator::finishProbeSide(Stream& s, bool anti) {
   s.rel = emitJoin(s, anti ? "anti" : "semi");
   s.join = Stream::JoinMatch();
   for (auto it = s.cols.begin(); it != s.cols.end();)
      it = it->second->build || it->second->kind == Expr::MARKER ? s.cols.erase(it) : std::next(it);
}

// nested-loop join: `pred` (may be null: cross product) is a conjunction of comparisons between a column of the outer
// stream and a column of the scanned buffer
void Translator::emitNestedLoop(Stream& s, const ExprP& pred) {
   StateP buf = states.at(s.nlBuild);
   Stream& b = buf->in;
   std::vector<std::string> resid;
   std::function<void(const ExprP&)> walk = [&](const ExprP& e0) {
      const ExprP e = stripCast(e0);
      if (e->kind == Expr::OP && e->name == "and") {
         for (auto& a : e->args) walk(a);
         return;
      }
      if (!(e->kind == Expr::OP && e->name == "cmp")) throw Unsupported("nested-loop join predicate that is not a conjunction of comparisons");
      ExprP l = stripCast(e->args[0]), r = stripCast(e->args[1]);
      std::string op = e->cmp;
      if (l->build && !r->build) {
         std::swap(l, r);
         op = mirrored(op);
      }
      if (l->build || !r->build) throw Unsupported("nested-loop join comparison that does not relate the two sides");
      const std::string bc = ensureCol(b, r, "nl_build"), pc = ensureCol(s, l, "nl_probe");
      resid.push_back(residualJson(pc, op, bc));
   };
   if (pred) walk(pred);
   if (resid.size() > 2) throw Unsupported("nested-loop join with more than two comparison conjuncts");
   flush(b);
   flush(s);
   s.rel = emit("join_nl", "j", {{"in", quote(s.rel)}, {"build", quote(b.rel)}, {"residual", joined(resid)}, {"kind", "\"inner\""}});
   s.names.insert(b.names.begin(), b.names.end());
   s.nlBuild.clear();
   s.unique.clear();
   adoptBuildCols(s);
}

void Translator::opScanList(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   if (s.join.probeHiv.empty()) throw Unsupported("scan_list outside a hash-indexed-view lookup");
   s.cols[op.at("elem").s("displayName")] = mk(Expr::REF);
   c.streams[ref] = s;
}
// gather: the columns behind a reference — of a window's view, of a group join's stored columns, of the one row of a constant single
// join, or of the build side of the hash join being matched
void Translator::opGather(const J& op, const std::string& ref, StepCtx& c) {
   Stream s = input(op, c);
   if (!s.win.view.empty()) gatherWindow(s, op);
   else if (!s.gjState.empty()) gatherGroupJoin(s, op);
   else if (!s.constState.empty()) gatherConstJoin(s, op);
   else gatherHashJoin(s, op);
   c.streams[ref] = s;
}
void Translator::gatherWindow(Stream& s, const J& op) {
   auto r = s.cols.find(op.at("reference").s("displayName"));
   if (r == s.cols.end() || r->second->kind != Expr::REF) throw Unsupported("gather through an undefined reference");
   StateP view = states.at(s.win.view);
   if (r->second->name == "w:cur") { // the columns of the current row
      for (auto& m : op.at("mapping").arr) {
         auto it = view->members.find(m.s("member"));
         if (it == view->members.end()) throw Unsupported("gather of member '" + m.s("member") + "' that was never materialised");
         s.cols[m.at("column").s("displayName")] = it->second;
      }
   } else if (r->second->name == "w:lookup") { // the aggregates of the frame, from the segment tree
      StateP seg = states.at(s.win.lookup);
      for (auto& m : op.at("mapping").arr) {
         const State::WinAgg* a = nullptr;
         for (auto& x : seg->winAggs)
            if (x.member == m.s("member")) a = &x;
         if (!a) throw Unsupported("gather of member '" + m.s("member") + "' the segment tree does not aggregate");
         static const std::set<std::string> known = {"sum", "min", "max", "count", "count_star"};
         if (!known.count(a->fn)) throw Unsupported("window aggregate '" + a->fn + "'");
         Stream::WinFn f;
         f.fn = a->fn;
         if (a->fn != "count_star") {
            auto it = view->members.find(a->source);
            if (it == view->members.end()) throw Unsupported("window aggregate over member '" + a->source + "' that was never materialised");
            f.col = ensureCol(s, it->second, stripSuffix(a->source));
         }
         f.as = sanitize(m.at("column").s("displayName"));
         s.win.fns.push_back(f);
         s.cols[m.at("column").s("displayName")] = mk(Expr::COL, f.as);
      }
   } else if (r->second->name == "w:static") {
      StateP agg = states.at(s.win.lookup);
      setFrame(s, INT64_MIN, INT64_MAX, true);
      for (auto& m : op.at("mapping").arr) {
         const AggSpec* a = nullptr;
         for (auto& x : agg->aggs)
            if (x.member == m.s("member")) a = &x;
         static const std::set<std::string> known = {"sum", "min", "max", "count", "count_star"};
         if (!a || !known.count(a->fn)) throw Unsupported("window aggregate of member '" + m.s("member") + "'");
         Stream::WinFn f;
         f.fn = a->fn;
         if (a->arg) f.col = ensureCol(s, a->arg, stripSuffix(a->member));
         f.as = sanitize(m.at("column").s("displayName"));
         s.win.fns.push_back(f);
         s.cols[m.at("column").s("displayName")] = mk(Expr::COL, f.as);
      }
   } else {
      throw Unsupported("gather through a frame reference");
   }
}
void Translator::gatherGroupJoin(Stream& s, const J& op) { // the left input's stored columns: resolved when the group join is emitted
   StateP st = states.at(s.gjState);
   for (auto& m : op.at("mapping").arr) {
      ExprP ph = mk(Expr::COL, "?" + m.s("member"));
      st->gjStored.push_back({m.s("member"), ph});
      s.cols[m.at("column").s("displayName")] = ph;
   }
}
// constant single join (SingleJoinLowering, constantJoin): every tuple meets the one scattered row
void Translator::gatherConstJoin(Stream& s, const J& op) {
   StateP st = states.at(s.constState);
   Stream& b = st->in;
   separateNames(s, st, false);
   for (auto& m : op.at("mapping").arr) {
      auto it = st->members.find(m.s("member"));
      if (it == st->members.end()) throw Unsupported("gather of member '" + m.s("member") + "' that was never scattered");
      const std::string col = ensureCol(b, it->second, stripSuffix(it->first));
      it->second = mk(Expr::COL, col);
      s.cols[m.at("column").s("displayName")] = it->second;
   }
   flush(b);
   flush(s);
   s.rel = emit("join_nl", "j", {{"in", quote(s.rel)}, {"build", quote(b.rel)}, {"residual", "[]"}, {"kind", "\"inner\""}});
   s.names.insert(b.names.begin(), b.names.end());
   s.constState.clear();
}
void Translator::gatherHashJoin(Stream& s, const J& op) {
   if (s.join.probeHiv.empty()) throw Unsupported("gather outside a hash join");
   s.join.inJoinBody = true;
   StateP hiv = states.at(s.join.probeHiv);
   separateNames(s, hiv->source, !hiv->ht.empty());
   for (auto& m : op.at("mapping").arr) {
      auto it = hiv->source->members.find(m.s("member"));
      if (it == hiv->source->members.end()) throw Unsupported("gather of member '" + m.s("member") + "' that the build side did not materialise");
      auto e = std::make_shared<Expr>(*stripCast(it->second));
      if (e->kind != Expr::COL) { // a computed build column: give it a name on the build relation first
         const std::string col = ensureCol(hiv->source->in, it->second, stripSuffix(it->first));
         it->second = mk(Expr::COL, col);
         e = std::make_shared<Expr>(*it->second);
      }
      e->build = true;
      s.cols[m.at("column").s("displayName")] = e;
   }
}
void Translator::opUnion(const J& op, const std::string& ref, StepCtx& c) {
   std::vector<Stream*> ins;
   for (auto& e : op.at("outerEdges").arr)
      if (e.s("type") == "stream") {
         auto it = c.streams.find(e.at("input").s("ref"));
         if (it == c.streams.end()) throw Unsupported("stream input '" + e.at("input").s("ref") + "' is not produced in this step");
         ins.push_back(&it->second);
      }
   if (ins.size() != 2) throw Unsupported("union of " + std::to_string(ins.size()) + " streams");
   Stream* m = ins[0]->antiBranch ? ins[1] : ins[0];
   Stream* n = ins[0]->antiBranch ? ins[0] : ins[1];
   // matches (columns mapped to their nullable copies) ∪ partner-less probe rows (the same columns mapped to NULL) of ONE
   // pending hash join = a left outer join (OuterJoinLowering / SingleJoinLowering without reverseSides)
   if (m->join.pending && !m->antiBranch && !m->join.probeHiv.empty() && n->antiBranch && !n->flagState.empty() && states.count(n->flagState) &&
       states.at(m->join.probeHiv)->source == states.at(n->flagState)) {
      // OuterJoinLowering with reverseSides (:1511-1525): the probing side's matches (the preserved BUILD side carries a flag they set) ∪ the
      // build rows whose flag stayed false, the probe side's columns NULL = the inner pairs followed by the unmatched build rows
      Stream s = *m;
      s.rel = emitJoin(s, s.fullOuter ? "full_outer" : "right_outer"); // (FullOuterJoinLowering, :1446-1484: the body united the matches with the partner-less probe rows)
      s.fullOuter = false;
      const Stream& bs = states.at(s.join.probeHiv)->source->in;
      s.names.insert(bs.names.begin(), bs.names.end());
      clearJoin(s);
      s.unique.clear();
      c.streams[ref] = s;
      return;
   }
   if (!m->join.pending && !n->join.pending && !m->antiBranch && !n->antiBranch && !m->lastMapped.empty() && m->lastMapped == n->lastMapped) {
      // UnionAllLowering (:622-634): both inputs mapped to the result columns (as nullable), then united
      Stream a = *m, b = *n;
      std::vector<std::string> lc, rc;
      for (auto& name : a.lastMapped) {
         lc.push_back(ensureCol(a, a.cols.at(name), name));
         rc.push_back(ensureCol(b, b.cols.at(name), name));
      }
      flush(a);
      flush(b);
      Stream s;
      s.rel = emit("set_op", "u", {{"kind", "\"union_all\""}, {"left", quote(a.rel)}, {"left_cols", nameList(lc)}, {"right", quote(b.rel)}, {"right_cols", nameList(rc)}});
      for (size_t k = 0; k < lc.size(); k++) {
         s.cols[a.lastMapped[k]] = mk(Expr::COL, lc[k]);
         s.names.insert(lc[k]);
      }
      c.streams[ref] = s;
      return;
   }
   if (!(m->join.pending && !m->antiBranch && n->join.pending && n->antiBranch && m->join.probeHiv == n->join.probeHiv && !m->join.probeHiv.empty()))
      throw Unsupported("union of two streams that are neither the halves of an outer join nor two mapped inputs of a UNION ALL");
   Stream s = *m;
   for (auto& kv : n->cols)
      if (kv.second->kind == Expr::NULLV && !s.cols.count(kv.first)) throw Unsupported("outer join: column '" + kv.first + "' is NULL on one side and undefined on the other");
   if (!states.at(s.join.probeHiv)->source->flagMember.empty()) { // the build entries carry a flag the matches set: a FULL outer join, emitted with its third part
      s.fullOuter = true;
      c.streams[ref] = s;
      return;
   }
   s.rel = emitJoin(s, "left_outer");
   {
      const Stream& bs = states.at(s.join.probeHiv)->source->in;
      s.names.insert(bs.names.begin(), bs.names.end());
   }
   clearJoin(s);
   for (auto it = s.cols.begin(); it != s.cols.end();) it = it->second->kind == Expr::MARKER ? s.cols.erase(it) : std::next(it);
   c.streams[ref] = s;
}
void Translator::opScatter(const J& op, const std::string& ref, StepCtx& c) { // only as part of the two marker idioms of semi / anti joins
   Stream s = input(op, c);
   if (!s.gjState.empty()) { // inner group join: the matched groups get their marker set
      states.at(s.gjState)->gjInner = true;
      c.streams[ref] = s;
      return;
   }
   if (!s.join.pending && !s.aggState.empty() && s.join.probeHiv.empty()) { // constant single join: the one row of this stream becomes the state
      StateP st = states.at(s.aggState);
      if (st->kind != State::UNKNOWN) throw Unsupported("scatter into a state that is already in use");
      st->kind = State::CONST1;
      for (auto& m : op.at("mapping").arr) {
         auto it = s.cols.find(m.at("column").s("displayName"));
         if (it == s.cols.end()) throw Unsupported("scatter of an undefined column");
         st->members[m.s("member")] = it->second;
      }
      s.aggState.clear();
      st->in = s;
      c.streams[ref] = s;
      return;
   }
   if (!s.join.pending) throw Unsupported("scatter outside the marker idiom of a semi / anti join");
   for (auto& m : op.at("mapping").arr) {
      auto it = s.cols.find(m.at("column").s("displayName"));
      if (it == s.cols.end() || it->second->kind != Expr::CONST_BOOL || !it->second->i) throw Unsupported("scatter of anything but the constant true");
   }
   if (!s.aggState.empty()) { // anyTuple (RelAlgToSubOp.cpp:1296-1305): a per-probe-row marker state → semi / anti keeping the probe side
      StateP st = states.at(s.aggState);
      st->kind = State::MARKER;
      s.aggState.clear();
      st->in = s;
   } else { // translateNLWithMarker: the flag member of the matched build entry → semi / anti keeping the BUILD side
      StateP hiv = states.at(s.join.probeHiv);
      StateP buf = hiv->source;
      const std::string& member = op.at("mapping").arr.at(0).s("member");
      if (!buf->members.count(member)) throw Unsupported("scatter into member '" + member + "' that the build side did not materialise");
      if (!buf->flagMember.empty()) throw Unsupported("two joins set flags in one build buffer");
      buf->flagMember = member;
      buf->flagProbe = std::make_shared<Stream>(s); // the join is emitted when the flag is read: all_true → semi_build, all_false → anti_build
      s.join.pending = false;
   }
   c.streams[ref] = s;
}
void Translator::opUnwrapOptionalRef(const J& op, const std::string& ref, StepCtx& c) { // group join: tuples without a group are dropped — the inner join emitted for the group join does that
   Stream s = input(op, c);
   if (s.gjState.empty()) throw Unsupported("unwrap_optional_ref outside a group join");
   c.streams[ref] = s;
}

// ---------------------------------------------------------------- group joins
// GroupJoinLowering: the left input created one entry per key (its stored columns are ANY aggregates), the right input looked its
// group up and aggregated into it.  Emitted as: distinct left keys (+ stored columns) → unique hash table → the right input
// probes it (inner) → the join predicate → group by the key with the aggregates.  The inner behaviour (marker member) keeps
// exactly the groups this produces; the outer behaviour left-outer-joins the left keys with them.
struct Translator::GroupJoin {
   StateP st; // the map: AGG, reduced by the left input, looked up and aggregated into by the right one
   const J& mapping; // of the scan of the map
   std::map<std::string, std::string> storedName; // gjval member → display name
   StateP left, fin; // the distinct left keys (+ stored columns) as a buffer; the final aggregation
   std::vector<std::string> keyMembers, keyNames, bk, pk; // per key: member, display name, build column, probe column
   Stream r; // the right input, from the probe on
};
// one entry of a scan's mapping, {"member": …, "column": {"displayName": …}}, as emitGroupBy reads it
static J mappingEntry(const std::string& member, const std::string& displayName) {
   J name, column, mem, entry;
   name.kind = mem.kind = J::STR;
   name.str = displayName;
   mem.str = member;
   column.kind = entry.kind = J::OBJ;
   column.obj = {{"displayName", name}};
   entry.obj = {{"member", mem}, {"column", column}};
   return entry;
}
// an entry that follows the key entries.  These lists used to be JSON text that was parsed again, every such entry led by a comma: without a
// key entry before it the text did not parse.  A scan of the map that names no key member is still refused, as an invalid document, in those words.
static void appendAfterKeys(J& list, const std::string& member, const std::string& displayName) {
   if (list.arr.empty()) throw std::runtime_error("plan JSON: value expected near '" + (", {\"member\": " + quote(member) + ", \"column\": {\"displayName\": ").substr(0, 24) + "'");
   list.arr.push_back(mappingEntry(member, displayName));
}
// the left side: one row per key; the stored columns are functionally dependent on it and travel as further keys
// (ANY over a string has no device form, a key has)
void Translator::groupJoinLeft(GroupJoin& g) {
   const StateP& st = g.st;
   for (auto& m : g.mapping.arr)
      if (m.s("member").rfind("gjval$", 0) == 0) g.storedName[m.s("member")] = m.at("column").s("displayName");
   J lm;
   lm.kind = J::ARR;
   for (auto& m : g.mapping.arr)
      if (isKeyMember(m.s("member"))) lm.arr.push_back(mappingEntry(m.s("member"), m.at("column").s("displayName")));
   std::vector<AggSpec> keep;
   for (auto& a : st->aggs) {
      if (a.fn == "any" && g.storedName.count(a.member) && a.arg) {
         st->in.cols[g.storedName[a.member]] = a.arg;
         appendAfterKeys(lm, "keyval$" + a.member, g.storedName[a.member]);
      } else {
         keep.push_back(a);
      }
   }
   st->aggs = keep;
   if (st->aggs.empty()) {
      AggSpec a;
      a.member = "distinct$count";
      a.fn = "count_star";
      st->aggs.push_back(a);
   }
   emitGroupBy(st, lm);
   g.left = std::make_shared<State>();
   g.left->kind = State::BUFFER;
   g.left->in = st->in;
   for (auto& m : g.mapping.arr)
      if (isKeyMember(m.s("member"))) {
         g.keyMembers.push_back(m.s("member"));
         g.keyNames.push_back(m.at("column").s("displayName"));
         g.left->members[m.s("member")] = mk(Expr::COL, st->aggOut.at(m.s("member")));
      }
   for (auto& sp : st->gjStored) {
      auto it = st->aggOut.find("keyval$" + sp.first);
      if (it == st->aggOut.end()) throw Unsupported("group join gathers member '" + sp.first + "' the left input did not store");
      g.left->members[sp.first] = mk(Expr::COL, it->second);
   }
}
// the right input probes the unique table of the left keys; the group join's predicate is applied to the joined rows
void Translator::groupJoinProbe(GroupJoin& g) {
   const StateP& st = g.st;
   Stream& r = g.r = *st->gjRight;
   separateNames(r, g.left, false);
   for (auto& sp : st->gjStored) { // the placeholders handed out by the gather become the (possibly renamed) stored columns
      sp.second->name = g.left->members.at(sp.first)->name;
      sp.second->build = false;
   }
   for (size_t k = 0; k < g.keyMembers.size(); k++) {
      ExprP right;
      for (auto& pr : st->gjPairs)
         if (pr.first == g.keyNames[k]) right = pr.second;
      if (!right) throw Unsupported("group join: no renaming names the right key of '" + g.keyNames[k] + "'");
      g.bk.push_back(g.left->members.at(g.keyMembers[k])->name);
      g.pk.push_back(ensureCol(r, right, "gj_key"));
   }
   flush(g.left->in);
   const std::string ht = emit("join_build", "h", {{"in", quote(g.left->in.rel)}, {"keys", nameList(g.bk)}, {"unique", "true"}});
   flush(r);
   r.rel = emit("join_probe", "j", {{"ht", quote(ht)}, {"in", quote(r.rel)}, {"keys", nameList(g.pk)}, {"kind", "\"inner\""}});
   r.names.insert(g.left->in.names.begin(), g.left->in.names.end());
   for (auto& e : st->gjFilters) applyFilter(r, e);
}
// the final aggregation: keyed by the (right) key columns, carrying the stored columns as further keys
void Translator::groupJoinAggregate(GroupJoin& g) {
   const StateP& st = g.st;
   g.fin = std::make_shared<State>();
   g.fin->kind = State::AGG;
   g.fin->in = g.r;
   g.fin->aggs = st->gjAggs;
   J fm;
   fm.kind = J::ARR;
   for (size_t k = 0; k < g.keyMembers.size(); k++) {
      g.fin->in.cols[g.keyNames[k]] = mk(Expr::COL, g.pk[k]);
      fm.arr.push_back(mappingEntry(g.keyMembers[k], g.keyNames[k]));
   }
   for (auto& sp : st->gjStored) {
      auto sn = g.storedName.find(sp.first);
      if (sn == g.storedName.end() || !st->gjInner) continue; // gathered for the predicate only / taken from the left side (groupJoinOuter)
      g.fin->in.cols[sn->second] = sp.second;
      appendAfterKeys(fm, "keyval$" + sp.first, sn->second);
   }
   for (auto& m : g.mapping.arr)
      if (!isKeyMember(m.s("member")) && !g.storedName.count(m.s("member"))) appendAfterKeys(fm, m.s("member"), m.at("column").s("displayName"));
   emitGroupBy(g.fin, fm);
}
// outer behaviour: every left key comes out, groups without a partner with their default aggregates (count 0, the others NULL): the left
// keys (+ stored columns) left-outer-joined with their groups
Stream Translator::groupJoinOuter(GroupJoin& g) {
   const StateP &st = g.st, &fin = g.fin;
   std::vector<std::string> gk;
   for (auto& km : g.keyMembers) gk.push_back(fin->aggOut.at(km));
   Stream s = g.left->in;
   flush(fin->in);
   const std::string ht = emit("join_build", "h", {{"in", quote(fin->in.rel)}, {"keys", nameList(gk)}, {"unique", "true"}});
   s.rel = emit("join_probe", "j", {{"ht", quote(ht)}, {"in", quote(s.rel)}, {"keys", nameList(g.bk)}, {"kind", "\"left_outer\""}});
   s.names.insert(fin->in.names.begin(), fin->in.names.end());
   for (auto& m : g.mapping.arr) {
      const std::string& name = m.at("column").s("displayName");
      if (isKeyMember(m.s("member"))) {
         s.cols[name] = g.left->members.at(m.s("member"));
      } else if (g.storedName.count(m.s("member"))) {
         auto it = st->aggOut.find("keyval$" + m.s("member"));
         if (it == st->aggOut.end()) throw Unsupported("group join scans a stored member the left input did not store");
         s.cols[name] = mk(Expr::COL, it->second);
      } else {
         auto it = fin->aggOut.find(m.s("member"));
         if (it == fin->aggOut.end()) throw Unsupported("group join scans member '" + m.s("member") + "' nothing aggregates");
         ExprP v = mk(Expr::COL, it->second);
         bool counts = false;
         for (auto& a : st->gjAggs) counts = counts || (a.member == m.s("member") && (a.fn == "count" || a.fn == "count_star"));
         if (counts) { // CountAggrFunc / CountStarAggrFunc start at 0 (createDefaultValue, :1812, :1826)
            ExprP zero = mk(Expr::CONST_INT), co = mk(Expr::OP, "coalesce");
            co->args = {v, zero};
            v = co;
         }
         s.cols[name] = v;
      }
   }
   return s;
}
// inner behaviour: exactly the groups the join produced
Stream Translator::groupJoinInner(GroupJoin& g) {
   Stream s = g.fin->in;
   for (auto& m : g.mapping.arr) {
      auto it = g.fin->aggOut.find(g.storedName.count(m.s("member")) ? "keyval$" + m.s("member") : m.s("member"));
      if (it == g.fin->aggOut.end()) { // the marker member: every group here has a partner
         ExprP t = mk(Expr::CONST_BOOL);
         t->i = 1;
         s.cols[m.at("column").s("displayName")] = t;
         continue;
      }
      ExprP c2 = mk(Expr::COL, it->second);
      c2->dtype = m.at("column").sOr("datatype", "");
      s.cols[m.at("column").s("displayName")] = c2;
   }
   return s;
}
Stream Translator::scanGroupJoin(const StateP& st, const J& mapping) {
   GroupJoin g{st, mapping, {}, nullptr, nullptr, {}, {}, {}, {}, {}};
   groupJoinLeft(g);
   groupJoinProbe(g);
   groupJoinAggregate(g);
   return st->gjInner ? groupJoinInner(g) : groupJoinOuter(g);
}

// ---------------------------------------------------------------- set operations
// the set operation whose counting map `s` scans: distinct kinds keep one row per key, the ALL kinds min(c1, c2) / max(c1 - c2, 0) rows
void Translator::emitSetOp(Stream& s, const std::string& kind) {
   StateP st = states.at(s.setState);
   flush(st->in);
   flush(*st->setRight);
   s.rel = emit("set_op", "u", {{"kind", quote(kind)}, {"left", quote(st->in.rel)}, {"left_cols", nameList(st->setLeftCols)}, {"right", quote(st->setRight->rel)}, {"right_cols", nameList(st->setRightCols)}});
   s.setState.clear();
   for (auto it = s.cols.begin(); it != s.cols.end();)
      it = it->second->kind == Expr::SETCNT || (it->second->kind == Expr::OP && it->second->name == "setop") ? s.cols.erase(it) : std::next(it);
}
// what a map over the two counters computes (CountingSetOperationLowering, :868-915; arith.cmpi / andi / subi / select: emitter extension E7)
std::string classifySet(const ExprP& e0) {
   const ExprP e = stripCast(e0);
   auto cnt = [](const ExprP& x, int which) { return stripCast(x)->kind == Expr::SETCNT && stripCast(x)->i == which; };
   auto zero = [](const ExprP& x) { return stripCast(x)->kind == Expr::CONST_INT && stripCast(x)->i == 0; };
   auto diff = [&](const ExprP& x) { return stripCast(x)->kind == Expr::OP && stripCast(x)->name == "sub" && cnt(stripCast(x)->args[0], 1) && cnt(stripCast(x)->args[1], 2); };
   if (e->kind != Expr::OP) return "";
   if (e->name == "and" && e->args.size() == 2) {
      const ExprP l = stripCast(e->args[0]), r = stripCast(e->args[1]);
      if (l->kind == Expr::OP && l->name == "cmp" && l->cmp == "GT" && cnt(l->args[0], 1) && zero(l->args[1]) && r->kind == Expr::OP && r->name == "cmp" && cnt(r->args[0], 2) && zero(r->args[1]))
         return r->cmp == "GT" ? "intersect" : r->cmp == "EQ" ? "except" : "";
   }
   if (e->name == "select" && e->args.size() == 3) {
      const ExprP c = stripCast(e->args[0]);
      if (c->kind == Expr::OP && c->name == "cmp" && c->cmp == "LT" && diff(c->args[0]) && zero(c->args[1]) && zero(e->args[1]) && diff(e->args[2])) return "except_all";
      if (c->kind == Expr::OP && c->name == "cmp" && c->cmp == "GT" && cnt(c->args[0], 1) && cnt(c->args[1], 2) && cnt(e->args[1], 2) && cnt(e->args[2], 1)) return "intersect_all";
   }
   return "";
}
Stream Translator::scanSetOp(const StateP& st, const J& mapping, StepCtx& c) { // the map both inputs of a set operation counted into
   Stream s;
   Stream &a = st->in, &b = *st->setRight;
   st->setLeftCols.clear();
   st->setRightCols.clear();
   std::vector<std::string> names;
   for (auto& m : mapping.arr) {
      if (m.s("member").rfind("keyval", 0) != 0) continue;
      const std::string& name = m.at("column").s("displayName");
      auto ia = a.cols.find(name), ib = b.cols.find(name);
      if (ia == a.cols.end() || ib == b.cols.end()) throw Unsupported("set operation: column '" + name + "' is not defined on both inputs");
      st->setLeftCols.push_back(ensureCol(a, ia->second, name));
      st->setRightCols.push_back(ensureCol(b, ib->second, name));
      names.push_back(name);
   }
   if (names.empty()) throw Unsupported("set operation without columns");
   for (size_t k = 0; k < names.size(); k++) {
      s.cols[names[k]] = mk(Expr::COL, st->setLeftCols[k]);
      s.names.insert(st->setLeftCols[k]);
   }
   s.setState = idOf(st, c);
   if (st->setLeftCounter.empty()) {
      emitSetOp(s, "union"); // UnionDistinctLowering: the keys of the map are the result
   } else {
      for (auto& m : mapping.arr) {
         const int which = m.s("member") == st->setLeftCounter ? 1 : m.s("member") == st->setRightCounter ? 2 : 0;
         if (!which) continue;
         ExprP cnt = mk(Expr::SETCNT);
         cnt->i = which;
         s.cols[m.at("column").s("displayName")] = cnt;
      }
   }
   return s;
}

// ---------------------------------------------------------------- windows
static ExprP wref(const char* what, int64_t k = 0) {
   ExprP r = mk(Expr::REF, what);
   r->i = k;
   return r;
}
static int64_t frameEnd(const ExprP& r) { // a reference into the continuous view as a frame end: offset from the current row, or unbounded
   if (r->kind != Expr::REF) throw Unsupported("window frame end that is not a view reference");
   if (r->name == "w:begin") return INT64_MIN;
   if (r->name == "w:end") return INT64_MAX;
   if (r->name == "w:cur") return 0;
   if (r->name == "w:off") return r->i;
   throw Unsupported("window frame end that is not a view reference");
}
void Translator::setFrame(Stream& s, int64_t from, int64_t to, bool haveTo) {
   if (s.win.frame && (s.win.from != from || (haveTo && s.win.hasTo && s.win.to != to))) throw Unsupported("window functions with different frames in one window");
   if (!s.win.frame) s.win.to = 0; // (a rank alone reads only the frame's begin)
   s.win.frame = true;
   s.win.from = from;
   if (haveTo) {
      s.win.to = to;
      s.win.hasTo = true;
   }
}
// the functions collected on this stream become ONE window step: partition + order of the view, one frame, one result column each
void Translator::flushWindow(Stream& s) {
   if (s.win.fns.empty()) return;
   StateP view = states.at(s.win.view);
   flush(s);
   auto end = [](int64_t v) { return v == INT64_MIN ? std::string("\"unbounded_preceding\"") : v == INT64_MAX ? std::string("\"unbounded_following\"") : std::to_string(v); };
   Fields w = {{"in", quote(s.rel)}};
   if (!view->partCols.empty()) w.push_back({"partition_by", nameList(view->partCols)});
   if (!view->sortCols.empty()) {
      std::vector<std::string> by;
      for (auto& k : view->sortCols) by.push_back(sortKey(k.first, k.second));
      w.push_back({"order_by", joined(by)});
   }
   w.push_back({"frame_from", end(s.win.from)});
   w.push_back({"frame_to", end(s.win.to)});
   std::vector<std::string> fns;
   for (auto& f : s.win.fns) {
      fns.push_back("{\"fn\": " + quote(f.fn) + (f.col.empty() ? "" : ", \"col\": " + quote(f.col)) + ", \"as\": " + quote(f.as) + "}");
      s.names.insert(f.as);
   }
   w.push_back({"fns", joined(fns)});
   s.rel = emit("window", "w", w);
   s.bareTable = false;
   s.unique.clear();
   Stream::Window done;
   done.staticView = s.win.staticView; // (the mark of a whole-partition scan is not part of the evaluation that ends here)
   s.win = done;
}
// a lookup that reads the aggregates of the frame of the window being evaluated on `s` (false: another kind of lookup)
bool Translator::lookupWindow(Stream& s, const StateP& st, const std::string& id, const J& op) {
   const std::string stateType = op.sOr("stateType", "");
   const char* what;
   if (stateType == "SimpleState" && st->kind == State::AGG && !s.win.view.empty() && st->in.win.staticView == s.win.view) {
      // the whole partition's aggregates, computed once by a scan of the view (frame UNBOUNDED PRECEDING … UNBOUNDED FOLLOWING)
      what = "w:static";
   } else if (stateType == "SegmentTreeView") { // the aggregates of the frame [keys[0], keys[1]] (the keys: emitter extension E8)
      const J* keys = op.get("keys");
      if (st->kind != State::SEGTREE || s.win.view.empty() || !keys || keys->arr.size() != 2) throw Unsupported("segment-tree lookup without its frame references (emitter extension E8)");
      auto b = s.cols.find(keys->arr[0].s("displayName")), e = s.cols.find(keys->arr[1].s("displayName"));
      if (b == s.cols.end() || e == s.cols.end()) throw Unsupported("segment-tree lookup through undefined references");
      setFrame(s, frameEnd(b->second), frameEnd(e->second), true);
      what = "w:lookup";
   } else {
      return false;
   }
   states[id] = st;
   s.win.lookup = id;
   s.cols[op.at("reference").s("displayName")] = wref(what);
   return true;
}
void Translator::opScanRef(const J& op, const std::string& ref, StepCtx& c) { // every entry of the continuous view, by reference
   StateP st = resolve(op.at("accesses").arr.at(0), c);
   if (st->kind != State::CONTVIEW) throw Unsupported("scan_ref over a state that is not a continuous view");
   Stream s = c.nested && !st->partCols.empty() ? *c.nested : st->in;
   s.win.view = idOf(st, c);
   s.cols[op.at("reference").s("displayName")] = wref("w:cur");
   c.streams[ref] = s;
}
void Translator::opFrameReference(const J& op, const std::string& ref, StepCtx& c) {
   const std::string& kind = op.s("subop"); // get_begin_reference | get_end_reference
   Stream s = input(op, c);
   if (s.win.view.empty()) throw Unsupported(kind + " outside a window evaluation");
   s.cols[op.at("reference").s("displayName")] = wref(kind == "get_begin_reference" ? "w:begin" : "w:end");
   c.streams[ref] = s;
}
void Translator::opOffsetReferenceBy(const J& op, const std::string& ref, StepCtx& c) { // ROWS k PRECEDING / FOLLOWING: the current reference moved by a constant, clamped into the partition
   Stream s = input(op, c);
   auto r = s.cols.find(op.at("reference").s("displayName"));
   auto o = s.cols.find(op.at("offset").s("displayName"));
   if (s.win.view.empty() || r == s.cols.end() || r->second->kind != Expr::REF || r->second->name != "w:cur" || o == s.cols.end() || stripCast(o->second)->kind != Expr::CONST_INT)
      throw Unsupported("offset_reference_by that does not move the current row of a window by a constant");
   s.cols[op.at("newRef").s("displayName")] = wref("w:off", stripCast(o->second)->i);
   c.streams[ref] = s;
}
void Translator::opEntriesBetween(const J& op, const std::string& ref, StepCtx& c) { // RankWindowFunc (:2043-2058): entries between the frame begin and the current row
   Stream s = input(op, c);
   auto l = s.cols.find(op.at("leftRef").s("displayName"));
   auto r = s.cols.find(op.at("rightRef").s("displayName"));
   if (s.win.view.empty() || l == s.cols.end() || r == s.cols.end() || r->second->kind != Expr::REF || r->second->name != "w:cur") throw Unsupported("entries_between that does not end at the current row of a window");
   ExprP b = mk(Expr::OP, "wbetween");
   b->i = frameEnd(l->second);
   s.cols[op.at("between").s("displayName")] = b;
   c.streams[ref] = s;
}
Stream Translator::scanContinuousView(const StateP& st, const J& mapping, StepCtx& c) { // every row of the (partition's) view once: the static aggregation of an UNBOUNDED … UNBOUNDED frame (:2497-2499)
   Stream s = c.nested && !st->partCols.empty() ? *c.nested : st->in;
   for (auto& m : mapping.arr) {
      auto it = st->members.find(m.s("member"));
      if (it == st->members.end()) throw Unsupported("scan of member '" + m.s("member") + "' that was never materialised");
      s.cols[m.at("column").s("displayName")] = it->second;
   }
   s.win.staticView = idOf(st, c);
   return s;
}
Stream Translator::scanPartitionMap(const StateP& st, const J& mapping, StepCtx& c) { // the map keyed by the PARTITION BY columns whose value is the partition's buffer
   st->partCols.clear();
   for (auto& m : mapping.arr) {
      const std::string& name = m.at("column").s("displayName");
      if (!isKeyMember(m.s("member"))) continue;
      auto it = st->in.cols.find(name);
      if (it == st->in.cols.end()) throw Unsupported("partition key '" + name + "' is not a column of the windowed stream");
      st->partCols.push_back(ensureCol(st->in, it->second, name));
   }
   Stream s = st->in; // (after the keys: ensureCol may have added columns)
   for (auto& m : mapping.arr)
      if (!isKeyMember(m.s("member"))) s.cols[m.at("column").s("displayName")] = wref("w:partbuf");
   s.partState = idOf(st, c);
   return s;
}

} // namespace ldbsubop
