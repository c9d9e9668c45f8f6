// eg_refine.cpp — eg_refine_plan and eg_refine_plans (include/eirgrid_hip.h): the loop "score every one-entry edit of a plan, apply the
// best one" with the plans, their variants and the pick of each winner on the device.  ONE loop serves both: eg_refine_plan is its case of
// one plan.  Per round the still-active plans' variants are packed into launches, a SEGMENT of consecutive variants per plan;
// k_plan_edits_many writes every variant's block from its plan's base block, the plan batch runs over the whole launch (eg_plans.cpp:
// stage_eval_snapshot, launch_plans, write_plan_blocks), k_refine_pick_many picks a winner per segment and keeps that plan's base
// block current (eg_refine_many.h; the packing and the launch are eg_plan_host.cpp's pack_neighbourhood and launch_variants).  The host
// follows every plan in a mirror, from which the next round's edits are enumerated.
// A plan never straddles two launches, so a single plan always gets a launch of exactly its own variants, whatever the launch size.
// eg_refine_plans_moves runs the same loop with move variants behind every plan's edits: k_plan_moves (eg_plan_moves.h) overwrites their
// blocks behind k_plan_edits_many, which has written a copy of the base for them.
// eg_repair_plans runs the same loop with another RULE: which kernel picks a segment's winner, what its entry says of the base, and what a
// winner means — a step, a stop, both.  RefineRule is the largest score (k_refine_pick_many); RepairRule the smallest violation of the
// context's plan constraints below the base's (eg_repair.h k_repair_pick_many), its weights uploaded behind the launch's segment table.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "eg_edit_order.h"
#include "eg_host.h"

using namespace eg;

namespace {
// a plan as the host follows it: the two lists, year by year
struct Mirror {
  std::vector<uint8_t> l[2][EG_YEARS];
  int64_t total(int w) const { int64_t n = 0; for (int y = 0; y < EG_YEARS; ++y) n += int64_t(l[w][y].size()); return n; }
  void counts(int32_t (&count)[2][EG_YEARS]) const {
    for (int w = 0; w < 2; ++w)
      for (int y = 0; y < EG_YEARS; ++y) count[w][y] = int32_t(l[w][y].size());
  }
};
// the plans of a valid set as mirrors, and the reverse (the set's names carried over)
std::vector<Mirror> mirrors_of(const eg_plan_set* p) {
  std::vector<Mirror> mirror((size_t(p->n_plans)));
  const int32_t* count[2] = {p->best_count, p->best_deficit_count};
  const uint8_t* flat[2] = {p->best_actions, p->best_deficit_actions};
  for (int w = 0; w < 2; ++w) {
    size_t at = 0;      // (k: the year-lists of the set, plan-major)
    for (size_t k = 0; k < mirror.size() * EG_YEARS; at += size_t(count[w][k]), ++k)
      mirror[k / EG_YEARS].l[w][k % EG_YEARS].assign(flat[w] + at, flat[w] + at + count[w][k]);
  }
  return mirror;
}
eg_plan_set* set_of(const std::vector<Mirror>& mirror, const char* const* names) {
  std::vector<int32_t> count[2];
  std::vector<uint8_t> flat[2];
  for (int w = 0; w < 2; ++w) {
    for (const Mirror& m : mirror)
      for (const std::vector<uint8_t>& l : m.l[w]) { count[w].push_back(int32_t(l.size())); flat[w].insert(flat[w].end(), l.begin(), l.end()); }
    flat[w].reserve(1);
  }
  return make_plan_set_n(int32_t(mirror.size()), count[0].data(), flat[0].data(), count[1].data(), flat[1].data(), names);
}
// variants of a round over lists of these totals (include/eirgrid_hip.h: none, deletes, replaces, appends)
int64_t n_variants(int64_t len0, int64_t len1, const eg_refine_opts& o) {
  return 1 + len0 + len1 + int64_t(o.n_replace) * len0 + (len0 < int64_t(snap::kBestCap) ? int64_t(EG_YEARS) * o.n_append : 0);
}
// ... and with the move variants behind them (eg_refine_plans_moves; mo == NULL: none); count0: the years' best_actions lengths
int64_t n_variants(const int32_t* count0, int64_t len0, int64_t len1, const eg_refine_opts& o, const eg_refine_move_opts* mo) {
  return n_variants(len0, len1, o) + (mo ? count_moves(count0, mo->max_shift) : 0);
}
void apply(Mirror& m, const eg_plan_edit& e) {
  std::vector<uint8_t>& l = m.l[e.list][e.year];
  if (e.kind == EG_EDIT_DELETE) l.erase(l.begin() + e.pos);
  else if (e.kind == EG_EDIT_REPLACE) l[e.pos] = e.action;
  else if (e.kind == EG_EDIT_INSERT) l.insert(l.begin() + e.pos, e.action);
}
void apply(Mirror& m, const eg_plan_move& v) {
  std::vector<uint8_t>& from = m.l[v.list][v.year];
  const uint8_t a = from[v.pos];
  from.erase(from.begin() + v.pos);
  std::vector<uint8_t>& to = m.l[v.list][v.to_year];
  to.insert(to.begin() + v.to_pos, a);
}
// who speaks in a message: the entry point `fn`, and the plan where the entry point takes many (the one-plan forms name none)
std::string who(const char* fn, bool name_plan, int32_t plan) { return std::string(fn) + ": " + (name_plan ? "plan " + std::to_string(plan) + ": " : ""); }
std::string too_many(int round, int64_t n) {
  return "round " + std::to_string(round) + " enumerates " + std::to_string(n) + " variants (at most " + std::to_string(EG_REFINE_MAX_VARIANTS) + ")";
}
// what both validators ask of the options, and of every plan's round 0 (the set itself is the caller's to check)
int32_t validate_opts(const char* fn, bool name_plan, const eg_plan_set* bases, const eg_refine_opts* o, const eg_refine_move_opts* mo = nullptr) {
  auto fail = [fn](const std::string& m) { set_error(std::string(fn) + ": " + m); return EG_ERR_BAD_ARG; };
  if (!o) return fail("NULL options");
  if (o->mode != 1 && o->mode != 2) return fail("mode " + std::to_string(o->mode) + " (1: optimization_mode None, 2: cost_only)");
  if (o->max_rounds < 1) return fail("max_rounds = " + std::to_string(o->max_rounds) + " (at least 1)");
  EG_TRY(validate_action_lists(fail, o->n_replace, o->replace_with, o->n_append, o->append_with));
  for (int32_t p = 0; p < bases->n_plans; ++p) {
    int64_t len[2] = {0, 0};
    for (int y = 0; y < EG_YEARS; ++y) { len[0] += bases->best_count[size_t(p) * EG_YEARS + y]; len[1] += bases->best_deficit_count[size_t(p) * EG_YEARS + y]; }
    const int64_t n = n_variants(bases->best_count + size_t(p) * EG_YEARS, len[0], len[1], *o, mo);
    if (n > EG_REFINE_MAX_VARIANTS) { set_error(who(fn, name_plan, p) + too_many(0, n)); return EG_ERR_BAD_ARG; }
  }
  return EG_OK;
}
// what the two many-plan validators ask of the set
int32_t validate_set(const char* fn, const eg_plan_set* bases) {
  EG_TRY(eg_plans_validate(bases));
  if (bases->n_plans <= EG_REFINE_MAX_PLANS) return EG_OK;
  set_error(std::string(fn) + ": the set holds " + std::to_string(bases->n_plans) + " plans (at most " + std::to_string(EG_REFINE_MAX_PLANS) + ")");
  return EG_ERR_BAD_ARG;
}
// EIRGRID_REFINE_LAUNCH_VARIANTS: the variants a launch may hold (a plan with more gets a launch to itself), read at every call
uint32_t launch_variants() {
  const char* v = std::getenv("EIRGRID_REFINE_LAUNCH_VARIANTS");
  if (!v || !*v) return EG_REFINE_MAX_VARIANTS;
  return uint32_t(std::min<long long>(std::max<long long>(std::atoll(v), 1), EG_REFINE_MAX_VARIANTS));
}
// one plan of a launch: its variants are [first, first + n) of the launch's
// (with moves: its edits, then its moves)
struct Seg { int32_t plan; uint32_t first, n; std::vector<eg_plan_edit> edits; std::vector<eg_plan_move> moves; };

// What a rule is given of a winner: where its step goes, and the edit or move it is (against the plan of its round)
struct Won { size_t at; bool is_move; const eg_plan_edit* edit; const eg_plan_move* move; int32_t n_variants; };
constexpr int kGoOn = -1;      // (a rule's verdict: the plan stays in the search)

// eg_refine_plan, eg_refine_plans, eg_refine_plans_moves: the largest score; a winner that is the base is a local optimum
struct RefineRule {
  using Entry = RefineEntry;
  static_assert(EG_REFINE_BASE_FAILED == 2 && EG_REFINE_MAX_ROUNDS == 1, "the loop's two own stop reasons");
  eg_refine_step* steps; eg_refine_move_step* msteps;      // (with moves the steps go to msteps)
  double* start_score;
  size_t extra_bytes() const { return 0; }
  void extra(uint8_t*) const {}
  void begin(int32_t p) const { if (start_score) start_score[p] = std::nan(""); }
  void base(int32_t p, const Entry& e) const { if (start_score && e.base_ok) start_score[p] = e.base_score; }
  int launch(eg_ctx* c, size_t at_segs, size_t, uint32_t n_segs, uint32_t n, int mode, uint32_t P) const {
    EG_LAUNCH("k_refine_pick_many", launch_refine_pick_many(c->out, c->d_refine_in + at_segs, n_segs, n, mode, c->d_refine_in, c->d_plans, c->d_refine_bases, P,
                                                            c->d_refine_log, nullptr));
    return EG_OK;
  }
  // the stop reason when the winner is the base; otherwise the step is recorded and the loop counts it
  int stays(int32_t, const Entry&) const { return EG_REFINE_LOCAL_OPTIMUM; }
  int step(int32_t, const Entry& e, const Won& w) const {
    if (msteps) {
      eg_refine_move_step& st = msteps[w.at];
      std::memset(&st, 0, sizeof(st));
      st.is_move = w.is_move ? 1 : 0;
      if (w.is_move) st.move = *w.move; else st.edit = *w.edit;
      st.variant = e.winner; st.n_variants = w.n_variants; st.n_failed = e.n_failed; st.score = e.score;
      std::memcpy(st.metrics, e.metrics, sizeof(st.metrics));
    } else {
      eg_refine_step& st = steps[w.at];
      st.edit = *w.edit; st.variant = e.winner; st.n_variants = w.n_variants; st.n_failed = e.n_failed; st.score = e.score;
      std::memcpy(st.metrics, e.metrics, sizeof(st.metrics));
    }
    return kGoOn;
  }
};

// eg_repair_plans: the smallest violation below the base's; a base that stays is feasible or stuck, a winner at V == 0 ends the descent
struct RepairRule {
  using Entry = RepairEntry;
  static_assert(EG_REPAIR_BASE_FAILED == EG_REFINE_BASE_FAILED && EG_REPAIR_MAX_ROUNDS == EG_REFINE_MAX_ROUNDS, "the loop's two own stop reasons");
  eg_repair_step* steps;
  double* start_violation; double* final_violation;
  std::vector<double> weights;      // k of them: the context's constraints at the call
  size_t extra_bytes() const { return sizeof(double) * weights.size(); }
  void extra(uint8_t* at) const { std::memcpy(at, weights.data(), extra_bytes()); }
  void begin(int32_t p) const {
    if (start_violation) start_violation[p] = std::nan("");
    if (final_violation) final_violation[p] = std::nan("");
  }
  void base(int32_t p, const Entry& e) const {
    if (!e.base_ok) return;
    if (start_violation) start_violation[p] = e.base_violation;
    if (final_violation) final_violation[p] = e.base_violation;
  }
  int launch(eg_ctx* c, size_t at_segs, size_t at_extra, uint32_t n_segs, uint32_t n, int mode, uint32_t P) const {
    if (c->feas_k != int(weights.size())) { set_error("eg_repair_plans: the launch was judged under " + std::to_string(c->feas_k) + " constraints, the call began under " + std::to_string(weights.size())); return EG_ERR_INTERNAL; }
    EG_LAUNCH("k_repair_pick_many", launch_repair_pick_many(c->out, c->d_refine_in + at_segs, n_segs, n, mode, c->d_refine_in, c->d_plans, c->d_refine_bases, P,
                                                            c->d_violated, c->d_excess, uint32_t(c->feas_k), reinterpret_cast<const double*>(c->d_refine_in + at_extra),
                                                            c->d_refine_log, nullptr));
    return EG_OK;
  }
  int stays(int32_t, const Entry& e) const { return e.base_violation == 0.0 ? EG_REPAIR_FEASIBLE : EG_REPAIR_STUCK; }
  int step(int32_t p, const Entry& e, const Won& w) const {
    eg_repair_step& st = steps[w.at];
    std::memset(&st, 0, sizeof(st));
    st.is_move = w.is_move ? 1 : 0;
    if (w.is_move) st.move = *w.move; else st.edit = *w.edit;
    st.variant = e.winner; st.n_variants = w.n_variants; st.n_failed = e.n_failed; st.n_feasible = e.n_feasible;
    st.violated = e.violated; st.violation = e.violation; st.score = e.score;
    std::memcpy(st.metrics, e.metrics, sizeof(st.metrics));
    if (final_violation) final_violation[p] = e.violation;
    return e.violation == 0.0 ? EG_REPAIR_FEASIBLE : kGoOn;      // (checked ahead of max_rounds)
  }
};

// the loop, for the validated plans of `bases` under `rule`: the rule's steps [P][max_rounds], n_steps / stop_reason / out's rows [P].
// mo: the move variants behind every plan's edits (eg_refine_plans_moves, eg_repair_plans); NULL: none
template <typename Rule>
int32_t search(const Rule& rule, const char* fn, bool name_plan, eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* bases,
               const eg_refine_opts* ro, uint64_t seed, uint64_t episode_index, eg_plan_set** refined, int32_t* n_steps, int32_t* stop_reason, eg_episode_out* out,
               const eg_refine_move_opts* mo = nullptr) {
  using Entry = typename Rule::Entry;
  static_assert(sizeof(Entry) <= kRefineEntryStride, "an entry takes a slot of the step log");
  *refined = nullptr;
  const int32_t P = bases->n_plans;
  std::vector<Mirror> mirror = mirrors_of(bases);
  // every buffer once, for the largest launch max_rounds steps can lead to: a plan's best_actions grows by an entry a step at most, and
  // only by an append (a round beyond EG_REFINE_MAX_VARIANTS is refused when it is reached); a launch holds a plan larger than the
  // launch size alone, else no more variants than the launch size
  const uint32_t launch_max = launch_variants();
  uint32_t n_cap = 0;
  {
    int64_t largest = 0, sum = 0;
    for (int32_t p = 0; p < P; ++p) {
      const int64_t len0 = mirror[size_t(p)].total(0), len1 = mirror[size_t(p)].total(1);
      const int64_t grown = ro->n_append > 0 ? std::min<int64_t>(len0 + ro->max_rounds, int64_t(snap::kBestCap)) : len0;
      // (moves: at most 2 * max_shift per entry, wherever the steps take the entries)
      const int64_t moves_most = mo ? grown * 2 * mo->max_shift : 0;
      const int64_t most = std::min<int64_t>(std::max(n_variants(len0, len1, *ro), 1 + grown + len1 + int64_t(ro->n_replace) * grown + int64_t(EG_YEARS) * ro->n_append) + moves_most,
                                             EG_REFINE_MAX_VARIANTS);
      largest = std::max(largest, most); sum += most;
    }
    n_cap = uint32_t(std::max(largest, std::min<int64_t>(sum, launch_max)));
  }
  const size_t segs_cap = std::min<size_t>(size_t(P), n_cap);
  EG_TRY(ensure_outputs(c, n_cap));
  EG_HIP(c->d_plans.reserve(size_t(n_cap) * snap::kPlanStride));
  EG_HIP(c->d_plan_index.reserve(n_cap));
  EG_HIP(c->d_refine_in.reserve(size_t(n_cap) * 12 + 16 + segs_cap * kRefineSegmentBytes + rule.extra_bytes()));
  EG_HIP(c->d_refine_log.reserve(size_t(kRefineLog) * kRefineEntryStride));
  static_assert(EG_REFINE_MAX_PLANS <= kRefineLog, "a launch's entries fit the step log");
  EG_HIP(c->d_refine_bases.reserve(size_t(P) * snap::kPlanStride));
  {      // the base blocks go up once; from then on k_refine_pick_many keeps them current
    std::vector<uint8_t> blocks(size_t(P) * snap::kPlanStride, 0);
    write_plan_blocks(bases, blocks.data());
    EG_HIP(hipMemcpy(c->d_refine_bases, blocks.data(), blocks.size(), hipMemcpyHostToDevice));
  }
  DevSnapshot S{};
  EG_TRY(stage_eval_snapshot(c, s, o, &S));
  std::vector<char> active(size_t(P), 1);
  for (int32_t p = 0; p < P; ++p) { n_steps[p] = 0; stop_reason[p] = EG_REFINE_MAX_ROUNDS; rule.begin(p); }
  std::vector<Seg> segs;
  std::vector<uint8_t> in, entries;
  Routing R;
  for (int round = 0;; ++round) {
    // the round's variant counts, plan by plan
    std::vector<std::pair<int32_t, uint32_t>> todo;      // (plan, variants), ascending
    for (int32_t p = 0; p < P; ++p) {
      if (!active[size_t(p)]) continue;
      int32_t count[2][EG_YEARS];
      mirror[size_t(p)].counts(count);
      const int64_t want = n_variants(count[0], mirror[size_t(p)].total(0), mirror[size_t(p)].total(1), *ro, mo);
      if (want > EG_REFINE_MAX_VARIANTS) { set_error(who(fn, name_plan, p) + too_many(round, want)); return EG_ERR_BAD_ARG; }
      todo.emplace_back(p, uint32_t(want));
    }
    if (todo.empty()) break;
    for (size_t t0 = 0; t0 < todo.size();) {
      // a launch: consecutive plans while they fit; a plan never straddles two launches
      size_t t1 = t0 + 1;
      uint32_t n = todo[t0].second;
      while (t1 < todo.size() && n + todo[t1].second <= launch_max) n += todo[t1++].second;
      const uint32_t n_segs = uint32_t(t1 - t0);
      if (n > n_cap || n_segs > segs_cap) { set_error(std::string(fn) + ": round " + std::to_string(round) + ": a launch of " + std::to_string(n) + " variants outgrew its buffers"); return EG_ERR_INTERNAL; }
      // what goes up in one copy: the packed edits (8 bytes a variant), every variant's base slot, the segment table, what the rule adds;
      // and the routing — the short variants of the whole launch first, then the long ones (launch_plans)
      const size_t at_slot = size_t(n) * 8, at_segs = (size_t(n) * 12 + 15) / 16 * 16, at_extra = at_segs + size_t(n_segs) * kRefineSegmentBytes;
      in.assign(at_extra + rule.extra_bytes(), 0);
      rule.extra(in.data() + at_extra);
      uint32_t* packed = reinterpret_cast<uint32_t*>(in.data());
      uint32_t* slot = reinterpret_cast<uint32_t*>(in.data() + at_slot);
      uint32_t* table = reinterpret_cast<uint32_t*>(in.data() + at_segs);
      segs.resize(n_segs); R.clear();
      uint32_t first = 0;
      bool any_moves = false;
      for (uint32_t k = 0; k < n_segs; ++k) {
        Seg& sg = segs[k];
        sg.plan = todo[t0 + k].first; sg.first = first; sg.n = todo[t0 + k].second;
        const Mirror& m = mirror[size_t(sg.plan)];
        int32_t count[2][EG_YEARS];
        m.counts(count);
        enumerate_edits(count[0], count[1], ro->replace_with, ro->n_replace, ro->append_with, ro->n_append, m.total(0) < int64_t(snap::kBestCap), sg.edits);
        sg.moves.clear();
        if (mo) enumerate_moves(count[0], mo->max_shift, sg.moves);
        if (sg.edits.size() + sg.moves.size() != size_t(sg.n)) { set_error(who(fn, name_plan, sg.plan) + "round " + std::to_string(round) + ": the enumeration and its count disagree"); return EG_ERR_INTERNAL; }
        if (pack_neighbourhood(uint32_t(sg.plan), m.total(0), sg.edits.data(), uint32_t(sg.edits.size()), sg.moves.data(), uint32_t(sg.moves.size()), first, packed, slot, R))
          any_moves = true;
        table[4 * k] = first; table[4 * k + 1] = sg.n; table[4 * k + 2] = uint32_t(sg.plan);
        first += sg.n;
      }
      EG_TRY(launch_variants(c, S, c->d_refine_bases, uint32_t(P), in, at_slot, n, R, any_moves, seed, episode_index));
      EG_TRY(rule.launch(c, at_segs, at_extra, n_segs, n, ro->mode, uint32_t(P)));
      entries.resize(size_t(n_segs) * kRefineEntryStride);
      EG_HIP(hipMemcpy(entries.data(), c->d_refine_log, entries.size(), hipMemcpyDeviceToHost));      // (waits for the launch)
      for (uint32_t k = 0; k < n_segs; ++k) {
        const Seg& sg = segs[k];
        const int32_t p = sg.plan;
        const std::string at = who(fn, name_plan, p) + "round " + std::to_string(round) + ": ";
        Mirror& m = mirror[size_t(p)];
        Entry e{};
        std::memcpy(&e, entries.data() + size_t(k) * kRefineEntryStride, sizeof(e));
        if (round == 0) rule.base(p, e);
        if (!e.base_ok) { stop_reason[p] = EG_REFINE_BASE_FAILED; active[size_t(p)] = 0; continue; }
        const uint32_t* mine = packed + 2 * size_t(sg.first);
        if (e.n != int32_t(sg.n) || e.winner < 0 || e.winner >= int32_t(sg.n) || e.edit[0] != mine[2 * size_t(e.winner)] || e.edit[1] != mine[2 * size_t(e.winner) + 1]) {
          set_error(at + "the device's step entry does not name a variant of the " + (name_plan ? "plan's " : "") + "round");
          return EG_ERR_INTERNAL;
        }
        // the plan on the device against the mirror: the totals of the winner's block
        const bool is_move = size_t(e.winner) >= sg.edits.size();
        if (is_move) apply(m, sg.moves[size_t(e.winner) - sg.edits.size()]);
        else if (e.winner != 0) apply(m, sg.edits[size_t(e.winner)]);
        if (e.off26 != int32_t(m.total(0)) || e.offd26 != int32_t(m.total(1))) {
          set_error(at + "the device's plan holds " + std::to_string(e.off26) + " + " + std::to_string(e.offd26) + " entries, the host's " +
                    std::to_string(m.total(0)) + " + " + std::to_string(m.total(1)));
          return EG_ERR_INTERNAL;
        }
        int stop = kGoOn;
        if (e.winner == 0) stop = rule.stays(p, e);
        else {
          const Won won{size_t(p) * size_t(ro->max_rounds) + size_t(n_steps[p]), is_move, is_move ? nullptr : &sg.edits[size_t(e.winner)],
                        is_move ? &sg.moves[size_t(e.winner) - sg.edits.size()] : nullptr, int32_t(sg.n)};
          stop = rule.step(p, e, won);
          if (++n_steps[p] == ro->max_rounds && stop == kGoOn) stop = EG_REFINE_MAX_ROUNDS;
        }
        if (stop != kGoOn) { stop_reason[p] = stop; active[size_t(p)] = 0; }
        if (!active[size_t(p)] && out) {      // the refined plan's record, before the next launch overwrites the records
          eg_episode_out row = out_row(out, size_t(p));
          EG_TRY(fetch_records(c->out.base + (size_t(sg.first) + size_t(e.winner)) * rec::stride, 1, &row));
          if (row.status && row.status[0] == EG_EP_INTERNAL) {      // (eg_refine_plan has always reported this one without a prefix)
            set_error((name_plan ? at : std::string()) + "k_rollout: helper-wave protocol timed out in the refined plan's episode (EG_EP_INTERNAL)");
            return EG_ERR_INTERNAL;
          }
        }
      }
      t0 = t1;
    }
  }
  *refined = set_of(mirror, bases->names);
  return EG_OK;
}
}  // namespace

extern "C" int32_t eg_refine_validate(const eg_plan_set* base, const eg_refine_opts* o) {
  EG_TRY(eg_plans_validate(base));
  if (base->n_plans != 1) { set_error("eg_refine_validate: the base holds " + std::to_string(base->n_plans) + " plans (exactly 1)"); return EG_ERR_BAD_ARG; }
  return validate_opts("eg_refine_validate", false, base, o);
}

extern "C" int32_t eg_refine_plans_validate(const eg_plan_set* bases, const eg_refine_opts* o) {
  EG_TRY(validate_set("eg_refine_plans_validate", bases));
  return validate_opts("eg_refine_plans_validate", true, bases, o);
}

extern "C" int32_t eg_refine_plan(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* base, const eg_refine_opts* ro, uint64_t seed,
                                  uint64_t episode_index, eg_plan_set** refined, eg_refine_step* steps, int32_t* n_steps, int32_t* stop_reason,
                                  double* start_score, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !refined || !steps || !n_steps || !stop_reason) { set_error("eg_refine_plan: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_refine_plan", [&] { return eg_refine_validate(base, ro); }));
  return search(RefineRule{steps, nullptr, start_score}, "eg_refine_plan", false, c, s, o, base, ro, seed, episode_index, refined, n_steps, stop_reason, out);
}

extern "C" int32_t eg_refine_plans(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* bases, const eg_refine_opts* ro, uint64_t seed,
                                   uint64_t episode_index, eg_plan_set** refined, eg_refine_step* steps, int32_t* n_steps, int32_t* stop_reason,
                                   double* start_score, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !refined || !steps || !n_steps || !stop_reason) { set_error("eg_refine_plans: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_refine_plans", [&] { return eg_refine_plans_validate(bases, ro); }));
  return search(RefineRule{steps, nullptr, start_score}, "eg_refine_plans", true, c, s, o, bases, ro, seed, episode_index, refined, n_steps, stop_reason, out);
}

namespace {
// what eg_refine_plans_moves_validate asks, in `fn`'s name; null_moves: NULL move options mean "no moves" (eg_repair_plans) and are not refused
int32_t validate_moves(const char* fn, const eg_plan_set* bases, const eg_refine_opts* o, const eg_refine_move_opts* mo, bool null_moves) {
  EG_TRY(validate_set(fn, bases));
  if (!mo && !null_moves) { set_error(std::string(fn) + ": NULL move options"); return EG_ERR_BAD_ARG; }
  if (mo && (mo->max_shift < 0 || mo->max_shift > EG_YEARS - 1)) {
    set_error(std::string(fn) + ": max_shift = " + std::to_string(mo->max_shift) + " (0.." + std::to_string(EG_YEARS - 1) + " years; 0: no moves)");
    return EG_ERR_BAD_ARG;
  }
  return validate_opts(fn, true, bases, o, mo);
}
}  // namespace

extern "C" int32_t eg_refine_plans_moves_validate(const eg_plan_set* bases, const eg_refine_opts* o, const eg_refine_move_opts* mo) {
  return validate_moves("eg_refine_plans_moves_validate", bases, o, mo, false);
}

extern "C" int32_t eg_refine_plans_moves(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* bases, const eg_refine_opts* ro,
                                         const eg_refine_move_opts* mo, uint64_t seed, uint64_t episode_index, eg_plan_set** refined, eg_refine_move_step* steps,
                                         int32_t* n_steps, int32_t* stop_reason, double* start_score, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !refined || !steps || !n_steps || !stop_reason) { set_error("eg_refine_plans_moves: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_refine_plans_moves", [&] { return eg_refine_plans_moves_validate(bases, ro, mo); }));
  return search(RefineRule{nullptr, steps, start_score}, "eg_refine_plans_moves", true, c, s, o, bases, ro, seed, episode_index, refined, n_steps, stop_reason, out, mo);
}

extern "C" int32_t eg_repair_plans_validate(const eg_plan_set* bases, const eg_refine_opts* o, const eg_refine_move_opts* mo, const double* weights, int32_t k) {
  const char* fn = "eg_repair_plans_validate";
  EG_TRY(check_repair_weights([fn](const std::string& m) { set_error(std::string(fn) + ": " + m); return EG_ERR_BAD_ARG; }, weights, k));
  return validate_moves(fn, bases, o, mo, true);
}

extern "C" int32_t eg_repair_plans(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* bases, const eg_refine_opts* ro,
                                   const eg_refine_move_opts* mo, const double* weights, uint64_t seed, uint64_t episode_index, eg_plan_set** repaired,
                                   eg_repair_step* steps, int32_t* n_steps, int32_t* stop_reason, double* start_violation, double* final_violation,
                                   eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !repaired || !steps || !n_steps || !stop_reason) { set_error("eg_repair_plans: bad argument"); return EG_ERR_BAD_ARG; }
  const int32_t k = c->rows.n + c->builds.n;      // (rows first, then builds: the excess row's columns)
  EG_TRY(plan_entry(c, s, o, "eg_repair_plans", [&] {
    if (c->streams.n >= 2) {      // (the pick folds V from the excess rows, and those are the last pass's: stream 0's)
      set_error("eg_repair_plans: " + std::to_string(c->streams.n) + " plan streams are set (eg_plan_streams_set): a repair reads the excess rows, which are stream 0's (clear the streams first)");
      return EG_ERR_BAD_ARG;
    }
    EG_TRY(check_repair_weights([](const std::string& m) { set_error("eg_repair_plans: " + m); return EG_ERR_BAD_ARG; }, weights, k));
    return validate_moves("eg_repair_plans", bases, ro, mo, true);
  }));
  RepairRule rule{steps, start_violation, final_violation, weights ? std::vector<double>(weights, weights + k) : std::vector<double>(size_t(k), 1.0)};
  return search(rule, "eg_repair_plans", true, c, s, o, bases, ro, seed, episode_index, repaired, n_steps, stop_reason, out, mo);
}
