// eg_refine.cpp — eg_refine_plan (include/eirgrid_hip.h): the loop "score every one-entry edit of the plan, apply the best one" with the
// plan, its variants and the pick of the winner on the device.  The pieces are eg_plans.cpp's (stage_eval_snapshot, pack_plan_edits,
// launch_plans, write_lists) and k_plan_edits; what is new is k_refine_pick (eg_refine.h) behind each round's rollout grids and the
// host's mirror of the plan, from which the next round's edits are enumerated.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "eg_edit_order.h"
#include "eg_host.h"

using namespace eg;

namespace {
// the plan as the host follows it: the two lists, year by year
struct Mirror {
  std::vector<uint8_t> l[2][EG_YEARS];
  int64_t total(int w) const { int64_t n = 0; for (int y = 0; y < EG_YEARS; ++y) n += int64_t(l[w][y].size()); return n; }
};
// variants of a round over lists of these totals (include/eirgrid_hip.h: none, deletes, replaces, appends)
int64_t n_variants(int64_t len0, int64_t len1, const eg_refine_opts& o) {
  return 1 + len0 + len1 + int64_t(o.n_replace) * len0 + (len0 < int64_t(snap::kBestCap) ? int64_t(EG_YEARS) * o.n_append : 0);
}
void enumerate(const Mirror& m, const eg_refine_opts& o, std::vector<eg_plan_edit>& edits) {      // the round's edits, in the canonical order
  int32_t count[2][EG_YEARS];
  for (int w = 0; w < 2; ++w)
    for (int y = 0; y < EG_YEARS; ++y) count[w][y] = int32_t(m.l[w][y].size());
  enumerate_edits(count[0], count[1], o.replace_with, o.n_replace, o.append_with, o.n_append, m.total(0) < int64_t(snap::kBestCap), edits);
}
void apply(Mirror& m, const eg_plan_edit& e) {
  std::vector<uint8_t>& l = m.l[e.list][e.year];
  if (e.kind == EG_EDIT_DELETE) l.erase(l.begin() + e.pos);
  else if (e.kind == EG_EDIT_REPLACE) l[e.pos] = e.action;
  else if (e.kind == EG_EDIT_INSERT) l.insert(l.begin() + e.pos, e.action);
}
std::string too_many(int round, int64_t n) {
  return "round " + std::to_string(round) + " enumerates " + std::to_string(n) + " variants (at most " + std::to_string(EG_REFINE_MAX_VARIANTS) + ")";
}
}  // namespace

extern "C" int32_t eg_refine_validate(const eg_plan_set* base, const eg_refine_opts* o) {
  auto fail = [](const std::string& m) { set_error("eg_refine_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(base));
  if (base->n_plans != 1) return fail("the base holds " + std::to_string(base->n_plans) + " plans (exactly 1)");
  if (!o) return fail("NULL options");
  if (o->mode != 1 && o->mode != 2) return fail("mode " + std::to_string(o->mode) + " (1: optimization_mode None, 2: cost_only)");
  if (o->max_rounds < 1) return fail("max_rounds = " + std::to_string(o->max_rounds) + " (at least 1)");
  const char* name[2] = {"replace_with", "append_with"};
  const int32_t count[2] = {o->n_replace, o->n_append};
  const uint8_t* list[2] = {o->replace_with, o->append_with};
  for (int k = 0; k < 2; ++k) {
    const std::string n_name = k == 0 ? "n_replace" : "n_append";
    if (count[k] < 0) return fail(n_name + " = " + std::to_string(count[k]));
    if (count[k] > 0 && !list[k]) return fail(std::string("NULL ") + name[k] + " with " + n_name + " = " + std::to_string(count[k]));
    for (int32_t i = 0; i < count[k]; ++i)
      if (list[k][i] >= EG_N_ACTIONS) return fail(std::string(name[k]) + "[" + std::to_string(i) + "]: action " + std::to_string(int(list[k][i])) + " >= " + std::to_string(EG_N_ACTIONS));
  }
  const int64_t n = n_variants(base->best_actions_len, base->best_deficit_actions_len, *o);
  if (n > EG_REFINE_MAX_VARIANTS) return fail(too_many(0, n));
  return EG_OK;
}

extern "C" int32_t eg_refine_plan(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* base, const eg_refine_opts* ro, uint64_t seed,
                                  uint64_t episode_index, eg_plan_set** refined, eg_refine_step* steps, int32_t* n_steps, int32_t* stop_reason,
                                  double* start_score, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !refined || !steps || !n_steps || !stop_reason) { set_error("eg_refine_plan: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->group_member) { set_error("eg_refine_plan: the context is a rank of an eg_group (plan batches on a group are not supported)"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_refine_validate(base, ro));
  EG_TRY(check_policy(s, o, "eg_refine_plan"));
  EG_HIP(hipSetDevice(c->device));
  *refined = nullptr; *n_steps = 0;
  Mirror m;
  {
    const int32_t* count[2] = {base->best_count, base->best_deficit_count};
    const uint8_t* flat[2] = {base->best_actions, base->best_deficit_actions};
    for (int w = 0; w < 2; ++w) {
      int64_t at = 0;
      for (int y = 0; y < EG_YEARS; ++y) { m.l[w][y].assign(flat[w] + at, flat[w] + at + count[w][y]); at += count[w][y]; }
    }
  }
  // every buffer once, for the largest round max_rounds steps can lead to: best_actions grows by an entry a step at most, and only by
  // an append; a round beyond EG_REFINE_MAX_VARIANTS is refused when it is reached
  const int64_t len0 = m.total(0), len1 = m.total(1);
  const int64_t grown = ro->n_append > 0 ? std::min<int64_t>(len0 + ro->max_rounds, int64_t(snap::kBestCap)) : len0;
  const uint32_t n_cap = uint32_t(std::min<int64_t>(std::max(n_variants(len0, len1, *ro), 1 + grown + len1 + int64_t(ro->n_replace) * grown + int64_t(EG_YEARS) * ro->n_append),
                                                    EG_REFINE_MAX_VARIANTS));
  EG_TRY(ensure_outputs(c, n_cap));
  EG_HIP(c->d_plans.reserve(size_t(n_cap) * snap::kPlanStride));
  EG_HIP(c->d_plan_index.reserve(n_cap));
  EG_HIP(c->d_plan_edit_in.reserve(snap::kPlanStride + size_t(n_cap) * 8));
  EG_HIP(c->d_refine_log.reserve(size_t(kRefineLog) * kRefineEntryStride));
  {      // the base block goes up once; from then on k_refine_pick keeps it current
    std::vector<uint8_t> block(snap::kPlanStride, 0);
    write_lists(block.data(), base->best_count, base->best_actions, base->best_deficit_count, base->best_deficit_actions);
    EG_HIP(hipMemcpy(c->d_plan_edit_in, block.data(), block.size(), hipMemcpyHostToDevice));
  }
  DevSnapshot S{};
  EG_TRY(stage_eval_snapshot(c, s, o, &S));
  uint8_t* d_edits = c->d_plan_edit_in + snap::kPlanStride;
  std::vector<eg_plan_edit> edits;
  std::vector<uint32_t> packed, idx;
  int stop = EG_REFINE_MAX_ROUNDS;
  int32_t last = 0;      // the refined plan's record among the last round's
  if (start_score) *start_score = std::nan("");
  for (int round = 0;; ++round) {
    const int64_t want = n_variants(m.total(0), m.total(1), *ro);
    if (want > EG_REFINE_MAX_VARIANTS) { set_error("eg_refine_plan: " + too_many(round, want)); return EG_ERR_BAD_ARG; }
    enumerate(m, *ro, edits);
    const uint32_t n = uint32_t(edits.size());
    packed.resize(size_t(n) * 2); idx.resize(n);
    uint32_t n_short = 0;
    pack_plan_edits(edits.data(), n, m.total(0), packed.data(), idx.data(), &n_short);
    EG_HIP(hipMemcpy(d_edits, packed.data(), size_t(n) * 8, hipMemcpyHostToDevice));
    EG_HIP(hipMemcpy(c->d_plan_index, idx.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    EG_LAUNCH("k_plan_edits", launch_plan_edits(c->d_plan_edit_in, d_edits, n, c->d_plans, nullptr));
    c->n_plan_blocks = n;
    EG_TRY(launch_plans(c, S, seed, episode_index, n, n_short, true));
    uint8_t* d_entry = c->d_refine_log + size_t(round % kRefineLog) * kRefineEntryStride;
    EG_LAUNCH("k_refine_pick", launch_refine_pick(c->out, n, ro->mode, d_edits, c->d_plans, c->d_plan_edit_in, d_entry, nullptr));
    RefineEntry e{};
    EG_HIP(hipMemcpy(&e, d_entry, sizeof(e), hipMemcpyDeviceToHost));      // (waits for the round)
    if (round == 0 && start_score && e.base_ok) *start_score = e.base_score;
    if (!e.base_ok) { stop = EG_REFINE_BASE_FAILED; break; }
    if (e.n != int32_t(n) || e.winner < 0 || e.winner >= int32_t(n) || e.edit[0] != packed[2 * size_t(e.winner)] || e.edit[1] != packed[2 * size_t(e.winner) + 1]) {
      set_error("eg_refine_plan: round " + std::to_string(round) + ": the device's step entry does not name a variant of the round");
      return EG_ERR_INTERNAL;
    }
    last = e.winner;
    // the plan on the device against the mirror: the totals of the winner's block
    if (e.winner != 0) apply(m, edits[size_t(e.winner)]);
    if (e.off26 != int32_t(m.total(0)) || e.offd26 != int32_t(m.total(1))) {
      set_error("eg_refine_plan: round " + std::to_string(round) + ": the device's plan holds " + std::to_string(e.off26) + " + " + std::to_string(e.offd26) +
                " entries, the host's " + std::to_string(m.total(0)) + " + " + std::to_string(m.total(1)));
      return EG_ERR_INTERNAL;
    }
    if (e.winner == 0) { stop = EG_REFINE_LOCAL_OPTIMUM; break; }
    eg_refine_step& st = steps[*n_steps];
    st.edit = edits[size_t(e.winner)]; st.variant = e.winner; st.n_variants = int32_t(n); st.n_failed = e.n_failed; st.score = e.score;
    std::memcpy(st.metrics, e.metrics, sizeof(st.metrics));
    if (++*n_steps == ro->max_rounds) { stop = EG_REFINE_MAX_ROUNDS; break; }
  }
  *stop_reason = stop;
  if (out && stop != EG_REFINE_BASE_FAILED) {
    EG_TRY(fetch_records(c->out.base + size_t(last) * rec::stride, 1, out));
    if (out->status && out->status[0] == EG_EP_INTERNAL) { set_error("k_rollout: helper-wave protocol timed out in the refined plan's episode (EG_EP_INTERNAL)"); return EG_ERR_INTERNAL; }
  }
  {
    int32_t count[2][EG_YEARS];
    std::vector<uint8_t> flat[2];
    for (int w = 0; w < 2; ++w)
      for (int y = 0; y < EG_YEARS; ++y) { count[w][y] = int32_t(m.l[w][y].size()); flat[w].insert(flat[w].end(), m.l[w][y].begin(), m.l[w][y].end()); }
    flat[0].reserve(1); flat[1].reserve(1);
    *refined = make_plan_set(count[0], flat[0].data(), count[1], flat[1].data(), base->names && base->names[0] ? base->names[0] : "");
  }
  return EG_OK;
}
