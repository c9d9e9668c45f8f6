// eg_plans.cpp — a policy in snapshot layout (shared with eg_upload_snapshot) and plan batches: eg_evaluate_plans, eg_evaluate_plan_edits,
// eg_evaluate_plan_moves, eg_evaluate_plan_crosses, eg_evaluate_plan_rewrites over one tail (evaluate_batch), launch_plans, and plan sets to blocks and back (the
// searches are written from these and eg_plan_host.cpp's pieces).
#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "eg_host.h"
#define EG_RM static inline
#include "eg_reduced_math.h"

using namespace eg;

// What eg_upload_snapshot and eg_evaluate_plans refuse in a policy snapshot (the pointers are checked by the caller)
int eg::check_policy(const eg_policy_snapshot* s, const eg_opts* o, const char* who) {
  if (o && o->enable_construction_delays) { set_error("enable_construction_delays is not implemented on the device (SURVEY §8(f) N4)"); return EG_ERR_UNSUPPORTED; }
  // the device walks rely on strictly positive weights (the reference clamps every weight to [1e-4, 0.999])
  for (int i = 0; i < EG_YEARS * EG_N_ACTIONS; ++i) if (!(s->weights[i] > 0.0)) { set_error(std::string(who) + ": weights must be > 0"); return EG_ERR_BAD_ARG; }
  for (int i = 0; i < EG_YEARS * EG_N_DEFICIT; ++i) if (!(s->deficit_weights[i] > 0.0)) { set_error(std::string(who) + ": deficit weights must be > 0"); return EG_ERR_BAD_ARG; }
  return EG_OK;
}
// The list section of a snapshot at `dst` (snap::best_mask .. snap::state; a plan block has the same layout): per year the masks
// (bit a: a occurs in best(y) or best_deficit(y) / in best_deficit(y)), the prefix offsets and the two lists.  count == NULL: none.
// The lists' total lengths are the caller's to check (<= snap::kBestCap).
void eg::write_lists(uint8_t* dst, const int32_t* count, const uint8_t* act, const int32_t* dcount, const uint8_t* dact) {
  constexpr size_t b = snap::best_mask;
  int32_t off[28] = {0}, offd[28] = {0};
  unsigned long long mask[26] = {0}, dmask[26] = {0};
  if (count)
    for (int y = 0; y < EG_YEARS; ++y) {
      off[y + 1] = off[y] + count[y]; offd[y + 1] = offd[y] + dcount[y];
      for (int i = off[y]; i < off[y + 1]; ++i) if (act[i] < 64) mask[y] |= 1ull << act[i];
      for (int i = offd[y]; i < offd[y + 1]; ++i) if (dact[i] < 64) { mask[y] |= 1ull << dact[i]; dmask[y] |= 1ull << dact[i]; }
    }
  std::memcpy(dst + (snap::best_mask - b), mask, sizeof(mask)); std::memcpy(dst + (snap::bestd_mask - b), dmask, sizeof(dmask));
  std::memcpy(dst + (snap::best_off - b), off, sizeof(off)); std::memcpy(dst + (snap::bestd_off - b), offd, sizeof(offd));
  if (count) { std::memcpy(dst + (snap::best_actions - b), act, size_t(off[26])); std::memcpy(dst + (snap::bestd_actions - b), dact, size_t(offd[26])); }
}
// The policy `s` in snapshot layout into the staging buffer h (snap::upload_bytes): packed rows, list section, scalars
void eg::stage_policy(eg_ctx* c, const eg_policy_snapshot* s, bool have_lists, uint8_t* h) {
  {  // packed policy rows; sampling.rs:182, :352-355, :406: the sums the samplers start from, folded in table order
    double* pol = reinterpret_cast<double*>(h + snap::pol);
    std::memset(pol, 0, sizeof(double) * EG_YEARS * snap::kPolRow);
    for (int y = 0; y < EG_YEARS; ++y) {
      double* row = pol + y * snap::kPolRow;
      double a = 0.0, b = 0.0, c2 = 0.0;
      for (int i = 0; i < EG_N_ACTIONS; ++i) { row[i] = s->weights[y * EG_N_ACTIONS + i]; a += row[i]; }
      for (int i = 0; i < EG_N_DEFICIT; ++i) row[snap::kPolDw + i] = s->deficit_weights[y * EG_N_DEFICIT + i];
      for (int i = 0; i < 14; ++i) b += s->deficit_weights[y * EG_N_DEFICIT + i];
      if (s->count_weights) for (int i = 0; i < EG_N_COUNTS; ++i) { row[snap::kPolCw + i] = s->count_weights[y * EG_N_COUNTS + i]; c2 += row[snap::kPolCw + i]; }
      row[snap::kPolTotMain] = a; row[snap::kPolTotDeficit] = b; row[snap::kPolTotCount] = c2;
      const HostTables& H = c->tables.H;      // the year's world scalars ride along (eg_internal.h, snap::kPolYear)
      double* ys = row + snap::kPolYear;
      ys[0] = H.pre_co2[y]; ys[1] = H.pre_tg[y]; ys[2] = H.pre_ig[y]; ys[3] = H.pre_sg[y]; ys[4] = H.pre_optot[y];
      ys[5] = H.usage[y]; ys[6] = H.population[y]; ys[7] = H.inflation[y]; ys[8] = H.carbon_price[y]; ys[9] = double(H.pre_opcnt[y]);
    }
  }
  if (have_lists) write_lists(h + snap::best_mask, s->best_count, s->best_actions, s->best_deficit_count, s->best_deficit_actions);
  else write_lists(h + snap::best_mask, nullptr, nullptr, nullptr, nullptr);
  {  // the policy's scalars as the kernels read them (snap::state)
    DevState st{};
    st.learning_rate = s->learning_rate; st.exploration_rate = s->exploration_rate;
    for (int i = 0; i < 4; ++i) st.best_metrics[i] = s->has_best ? s->best_metrics[i] : 0.0;
    st.stall = s->iterations_without_improvement; st.iteration_count = c->push_iteration_count; st.failed_total = c->push_failed;
    st.has_best = s->has_best ? 1 : 0; st.has_cw = s->count_weights ? 1 : 0; st.has_lists = have_lists ? 1 : 0;
    rm::derive_state(st);
    std::memcpy(h + snap::state, &st, sizeof(st));
  }
}
// what the kernels get of a snapshot at d_base and the caller's options (none: the defaults)
DevSnapshot eg::snapshot_of(uint8_t* d_base, const eg_opts* o) {
  DevSnapshot S{};
  S.base = d_base;
  S.enable_energy_sales = o ? (o->enable_energy_sales ? 1 : 0) : 1;
  S.write_yearly = o ? (o->write_yearly ? 1 : 0) : 1;
  return S;
}

// A plan batch (eg_evaluate_plans) over the n episodes of c->out: c->d_plan_index lists the n_short short plans (<= kShortReplayMax
// actions), then the long ones.  The short-replay variant runs over exactly the short ones; the long ones go to k_replay_solo and the
// long-replay variant, in launches of at most as many episodes as the penalty-field pool has slots (a long replay claims one per
// launch epoch).  The hoist, the statistics epilogue and the best_result / top-K folds do not run.  With plan constraints set
// (eg_plan_constraints_set) k_plan_constraints runs behind the last grid, once, over the n records.
static int plans_pass(eg_ctx* c, const DevSnapshot& S, uint64_t seed, uint64_t first_index, uint32_t n, uint32_t n_short, bool same_index) {
  const uint32_t n_long = n - n_short;
  const bool helper = n <= c->helper_max_episodes;
  uint32_t done = 0;
  for (bool first = true; first || done < n_long; first = false) {
    uint32_t chunk = n_long - done;
    EG_TRY(prepare_heavy(c, chunk, chunk == 0));
    if (c->dev.heavy && chunk > c->dev.heavy_slots) chunk = c->dev.heavy_slots;
    RolloutPlan plan{};
    plan.plans = true; plan.helper_waves = helper; plan.same_index = same_index;
    plan.n_short = first ? n_short : 0u;
    plan.n_heavy = plan.n_short + chunk; plan.n_lean = 0; plan.mode = 1u;
    plan.d_index = c->d_plan_index; plan.d_index_long = c->d_plan_index + n_short + done;
    if (chunk > 0 && !helper) EG_TRY(arm_solo(c, plan, chunk));
    int slot = 0;
    EG_TRY(ring_take(c, plan, slot));
    EG_LAUNCH_AS("k_rollout launch (plan batch)", launch_rollout(c->dev, S, c->out, seed, first_index, n, nullptr, 1u, nullptr, plan));
    ring_commit(c, slot, 1);
    done += chunk;
  }
  c->last_n = n; c->last_first = first_index; c->feas_k = 0; c->ran = {};
  // the context's constraints over all n records, behind the grids on their stream: what the caller enqueues next reads the demoted statuses
  return c->rows.n + c->builds.n > 0 ? constrain_batch(c, n) : EG_OK;
}
// Every plan batch goes through here.  Without plan streams (eg_plan_streams_set) it is the one pass above.  With R >= 2 set it is R passes,
// pass r the batch as it runs without streams at first_index + r, from r = R - 1 down to 0 — so the records, the feasibility side buffers,
// last_n / last_first / feas_k are stream 0's when it returns — with k_ensemble_keep behind each (slab r of the context's store) and
// k_ensemble_commit behind the last: the committed metrics and status over the records', an eg_ensemble_row a variant (eg_streams.cpp).
// All on the null stream, behind the grids as the constraint kernel is: a pass's grids start behind the copy of the pass before.
int eg::launch_plans(eg_ctx* c, const DevSnapshot& S, uint64_t seed, uint64_t first_index, uint32_t n, uint32_t n_short, bool same_index) {
  const eg_ctx::Streams st = c->streams;
  if (st.n < 2) return plans_pass(c, S, seed, first_index, n, n_short, same_index);
  for (int r = st.n - 1; r >= 0; --r) {
    EG_TRY(plans_pass(c, S, seed, first_index + uint64_t(r), n, n_short, same_index));
    EG_TRY(ensemble_keep(c, n, r, st.n));
  }
  return ensemble_commit(c, n, st.n, st.tail, st.mode);
}
// The policy a plan batch is evaluated under into a device snapshot of its own (c->d_eval_snap) — has_best = 1 and lists present
// (empty: every episode reads its plan block instead) — with its stalled-sampler tables; *S: what the launches get, the plan pool set.
int eg::stage_eval_snapshot(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, DevSnapshot* S) {
  eg_policy_snapshot ps = *s;
  static const int32_t kNoCounts[EG_YEARS] = {};
  static const uint8_t kNoActions[1] = {0};
  ps.has_best = 1; ps.best_count = kNoCounts; ps.best_deficit_count = kNoCounts; ps.best_actions = kNoActions; ps.best_deficit_actions = kNoActions;
  EG_HIP(c->d_eval_snap.reserve(snap::upload_bytes));
  EG_HIP(hipStreamSynchronize(nullptr));   // the pinned staging buffer may still feed the previous copy
  stage_policy(c, &ps, true, c->h_snap);
  EG_HIP(hipMemcpyAsync(c->d_eval_snap, c->h_snap, snap::upload_bytes, hipMemcpyHostToDevice, nullptr));
  EG_LAUNCH("k_stalled_tables", launch_stalled_tables(c->d_eval_snap, nullptr));      // sampling.rs:190-220, as at upload
  *S = snapshot_of(c->d_eval_snap, o);
  S->plan_pool = c->d_plans;
  return EG_OK;
}
namespace {
// The rest of a plan batch of the n variants `idx` routes, the n_short short ones first.  `in` goes up: the plan blocks themselves into c->d_plans (Blocks::kHost), else into
// c->d_plan_edit_in the base block (a cross batch: the n_parents parent blocks; a rewrite batch: behind them the n_maps maps, kRewriteMapStride
// bytes each), then the packed edits, moves, crosses or rewrites, from which k_plan_edits / k_plan_moves / k_plan_crosses /
// k_plan_rewrites writes the blocks on the launches' stream.  Then the index, the policy into its device
// snapshot, the launches and the fetch.
// (The snapshot is staged last before the launches: a launch's start event takes the time the stream's previous command ended — with
//  the snapshot staged first, eg_timing_read counted the host building the plan blocks.)
enum class Blocks { kHost, kEdits, kMoves, kCrosses, kRewrites };      // who writes the plan blocks: the host has, k_plan_edits, k_plan_moves, k_plan_crosses, k_plan_rewrites
int evaluate_batch(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, Blocks blocks, const std::vector<uint8_t>& in, const std::vector<uint32_t>& idx,
                   uint32_t n_short, uint64_t seed, uint64_t first_index, bool same_index, eg_episode_out* out, uint32_t n_parents = 1u, uint32_t n_maps = 0u) {
  const uint32_t n = uint32_t(idx.size());
  EG_TRY(ensure_outputs(c, n));
  EG_HIP(c->d_plans.reserve(size_t(n) * snap::kPlanStride));
  EG_HIP(c->d_plan_index.reserve(n));
  if (blocks != Blocks::kHost) EG_HIP(c->d_plan_edit_in.reserve(in.size()));
  EG_HIP(hipMemcpy(blocks == Blocks::kHost ? c->d_plans.ptr : c->d_plan_edit_in.ptr, in.data(), in.size(), hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(c->d_plan_index, idx.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  DevSnapshot S{};
  EG_TRY(stage_eval_snapshot(c, s, o, &S));
  const uint8_t* d_in = c->d_plan_edit_in;
  if (blocks == Blocks::kEdits) EG_LAUNCH("k_plan_edits", launch_plan_edits(d_in, d_in + snap::kPlanStride, n, c->d_plans, nullptr));
  if (blocks == Blocks::kMoves) EG_LAUNCH("k_plan_moves", launch_plan_moves(d_in, 1u, nullptr, d_in + snap::kPlanStride, n, c->d_plans, nullptr));
  if (blocks == Blocks::kCrosses) EG_LAUNCH("k_plan_crosses", launch_plan_crosses(d_in, n_parents, d_in + size_t(n_parents) * snap::kPlanStride, n, c->d_plans, nullptr));
  if (blocks == Blocks::kRewrites) {
    const uint8_t* d_maps = d_in + size_t(n_parents) * snap::kPlanStride;
    EG_LAUNCH("k_plan_rewrites", launch_plan_rewrites(d_in, n_parents, d_maps, n_maps, d_maps + size_t(n_maps) * kRewriteMapStride, n, c->d_plans, nullptr));
  }
  c->n_plan_blocks = n;
  EG_TRY(launch_plans(c, S, seed, first_index, n, n_short, same_index));
  return out ? eg_fetch(c, out) : EG_OK;
}
// what goes up for an edit or move batch of n variants: the base plan's block, then room for 8 bytes a variant; *base_len: of its best_actions
std::vector<uint8_t> base_and_room(const eg_plan_set* base, uint32_t n, int64_t* base_len) {
  std::vector<uint8_t> in(snap::kPlanStride + size_t(n) * 8, 0);
  write_plan_blocks(base, in.data());
  *base_len = 0;
  for (int y = 0; y < EG_YEARS; ++y) *base_len += base->best_count[y];
  return in;
}
}  // namespace

extern "C" int32_t eg_evaluate_plans(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* p, uint64_t seed, uint64_t first_index,
                          eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights) { set_error("eg_evaluate_plans: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_evaluate_plans", [&] { return eg_plans_validate(p); }));
  const uint32_t n = uint32_t(p->n_plans);
  // the plan blocks (the list section's layout, one per plan) and the routing, from the plans' best_actions totals
  std::vector<uint8_t> blocks(size_t(n) * snap::kPlanStride, 0);
  write_plan_blocks(p, blocks.data());
  std::vector<int32_t> off[2];
  parent_offsets(p, off);
  Routing R;
  for (uint32_t j = 0; j < n; ++j) R.add(j, off[0][size_t(j) * 27 + EG_YEARS]);
  const uint32_t n_short = R.finish();
  return evaluate_batch(c, s, o, Blocks::kHost, blocks, R.idx, n_short, seed, first_index, false, out);
}

// ---------------------------------------------------------------- plan edits (include/eirgrid_hip.h eg_evaluate_plan_edits)
extern "C" int32_t eg_plan_edits_validate(const eg_plan_set* base, const eg_plan_edit* edits, int32_t n_edits) {
  auto fail = [](const std::string& m) { set_error("eg_plan_edits_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(base));
  if (base->n_plans != 1) return fail("the base holds " + std::to_string(base->n_plans) + " plans (exactly 1)");
  if (n_edits < 1) return fail("n_edits = " + std::to_string(n_edits) + " (at least 1)");
  if (!edits) return fail("NULL edits");
  const char* field[2] = {"best_actions", "best_deficit_actions"};
  const int32_t* count[2] = {base->best_count, base->best_deficit_count};
  int64_t total[2] = {0, 0};
  for (int w = 0; w < 2; ++w) for (int y = 0; y < EG_YEARS; ++y) total[w] += count[w][y];
  for (int32_t j = 0; j < n_edits; ++j) {
    const eg_plan_edit& e = edits[j];
    const std::string who = "edit " + std::to_string(j) + ": ";
    if (e.kind > EG_EDIT_INSERT) return fail(who + "kind " + std::to_string(int(e.kind)) + " (0 none, 1 delete, 2 replace, 3 insert)");
    if (e.kind == EG_EDIT_NONE) continue;      // (the base plan itself: the other fields are not read)
    if (e.list > 1) return fail(who + "list " + std::to_string(int(e.list)) + " (0 best_actions, 1 best_deficit_actions)");
    if (e.year >= EG_YEARS) return fail(who + "year " + std::to_string(int(e.year)) + " (a year index 0.." + std::to_string(EG_YEARS - 1) + ")");
    const int64_t len = count[e.list][e.year];
    const std::string where = std::string(field[e.list]) + " year " + std::to_string(2025 + int(e.year)) + " (" + std::to_string(len) + " entries)";
    if (e.kind == EG_EDIT_INSERT ? int64_t(e.pos) > len : int64_t(e.pos) >= len)
      return fail(who + "pos " + std::to_string(e.pos) + " outside " + where + (e.kind == EG_EDIT_INSERT ? ": an insert takes 0..len" : ": 0..len-1"));
    if (e.kind == EG_EDIT_INSERT && total[e.list] + 1 > int64_t(snap::kBestCap))
      return fail(who + "the insert makes " + field[e.list] + " " + std::to_string(total[e.list] + 1) + " entries (at most " + std::to_string(snap::kBestCap) + ")");
    if (e.kind != EG_EDIT_DELETE && e.action >= EG_N_ACTIONS)
      return fail(who + "action " + std::to_string(int(e.action)) + " >= " + std::to_string(EG_N_ACTIONS));
  }
  return EG_OK;
}

extern "C" int32_t eg_evaluate_plan_edits(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* base, const eg_plan_edit* edits,
                                          int32_t n_edits, uint64_t seed, uint64_t first_index, int32_t same_index, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights) { set_error("eg_evaluate_plan_edits: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_evaluate_plan_edits", [&] { return eg_plan_edits_validate(base, edits, n_edits); }));
  const uint32_t n = uint32_t(n_edits);
  int64_t base_len = 0;
  std::vector<uint8_t> in = base_and_room(base, n, &base_len);
  std::vector<uint32_t> idx(n);
  uint32_t n_short = 0;
  pack_plan_edits(edits, n, base_len, reinterpret_cast<uint32_t*>(in.data() + snap::kPlanStride), idx.data(), &n_short);
  return evaluate_batch(c, s, o, Blocks::kEdits, in, idx, n_short, seed, first_index, same_index != 0, out);
}

// ---------------------------------------------------------------- plan moves (include/eirgrid_hip.h eg_evaluate_plan_moves)
// what goes up per move, 8 bytes (eg_plan_moves.h unpack_move); the first byte is no edit kind
static_assert(sizeof(eg_plan_move) == 12 && sizeof(eg_refine_move_step) == 80, "the move structs are part of the C ABI");
void eg::pack_plan_move(const eg_plan_move& m, uint32_t* packed) {
  packed[0] = kPlanMoveTag | uint32_t(m.list) << 8 | uint32_t(m.year) << 16 | uint32_t(m.to_year) << 24;
  packed[1] = m.pos | m.to_pos << 16;
}

extern "C" int32_t eg_plan_moves_validate(const eg_plan_set* base, const eg_plan_move* moves, int32_t n_moves) {
  auto fail = [](const std::string& m) { set_error("eg_plan_moves_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(base));
  if (base->n_plans != 1) return fail("the base holds " + std::to_string(base->n_plans) + " plans (exactly 1)");
  if (n_moves < 1) return fail("n_moves = " + std::to_string(n_moves) + " (at least 1)");
  if (!moves) return fail("NULL moves");
  const char* field[2] = {"best_actions", "best_deficit_actions"};
  const int32_t* count[2] = {base->best_count, base->best_deficit_count};
  for (int32_t j = 0; j < n_moves; ++j) {
    const eg_plan_move& m = moves[j];
    const std::string who = "move " + std::to_string(j) + ": ";
    if (m.list > 1) return fail(who + "list " + std::to_string(int(m.list)) + " (0 best_actions, 1 best_deficit_actions)");
    if (m.year >= EG_YEARS) return fail(who + "year " + std::to_string(int(m.year)) + " (a year index 0.." + std::to_string(EG_YEARS - 1) + ")");
    if (m.to_year >= EG_YEARS) return fail(who + "to_year " + std::to_string(int(m.to_year)) + " (a year index 0.." + std::to_string(EG_YEARS - 1) + ")");
    const int64_t len = count[m.list][m.year];
    if (int64_t(m.pos) >= len)
      return fail(who + "pos " + std::to_string(m.pos) + " outside " + field[m.list] + " year " + std::to_string(2025 + int(m.year)) + " (" + std::to_string(len) + " entries): 0..len-1");
    const int64_t to_len = count[m.list][m.to_year] - (m.to_year == m.year ? 1 : 0);
    if (int64_t(m.to_pos) > to_len)
      return fail(who + "to_pos " + std::to_string(m.to_pos) + " outside " + field[m.list] + " year " + std::to_string(2025 + int(m.to_year)) + " (" + std::to_string(to_len) +
                  " entries after the removal)");
  }
  return EG_OK;
}

extern "C" int32_t eg_evaluate_plan_moves(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* base, const eg_plan_move* moves,
                                          int32_t n_moves, uint64_t seed, uint64_t first_index, int32_t same_index, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights) { set_error("eg_evaluate_plan_moves: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_evaluate_plan_moves", [&] { return eg_plan_moves_validate(base, moves, n_moves); }));
  const uint32_t n = uint32_t(n_moves);
  int64_t base_len = 0;
  std::vector<uint8_t> in = base_and_room(base, n, &base_len);
  uint32_t* packed = reinterpret_cast<uint32_t*>(in.data() + snap::kPlanStride);
  Routing R;      // (a move keeps the lists' lengths, so every variant takes the base's route)
  for (uint32_t j = 0; j < n; ++j) { pack_plan_move(moves[j], packed + 2 * size_t(j)); R.add(j, base_len); }
  const uint32_t n_short = R.finish();
  return evaluate_batch(c, s, o, Blocks::kMoves, in, R.idx, n_short, seed, first_index, same_index != 0, out);
}

// ---------------------------------------------------------------- plan crosses (include/eirgrid_hip.h eg_evaluate_plan_crosses)
static_assert(sizeof(eg_plan_cross) == 6, "eg_plan_cross is part of the C ABI");
static_assert(EG_CROSS_MAX_PARENTS <= 256, "a parent index is packed into one byte (eg_plan_crosses.h unpack_cross)");
// the two lists' prefix offsets of every plan of a valid set: off[w][p * 27 + y], w = 0 best_actions, 1 best_deficit_actions
void eg::parent_offsets(const eg_plan_set* p, std::vector<int32_t> off[2]) {
  const int32_t* count[2] = {p->best_count, p->best_deficit_count};
  for (int w = 0; w < 2; ++w) {
    off[w].assign(size_t(p->n_plans) * 27, 0);
    for (int32_t j = 0; j < p->n_plans; ++j)
      for (int y = 0; y < EG_YEARS; ++y) off[w][size_t(j) * 27 + y + 1] = off[w][size_t(j) * 27 + y] + count[w][size_t(j) * EG_YEARS + y];
  }
}
// the length of list w of the child of cross x: a's, with a's window taken out and b's put in
int64_t eg::child_len(const std::vector<int32_t>& off, const eg_plan_cross& x) {
  const int32_t* oa = off.data() + size_t(x.a) * 27;
  const int32_t* ob = off.data() + size_t(x.b) * 27;
  return int64_t(oa[EG_YEARS]) - (oa[x.to_year] - oa[x.from_year]) + (ob[x.to_year] - ob[x.from_year]);
}
// what goes up per cross, 8 bytes (eg_plan_crosses.h unpack_cross)
void eg::pack_plan_cross(const eg_plan_cross& x, uint32_t* packed) {
  packed[0] = uint32_t(x.a) | uint32_t(x.b) << 8 | uint32_t(x.from_year) << 16 | uint32_t(x.to_year) << 24;
  packed[1] = 0u;
}
// every plan of a valid set as a plan block at dst (zeroed by the caller), snap::kPlanStride bytes apart
void eg::write_plan_blocks(const eg_plan_set* p, uint8_t* dst) {
  int64_t pos = 0, dpos = 0;
  for (int32_t j = 0; j < p->n_plans; ++j) {
    const int32_t* cnt = p->best_count + size_t(j) * EG_YEARS;
    const int32_t* dcnt = p->best_deficit_count + size_t(j) * EG_YEARS;
    write_lists(dst + size_t(j) * snap::kPlanStride, cnt, p->best_actions + pos, dcnt, p->best_deficit_actions + dpos);
    for (int y = 0; y < EG_YEARS; ++y) { pos += cnt[y]; dpos += dcnt[y]; }
  }
}

// the blocks of n plans as they stood on the device, decoded into a plan set (the reverse of write_lists)
int eg::decode_plan_blocks(const uint8_t* blocks, int32_t n, const char* who, eg_plan_set** set) {
  std::vector<int32_t> count[2];
  std::vector<uint8_t> flat[2];
  const size_t at_off[2] = {snap::best_off - snap::best_mask, snap::bestd_off - snap::best_mask};
  const size_t at_act[2] = {snap::best_actions - snap::best_mask, snap::bestd_actions - snap::best_mask};
  for (int w = 0; w < 2; ++w)
    for (int32_t p = 0; p < n; ++p) {
      const uint8_t* b = blocks + size_t(p) * snap::kPlanStride;
      int32_t off[28];
      std::memcpy(off, b + at_off[w], sizeof(off));
      for (int y = 0; y < EG_YEARS; ++y) {
        if (off[0] != 0 || off[y + 1] < off[y] || off[y + 1] > int32_t(snap::kBestCap)) {
          set_error(std::string(who) + ": plan " + std::to_string(p) + " of the population has corrupt offsets on the device");
          return EG_ERR_INTERNAL;
        }
        count[w].push_back(off[y + 1] - off[y]);
      }
      flat[w].insert(flat[w].end(), b + at_act[w], b + at_act[w] + off[EG_YEARS]);
    }
  flat[0].reserve(1); flat[1].reserve(1);
  *set = make_plan_set_n(n, count[0].data(), flat[0].data(), count[1].data(), flat[1].data(), nullptr);
  return EG_OK;
}

extern "C" int32_t eg_plan_crosses_validate(const eg_plan_set* parents, const eg_plan_cross* crosses, int32_t n_crosses) {
  auto fail = [](const std::string& m) { set_error("eg_plan_crosses_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(parents));
  if (parents->n_plans > EG_CROSS_MAX_PARENTS)
    return fail("the set holds " + std::to_string(parents->n_plans) + " plans (at most " + std::to_string(EG_CROSS_MAX_PARENTS) + ")");
  if (n_crosses < 1 || n_crosses > EG_CROSS_MAX_VARIANTS) return fail("n_crosses = " + std::to_string(n_crosses) + " (1.." + std::to_string(EG_CROSS_MAX_VARIANTS) + ")");
  if (!crosses) return fail("NULL crosses");
  const char* field[2] = {"best_actions", "best_deficit_actions"};
  std::vector<int32_t> off[2];
  parent_offsets(parents, off);
  for (int32_t j = 0; j < n_crosses; ++j) {
    const eg_plan_cross& x = crosses[j];
    const std::string who = "cross " + std::to_string(j) + ": ";
    if (int32_t(x.a) >= parents->n_plans) return fail(who + "a " + std::to_string(int(x.a)) + " >= n_plans " + std::to_string(parents->n_plans));
    if (int32_t(x.b) >= parents->n_plans) return fail(who + "b " + std::to_string(int(x.b)) + " >= n_plans " + std::to_string(parents->n_plans));
    if (x.to_year > EG_YEARS) return fail(who + "to_year " + std::to_string(int(x.to_year)) + " (at most " + std::to_string(EG_YEARS) + ")");
    if (x.from_year > x.to_year) return fail(who + "from_year " + std::to_string(int(x.from_year)) + " > to_year " + std::to_string(int(x.to_year)));
    for (int w = 0; w < 2; ++w) {
      const int64_t len = child_len(off[w], x);
      if (len > int64_t(snap::kBestCap))
        return fail(who + field[w] + " would hold " + std::to_string(len) + " entries (at most " + std::to_string(snap::kBestCap) + ")");
    }
  }
  return EG_OK;
}

extern "C" int32_t eg_evaluate_plan_crosses(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* parents, const eg_plan_cross* crosses,
                                            int32_t n_crosses, uint64_t seed, uint64_t first_index, int32_t same_index, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights) { set_error("eg_evaluate_plan_crosses: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_evaluate_plan_crosses", [&] { return eg_plan_crosses_validate(parents, crosses, n_crosses); }));
  const uint32_t n = uint32_t(n_crosses), P = uint32_t(parents->n_plans);
  // what goes up: every parent's block, once, and the packed crosses (eg_plan_crosses.h unpack_cross); the routing from the counts — two
  // short parents can make a long child and the reverse
  std::vector<uint8_t> in(size_t(P) * snap::kPlanStride + size_t(n) * 8, 0);
  write_plan_blocks(parents, in.data());
  std::vector<int32_t> off[2];
  parent_offsets(parents, off);
  uint32_t* packed = reinterpret_cast<uint32_t*>(in.data() + size_t(P) * snap::kPlanStride);
  Routing R;
  for (uint32_t j = 0; j < n; ++j) { pack_plan_cross(crosses[j], packed + 2 * size_t(j)); R.add(j, child_len(off[0], crosses[j])); }
  const uint32_t n_short = R.finish();
  return evaluate_batch(c, s, o, Blocks::kCrosses, in, R.idx, n_short, seed, first_index, same_index != 0, out, P);
}

// ---------------------------------------------------------------- plan rewrites (include/eirgrid_hip.h eg_evaluate_plan_rewrites)
static_assert(sizeof(eg_action_map) == 61 && sizeof(eg_plan_rewrite) == 8, "the rewrite structs are part of the C ABI");
static_assert(sizeof(eg_action_map) <= kRewriteMapStride && EG_REWRITE_MAX_MAPS <= 65536 && EG_CROSS_MAX_PARENTS <= 65536, "a plan and a map index are packed into 16 bits each");
// what goes up per rewrite, 8 bytes (eg_plan_rewrites.h unpack_rewrite)
void eg::pack_plan_rewrite(const eg_plan_rewrite& r, uint32_t* packed) {
  packed[0] = uint32_t(r.plan) | uint32_t(r.map) << 16;
  packed[1] = uint32_t(r.from_year) | uint32_t(r.to_year) << 8 | uint32_t(r.lists) << 16;
}

extern "C" int32_t eg_plan_rewrites_validate(const eg_plan_set* plans, const eg_action_map* maps, int32_t n_maps, const eg_plan_rewrite* rewrites, int32_t n_rewrites) {
  auto fail = [](const std::string& m) { set_error("eg_plan_rewrites_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(plans));
  if (plans->n_plans > EG_CROSS_MAX_PARENTS)
    return fail("the set holds " + std::to_string(plans->n_plans) + " plans (at most " + std::to_string(EG_CROSS_MAX_PARENTS) + ")");
  if (n_maps < 1 || n_maps > EG_REWRITE_MAX_MAPS) return fail("n_maps = " + std::to_string(n_maps) + " (1.." + std::to_string(EG_REWRITE_MAX_MAPS) + ")");
  if (!maps) return fail("NULL maps");
  for (int32_t m = 0; m < n_maps; ++m)
    for (int e = 0; e < EG_N_ACTIONS; ++e)
      if (maps[m].to[e] >= EG_N_ACTIONS && maps[m].to[e] != EG_REWRITE_DROP)
        return fail("map " + std::to_string(m) + ": to[" + std::to_string(e) + "] = " + std::to_string(int(maps[m].to[e])) + " (0.." + std::to_string(EG_N_ACTIONS - 1) + " or 0xFF drop)");
  if (n_rewrites < 1 || n_rewrites > EG_REWRITE_MAX_VARIANTS)
    return fail("n_rewrites = " + std::to_string(n_rewrites) + " (1.." + std::to_string(EG_REWRITE_MAX_VARIANTS) + ")");
  if (!rewrites) return fail("NULL rewrites");
  for (int32_t j = 0; j < n_rewrites; ++j) {
    const eg_plan_rewrite& r = rewrites[j];
    const std::string who = "rewrite " + std::to_string(j) + ": ";
    if (int32_t(r.plan) >= plans->n_plans) return fail(who + "plan " + std::to_string(int(r.plan)) + " >= n_plans " + std::to_string(plans->n_plans));
    if (int32_t(r.map) >= n_maps) return fail(who + "map " + std::to_string(int(r.map)) + " >= n_maps " + std::to_string(n_maps));
    if (r.to_year > EG_YEARS) return fail(who + "to_year " + std::to_string(int(r.to_year)) + " (at most " + std::to_string(EG_YEARS) + ")");
    if (r.from_year > r.to_year) return fail(who + "from_year " + std::to_string(int(r.from_year)) + " > to_year " + std::to_string(int(r.to_year)));
    if (r.lists > 3) return fail(who + "lists " + std::to_string(int(r.lists)) + " (bit 0 best_actions, bit 1 best_deficit_actions)");
    if (r.pad != 0) return fail(who + "pad " + std::to_string(int(r.pad)) + " (must be 0)");
  }
  return EG_OK;
}

extern "C" int32_t eg_evaluate_plan_rewrites(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* plans, const eg_action_map* maps, int32_t n_maps,
                                             const eg_plan_rewrite* rewrites, int32_t n_rewrites, uint64_t seed, uint64_t first_index, int32_t same_index,
                                             eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights) { set_error("eg_evaluate_plan_rewrites: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(plan_entry(c, s, o, "eg_evaluate_plan_rewrites", [&] { return eg_plan_rewrites_validate(plans, maps, n_maps, rewrites, n_rewrites); }));
  const uint32_t n = uint32_t(n_rewrites), P = uint32_t(plans->n_plans), M = uint32_t(n_maps);
  // what goes up: every plan's block, once, the maps padded with drop bytes to kRewriteMapStride, and the packed rewrites
  const size_t at_maps = size_t(P) * snap::kPlanStride, at_packed = at_maps + size_t(M) * kRewriteMapStride;
  std::vector<uint8_t> in(at_packed + size_t(n) * 8, 0);
  write_plan_blocks(plans, in.data());
  for (uint32_t m = 0; m < M; ++m) {
    std::memset(in.data() + at_maps + size_t(m) * kRewriteMapStride, EG_REWRITE_DROP, kRewriteMapStride);
    std::memcpy(in.data() + at_maps + size_t(m) * kRewriteMapStride, maps[m].to, sizeof(maps[m].to));
  }
  // the routing, from the child's best_actions length: the plan's, less the entries of the window the map drops.  A histogram of every
  // plan's best_actions by year and action, built once; per (plan, map) pair the call meets, the dropped entries in front of every year
  std::vector<int32_t> off[2];
  parent_offsets(plans, off);
  std::vector<int32_t> hist(size_t(P) * EG_YEARS * EG_N_ACTIONS, 0);
  {
    size_t pos = 0;
    for (uint32_t p = 0; p < P; ++p)
      for (int y = 0; y < EG_YEARS; ++y)
        for (int32_t i = 0; i < plans->best_count[size_t(p) * EG_YEARS + y]; ++i) ++hist[(size_t(p) * EG_YEARS + y) * EG_N_ACTIONS + plans->best_actions[pos++]];
  }
  std::unordered_map<uint32_t, std::vector<int32_t>> dropped;      // plan | map << 16 -> [27] prefix sums over the years
  auto dropped_before = [&](uint32_t p, uint32_t m) -> const std::vector<int32_t>& {
    auto it = dropped.find(p | m << 16);
    if (it != dropped.end()) return it->second;
    std::vector<int32_t> d(EG_YEARS + 1, 0);
    for (int y = 0; y < EG_YEARS; ++y) {
      d[y + 1] = d[y];
      for (int e = 0; e < EG_N_ACTIONS; ++e) if (maps[m].to[e] == EG_REWRITE_DROP) d[y + 1] += hist[(size_t(p) * EG_YEARS + y) * EG_N_ACTIONS + e];
    }
    return dropped.emplace(p | m << 16, std::move(d)).first->second;
  };
  uint32_t* packed = reinterpret_cast<uint32_t*>(in.data() + at_packed);
  Routing R;
  for (uint32_t j = 0; j < n; ++j) {
    const eg_plan_rewrite& r = rewrites[j];
    pack_plan_rewrite(r, packed + 2 * size_t(j));
    int64_t len = off[0][size_t(r.plan) * 27 + EG_YEARS];
    if ((r.lists & 1) && r.to_year > r.from_year) { const std::vector<int32_t>& d = dropped_before(r.plan, r.map); len -= d[r.to_year] - d[r.from_year]; }
    R.add(j, len);
  }
  const uint32_t n_short = R.finish();
  return evaluate_batch(c, s, o, Blocks::kRewrites, in, R.idx, n_short, seed, first_index, same_index != 0, out, P, M);
}

extern "C" int32_t eg_debug_fetch_plan_block(eg_ctx* c, uint32_t plan, uint8_t* out) {
  static_assert(EG_PLAN_BLOCK_BYTES == snap::kPlanStride, "plan block size is part of the C ABI");
  if (!c || !out) { set_error("eg_debug_fetch_plan_block: bad argument"); return EG_ERR_BAD_ARG; }
  if (!c->d_plans.ptr || size_t(plan) >= c->n_plan_blocks) { set_error("eg_debug_fetch_plan_block: plan " + std::to_string(plan) + " is not in the last plan batch (" + std::to_string(c->n_plan_blocks) + " plans)"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipDeviceSynchronize());
  EG_HIP(hipMemcpy(out, c->d_plans + size_t(plan) * snap::kPlanStride, snap::kPlanStride, hipMemcpyDeviceToHost));
  return EG_OK;
}
