// eg_plan_host.cpp — the pieces a plan search is written from (eg_host.h lists them): the entry preamble, a launch's
// packing and routing, the launch of a chunk of variants, the private archive of eg_breed_plans / eg_explore_plans and the option checks
// the validators share.  Each exists once: eg_plans / eg_refine / eg_breed / eg_explore / eg_debug .cpp call them.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "eg_host.h"

using namespace eg;

int eg::plan_entry(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const char* fn, const std::function<int32_t()>& validate) {
  if (c->group_member) { set_error(std::string(fn) + ": the context is a rank of an eg_group (plan batches on a group are not supported)"); return EG_ERR_BAD_ARG; }
  EG_TRY(validate());
  EG_TRY(check_policy(s, o, fn));
  if (c->rows.n > 0 && o && !o->write_yearly) {
    set_error(std::string(fn) + ": write_yearly = 0 while " + std::to_string(c->rows.n) + " plan constraints are set (the yearly rows are what they judge)");
    return EG_ERR_BAD_ARG;
  }
  EG_HIP(hipSetDevice(c->device));
  return EG_OK;
}

// ---------------------------------------------------------------- packing and routing
namespace {
// an edit's 8 bytes (eg_plan_edits.h unpack); returns the length of the variant's best_actions list: the base's, one entry longer or shorter
int64_t pack_edit(const eg_plan_edit& e, int64_t base_len, uint32_t* packed) {
  const bool none = e.kind == EG_EDIT_NONE;
  packed[0] = none ? 0u : uint32_t(e.kind) | uint32_t(e.list) << 8 | uint32_t(e.year) << 16 | uint32_t(e.kind == EG_EDIT_DELETE ? 0 : e.action) << 24;
  packed[1] = none ? 0u : e.pos;
  return base_len + (!none && e.list == 0 ? (e.kind == EG_EDIT_INSERT ? 1 : e.kind == EG_EDIT_DELETE ? -1 : 0) : 0);
}
}  // namespace
// What a plan-edit batch uploads behind the base block, 8 bytes per variant, and its routing
void eg::pack_plan_edits(const eg_plan_edit* edits, uint32_t n, int64_t base_len, uint32_t* packed, uint32_t* idx, uint32_t* n_short) {
  Routing R;
  for (uint32_t j = 0; j < n; ++j) R.add(j, pack_edit(edits[j], base_len, packed + 2 * size_t(j)));
  *n_short = R.finish();
  std::copy(R.idx.begin(), R.idx.end(), idx);
}
bool eg::pack_neighbourhood(uint32_t base_slot, int64_t len0, const eg_plan_edit* edits, uint32_t n_edits, const eg_plan_move* moves, uint32_t n_moves, uint32_t first,
                            uint32_t* packed, uint32_t* slot, Routing& R) {
  for (uint32_t j = 0; j < n_edits; ++j) R.add(first + j, pack_edit(edits[j], len0, packed + 2 * (size_t(first) + j)));
  for (uint32_t j = n_edits; j < n_edits + n_moves; ++j) {      // a move keeps the lengths: the base's route
    pack_plan_move(moves[j - n_edits], packed + 2 * (size_t(first) + j));
    R.add(first + j, len0);
  }
  std::fill(slot + first, slot + first + n_edits + n_moves, base_slot);
  return n_moves > 0;
}
int eg::launch_variants(eg_ctx* c, const DevSnapshot& S, const uint8_t* d_bases, uint32_t n_bases, const std::vector<uint8_t>& in, size_t at_slot, uint32_t n,
                        Routing& R, bool any_moves, uint64_t seed, uint64_t index) {
  const uint32_t n_short = R.finish();
  // (synchronous copies on the null stream: they wait for the previous launch, whose kernels read what they overwrite)
  EG_HIP(hipMemcpy(c->d_refine_in, in.data(), in.size(), hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(c->d_plan_index, R.idx.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
  const uint32_t* d_slot = reinterpret_cast<const uint32_t*>(c->d_refine_in + at_slot);
  EG_LAUNCH("k_plan_edits_many", launch_plan_edits_many(d_bases, n_bases, d_slot, c->d_refine_in, n, c->d_plans, nullptr));
  // (the move variants' blocks: over the base copies k_plan_edits_many has just written for them, on the same stream)
  if (any_moves) EG_LAUNCH("k_plan_moves", launch_plan_moves(d_bases, n_bases, d_slot, c->d_refine_in, n, c->d_plans, nullptr));
  c->n_plan_blocks = n;
  return launch_plans(c, S, seed, index, n, n_short, true);
}

// ---------------------------------------------------------------- the private archive
int eg::archive_begin(eg_ctx* c, int32_t cap, int32_t objectives, int32_t mode, const std::function<int()>& between) {
  EG_HIP(c->d_breed.reserve(breed_at::total));
  EG_HIP(c->d_breed_work.reserve(pareto_work_bytes(EG_CROSS_MAX_VARIANTS)));
  ParetoState st{};
  st.cap = cap; st.objectives = objectives; st.mode = pareto_rank_mode(mode); st.pad = pareto_keep_spread(mode) ? kParetoKeepSpread : 0;
  EG_HIP(hipMemcpy(c->d_breed, &st, sizeof(st), hipMemcpyHostToDevice));
  c->breed_spread = pareto_keep_spread(mode);
  if (between) EG_TRY(between());
  const BreedCounters zero{};
  EG_HIP(hipMemcpy(c->d_breed + breed_at::counters, &zero, sizeof(zero), hipMemcpyHostToDevice));
  return EG_OK;
}
int eg::archive_upload(eg_ctx* c, const eg_plan_set* set, int array) {
  std::vector<uint8_t> blocks(size_t(set->n_plans) * snap::kPlanStride, 0);
  write_plan_blocks(set, blocks.data());
  EG_HIP(hipMemcpy(archive_array(c, array), blocks.data(), blocks.size(), hipMemcpyHostToDevice));
  return EG_OK;
}
int eg::archive_fold(eg_ctx* c, uint32_t n, uint64_t first_index) {
  const ParetoWork work = pareto_work(c->d_breed_work, EG_CROSS_MAX_VARIANTS);
  EG_LAUNCH("k_pareto_filter .. k_pareto_finalize", launch_pareto_fold(c->d_breed, work, c->out, n, first_index, c->breed_spread, nullptr));
  EG_LAUNCH("k_breed_gather", launch_breed_gather(c->d_breed, c->out, n, first_index, c->d_plans, nullptr));
  return EG_OK;
}
int eg::archive_read_generation(eg_ctx* c, std::vector<uint8_t>& rb) {
  rb.resize(breed_at::kReadbackBytes);
  EG_HIP(hipMemcpy(rb.data(), c->d_breed + breed_at::readback, rb.size(), hipMemcpyDeviceToHost));
  return EG_OK;
}
bool eg::archive_row(const std::vector<uint8_t>& rb, int32_t r, int32_t cap, ParetoEntry* entry, int32_t (&tab)[2][28]) {
  if (r < 0 || r >= EG_PARETO_MAX) return false;
  const uint8_t* row = rb.data() + kBreedHeaderBytes + size_t(r) * kBreedRowBytes;
  std::memcpy(entry, row, sizeof(*entry));
  std::memcpy(tab, row + 64, sizeof(tab));
  bool ok = entry->slot >= 0 && entry->slot < cap;
  for (int w = 0; w < 2 && ok; ++w) {
    ok = tab[w][0] == 0;
    for (int y = 0; y < EG_YEARS && ok; ++y) ok = tab[w][y + 1] >= tab[w][y] && tab[w][y + 1] <= int32_t(snap::kBestCap);
  }
  return ok;
}
int eg::archive_fetch_record(eg_ctx* c, int32_t slot, const eg_episode_out* out, size_t r) {
  if (!out) return EG_OK;
  eg_episode_out row = out_row(out, r);
  return fetch_records(c->d_breed + breed_at::records + size_t(slot) * rec::stride, 1, &row);
}
int eg::decode_device_blocks(const uint8_t* d_blocks, int32_t n, const int32_t* slots, const char* who, eg_plan_set** set) {
  std::vector<uint8_t> blocks(size_t(n) * snap::kPlanStride);
  if (!slots) EG_HIP(hipMemcpy(blocks.data(), d_blocks, blocks.size(), hipMemcpyDeviceToHost));
  else
    for (int32_t r = 0; r < n; ++r)
      EG_HIP(hipMemcpy(blocks.data() + size_t(r) * snap::kPlanStride, d_blocks + size_t(slots[r]) * snap::kPlanStride, snap::kPlanStride, hipMemcpyDeviceToHost));
  return decode_plan_blocks(blocks.data(), n, who, set);
}

// ---------------------------------------------------------------- option checks
int32_t eg::check_mode(const Fail& fail, int32_t mode) {
  const int32_t rank = pareto_rank_mode(mode);      // (EG_PARETO_KEEP_SPREAD may be OR-ed into either; the message is the one the tests pin)
  return rank != 1 && rank != 2 ? fail("mode " + std::to_string(mode) + " is neither 1 (optimization_mode None) nor 2 (cost_only)") : EG_OK;
}
int32_t eg::check_objectives(const Fail& fail, int32_t objectives) {
  return objectives < 1 || objectives > 15 ? fail("objectives " + std::to_string(objectives) + " is outside 1..15 (bit i = metric i)") : EG_OK;
}
int32_t eg::check_cap(const Fail& fail, int32_t cap) {
  return cap < 1 || cap > EG_PARETO_MAX ? fail("cap " + std::to_string(cap) + " is outside 1..EG_PARETO_MAX (" + std::to_string(EG_PARETO_MAX) + ")") : EG_OK;
}
int32_t eg::check_launch_variants(const Fail& fail, int32_t launch_variants) {
  if (launch_variants >= 0 && launch_variants <= EG_CROSS_MAX_VARIANTS) return EG_OK;
  return fail("launch_variants = " + std::to_string(launch_variants) + " (1.." + std::to_string(EG_CROSS_MAX_VARIANTS) + "; 0: " + std::to_string(EG_CROSS_MAX_VARIANTS) + ")");
}
int32_t eg::check_repair_weights(const Fail& fail, const double* weights, int32_t k) {
  if (k < 1) return fail("no plan constraints are set (eg_plan_constraints_set first: a repair descends on their violation)");
  if (k > EG_CONSTRAINTS_MAX) return fail("k = " + std::to_string(k) + " constraints (at most " + std::to_string(EG_CONSTRAINTS_MAX) + ")");
  for (int32_t i = 0; weights && i < k; ++i)
    if (!std::isfinite(weights[i]) || !(weights[i] > 0.0)) return fail("weights[" + std::to_string(i) + "] = " + std::to_string(weights[i]) + " (finite and > 0)");
  return EG_OK;
}
int32_t eg::validate_action_lists(const Fail& fail, int32_t n_replace, const uint8_t* replace_with, int32_t n_append, const uint8_t* append_with) {
  const char* name[2] = {"replace_with", "append_with"};
  const int32_t count[2] = {n_replace, n_append};
  const uint8_t* list[2] = {replace_with, append_with};
  for (int k = 0; k < 2; ++k) {
    const std::string n_name = k == 0 ? "n_replace" : "n_append";
    if (count[k] < 0) return fail(n_name + " = " + std::to_string(count[k]));
    if (count[k] > 0 && !list[k]) return fail(std::string("NULL ") + name[k] + " with " + n_name + " = " + std::to_string(count[k]));
    for (int32_t i = 0; i < count[k]; ++i)
      if (list[k][i] >= EG_N_ACTIONS) return fail(std::string(name[k]) + "[" + std::to_string(i) + "]: action " + std::to_string(int(list[k][i])) + " >= " + std::to_string(EG_N_ACTIONS));
  }
  return EG_OK;
}
