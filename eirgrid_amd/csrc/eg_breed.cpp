// eg_breed.cpp — eg_breed_plans: generations of plan crosses with Pareto selection (include/eirgrid_hip.h), and its validator.  The host
// enumerates a generation's variants from the population's prefix offsets, uploads 8 bytes a variant and the routing chunk by chunk, and
// reads one buffer back per generation; the blocks stay on the device (eg_breed.h k_breed_gather, k_breed_turnover).
#include <algorithm>
#include <cstring>

#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_breed_opts) == 40 && sizeof(eg_breed_generation) == 40 && sizeof(eg_breed_member) == 56, "the breed structs are part of the C ABI");
static_assert(EG_CROSS_MAX_PARENTS == EG_PARETO_MAX, "a whole archive is a parent set");

extern "C" int32_t eg_breed_validate(const eg_plan_set* parents, const eg_breed_opts* bo) {
  auto fail = [](const std::string& m) { set_error("eg_breed_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(parents));
  if (parents->n_plans > EG_CROSS_MAX_PARENTS)
    return fail("the set holds " + std::to_string(parents->n_plans) + " plans (at most " + std::to_string(EG_CROSS_MAX_PARENTS) + ")");
  if (!bo) return fail("NULL options");
  if (bo->mode != 1 && bo->mode != 2) return fail("mode " + std::to_string(bo->mode) + " is neither 1 (optimization_mode None) nor 2 (cost_only)");
  if (bo->objectives < 1 || bo->objectives > 15) return fail("objectives " + std::to_string(bo->objectives) + " is outside 1..15 (bit i = metric i)");
  if (bo->cap < 1 || bo->cap > EG_PARETO_MAX) return fail("cap " + std::to_string(bo->cap) + " is outside 1..EG_PARETO_MAX (" + std::to_string(EG_PARETO_MAX) + ")");
  if (bo->max_generations < 1) return fail("max_generations = " + std::to_string(bo->max_generations) + " (at least 1)");
  if (bo->launch_variants < 0 || bo->launch_variants > EG_CROSS_MAX_VARIANTS)
    return fail("launch_variants = " + std::to_string(bo->launch_variants) + " (1.." + std::to_string(EG_CROSS_MAX_VARIANTS) + "; 0: " + std::to_string(EG_CROSS_MAX_VARIANTS) + ")");
  if (bo->n_cuts < 0 || bo->n_cuts > EG_YEARS - 1) return fail("n_cuts = " + std::to_string(bo->n_cuts) + " (0.." + std::to_string(EG_YEARS - 1) + "; 0: every cut)");
  if (bo->n_cuts > 0 && !bo->cuts) return fail("NULL cuts with n_cuts = " + std::to_string(bo->n_cuts));
  for (int32_t i = 0; i < bo->n_cuts; ++i)
    if (bo->cuts[i] < 1 || bo->cuts[i] > EG_YEARS - 1)
      return fail("cuts[" + std::to_string(i) + "] = " + std::to_string(int(bo->cuts[i])) + " (a year index 1.." + std::to_string(EG_YEARS - 1) + ")");
  return EG_OK;
}

namespace {
const char* const kFn = "eg_breed_plans";

// the blocks of a population as they stand on the device, decoded into a plan set (the reverse of write_lists)
int decode_population(const uint8_t* d_blocks, int32_t n, eg_plan_set** population) {
  std::vector<uint8_t> blocks(size_t(n) * snap::kPlanStride);
  EG_HIP(hipMemcpy(blocks.data(), d_blocks, blocks.size(), hipMemcpyDeviceToHost));
  return decode_plan_blocks(blocks.data(), n, kFn, population);
}
}  // namespace

extern "C" int32_t eg_breed_plans(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* parents, const eg_breed_opts* bo, uint64_t seed,
                                  uint64_t episode_index, eg_plan_set** population, eg_breed_generation* generations, eg_breed_member* members,
                                  int32_t* n_generations, int32_t* stop_reason, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !population || !generations || !members || !n_generations || !stop_reason) {
    set_error(std::string(kFn) + ": bad argument"); return EG_ERR_BAD_ARG;
  }
  if (c->group_member) { set_error(std::string(kFn) + ": the context is a rank of an eg_group (plan batches on a group are not supported)"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_breed_validate(parents, bo));
  EG_TRY(check_policy(s, o, kFn));
  EG_HIP(hipSetDevice(c->device));
  const uint32_t L = bo->launch_variants == 0 ? uint32_t(EG_CROSS_MAX_VARIANTS) : uint32_t(bo->launch_variants);
  std::vector<uint8_t> cuts(bo->cuts, bo->cuts + bo->n_cuts);
  if (cuts.empty()) for (int y = 1; y < EG_YEARS; ++y) cuts.push_back(uint8_t(y));
  // the private archive: allocated at the first call, started empty at every call (a call that failed may have left anything behind)
  EG_HIP(c->d_breed.reserve(breed_at::total));
  EG_HIP(c->d_breed_work.reserve(pareto_work_bytes(EG_CROSS_MAX_VARIANTS)));
  const ParetoWork work = pareto_work(c->d_breed_work, EG_CROSS_MAX_VARIANTS);
  uint8_t* const d_parents[2] = {c->d_breed + breed_at::parents, c->d_breed + breed_at::parents + breed_at::kParentArray};
  {
    ParetoState st{};
    st.cap = bo->cap; st.objectives = bo->objectives; st.mode = bo->mode;
    EG_HIP(hipMemcpy(c->d_breed, &st, sizeof(st), hipMemcpyHostToDevice));
    const BreedCounters zero{};
    EG_HIP(hipMemcpy(c->d_breed + breed_at::counters, &zero, sizeof(zero), hipMemcpyHostToDevice));
    // generation 0: the parents' blocks go up, as eg_evaluate_plan_crosses stages them; no block goes up after this
    std::vector<uint8_t> blocks(size_t(parents->n_plans) * snap::kPlanStride, 0);
    write_plan_blocks(parents, blocks.data());
    EG_HIP(hipMemcpy(d_parents[0], blocks.data(), blocks.size(), hipMemcpyHostToDevice));
  }
  EG_HIP(c->d_plan_edit_in.reserve(size_t(EG_CROSS_MAX_VARIANTS) * 8));
  DevSnapshot S{};
  EG_TRY(stage_eval_snapshot(c, s, o, &S));
  std::vector<int32_t> off[2];
  parent_offsets(parents, off);
  int32_t n = parents->n_plans;
  int cur = 0;
  std::vector<eg_plan_cross> variants;
  std::vector<uint32_t> packed, idx, longs;
  std::vector<uint8_t> rb(breed_at::kReadbackBytes);
  std::vector<int32_t> slots;      // the record slots of the last generation's survivors
  *n_generations = 0; *stop_reason = EG_BREED_MAX_GENERATIONS;
  for (int32_t g = 0; g < bo->max_generations; ++g) {
    const std::string at = std::string(kFn) + ": generation " + std::to_string(g) + ": ";
    eg_breed_generation& G = generations[g];
    G = eg_breed_generation{};
    G.n_parents = n;
    variants.clear();
    for (int32_t p = 0; p < n; ++p) variants.push_back(eg_plan_cross{uint16_t(p), uint16_t(p), 0, 0});
    for (int32_t a = 0; a < n; ++a)
      for (int32_t b = 0; b < n; ++b) {
        if (b == a) continue;
        for (const uint8_t cut : cuts) {
          const eg_plan_cross x{uint16_t(a), uint16_t(b), cut, uint8_t(EG_YEARS)};
          if (child_len(off[0], x) > int64_t(snap::kBestCap) || child_len(off[1], x) > int64_t(snap::kBestCap)) { G.n_skipped += 1; continue; }
          variants.push_back(x);
        }
      }
    const size_t V = variants.size();
    G.n_variants = int64_t(V);
    const uint32_t n_cap = uint32_t(std::min<size_t>(V, L));
    EG_TRY(ensure_outputs(c, n_cap));
    EG_HIP(c->d_plans.reserve(size_t(n_cap) * snap::kPlanStride));
    EG_HIP(c->d_plan_index.reserve(n_cap));
    S.plan_pool = c->d_plans;      // (the pool may have been a smaller one, or none, when the snapshot was staged)
    for (size_t first = 0; first < V; first += L) {
      const uint32_t m = uint32_t(std::min<size_t>(V - first, L));
      packed.assign(size_t(m) * 2, 0u); idx.clear(); longs.clear();
      for (uint32_t j = 0; j < m; ++j) {
        const eg_plan_cross& x = variants[first + j];
        pack_plan_cross(x, packed.data() + 2 * size_t(j));
        (child_len(off[0], x) > kShortReplayMax ? longs : idx).push_back(j);
      }
      const uint32_t n_short = uint32_t(idx.size());
      idx.insert(idx.end(), longs.begin(), longs.end());
      // (synchronous copies on the null stream: they wait for the previous chunk, whose kernels read what they overwrite)
      EG_HIP(hipMemcpy(c->d_plan_edit_in, packed.data(), size_t(m) * 8, hipMemcpyHostToDevice));
      EG_HIP(hipMemcpy(c->d_plan_index, idx.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice));
      EG_LAUNCH("k_plan_crosses", launch_plan_crosses(d_parents[cur], uint32_t(n), c->d_plan_edit_in, m, c->d_plans, nullptr));
      c->n_plan_blocks = m;
      EG_TRY(launch_plans(c, S, seed, episode_index, m, n_short, true));
      EG_LAUNCH("k_pareto_filter .. k_pareto_finalize", launch_pareto_fold(c->d_breed, work, c->out, m, uint64_t(first), nullptr));
      EG_LAUNCH("k_breed_gather", launch_breed_gather(c->d_breed, c->out, m, uint64_t(first), c->d_plans, nullptr));
    }
    EG_LAUNCH("k_breed_turnover", launch_breed_turnover(c->d_breed, 1 - cur, nullptr));
    EG_HIP(hipMemcpy(rb.data(), c->d_breed + breed_at::readback, rb.size(), hipMemcpyDeviceToHost));      // (waits for the generation)
    BreedHeader h{};
    std::memcpy(&h, rb.data(), sizeof(h));
    if (h.n_held < 0 || h.n_held > bo->cap || h.n_valid < 0 || h.n_valid > int64_t(V) || (h.n_held == 0) != (h.n_valid == 0)) {
      set_error(at + "the device's readback header is corrupt"); return EG_ERR_INTERNAL;
    }
    G.n_kept = h.n_held; G.n_valid = h.n_valid; G.n_dropped = h.n_dropped;
    *n_generations = g + 1;
    if (h.n_held == 0) {      // no valid variant: the population of this generation stands in the current parent array
      *stop_reason = EG_BREED_EMPTY;
      return decode_population(d_parents[cur], n, population);
    }
    std::vector<int32_t> next_off[2];
    next_off[0].assign(size_t(h.n_held) * 27, 0); next_off[1].assign(size_t(h.n_held) * 27, 0);
    slots.assign(size_t(h.n_held), 0);
    bool only_parents = h.n_held == n;
    long long before = -1;
    for (int32_t r = 0; r < h.n_held; ++r) {
      const uint8_t* row = rb.data() + kBreedHeaderBytes + size_t(r) * kBreedRowBytes;
      ParetoEntry e{};
      std::memcpy(&e, row, sizeof(e));
      int32_t tab[2][28];
      std::memcpy(tab, row + 64, sizeof(tab));
      bool ok = e.index > before && e.index < (long long)V && e.slot >= 0 && e.slot < bo->cap;
      for (int w = 0; w < 2 && ok; ++w) {
        ok = tab[w][0] == 0;
        for (int y = 0; y < EG_YEARS && ok; ++y) ok = tab[w][y + 1] >= tab[w][y] && tab[w][y + 1] <= int32_t(snap::kBestCap);
      }
      // the block against the host's count: the survivor's list lengths are its cross's
      ok = ok && tab[0][EG_YEARS] == child_len(off[0], variants[size_t(e.index)]) && tab[1][EG_YEARS] == child_len(off[1], variants[size_t(e.index)]);
      if (!ok) { set_error(at + "the device's readback row " + std::to_string(r) + " does not describe a variant of the generation"); return EG_ERR_INTERNAL; }
      before = e.index;
      eg_breed_member& M = members[size_t(g) * size_t(bo->cap) + size_t(r)];
      M = eg_breed_member{};
      M.cross = variants[size_t(e.index)]; M.variant = int32_t(e.index); M.score = e.score;
      std::memcpy(M.metrics, e.metrics, sizeof(M.metrics));
      if (e.index >= n) { G.n_children_kept += 1; only_parents = false; }
      slots[size_t(r)] = e.slot;
      for (int w = 0; w < 2; ++w) std::copy(tab[w], tab[w] + 27, next_off[w].begin() + size_t(r) * 27);
    }
    cur = 1 - cur; n = h.n_held;
    off[0].swap(next_off[0]); off[1].swap(next_off[1]);
    if (only_parents) { *stop_reason = EG_BREED_CONVERGED; break; }
  }
  if (out)
    for (int32_t r = 0; r < n; ++r) {
      eg_episode_out row = out_row(out, size_t(r));
      EG_TRY(fetch_records(c->d_breed + breed_at::records + size_t(slots[size_t(r)]) * rec::stride, 1, &row));
    }
  return decode_population(d_parents[cur], n, population);
}
