// eg_breed.cpp — eg_breed_plans: generations of plan crosses with Pareto selection (include/eirgrid_hip.h), and its validator.  The host
// enumerates a generation's variants from the population's prefix offsets, uploads 8 bytes a variant and the routing chunk by chunk, and
// reads one buffer back per generation; the blocks stay on the device (eg_breed.h k_breed_gather, k_breed_turnover).  The archive and
// the shared option checks are eg_plan_host.cpp's.
#include <algorithm>
#include <cstring>

#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_breed_opts) == 40 && sizeof(eg_breed_generation) == 40 && sizeof(eg_breed_member) == 56, "the breed structs are part of the C ABI");
static_assert(EG_CROSS_MAX_PARENTS == EG_PARETO_MAX, "a whole archive is a parent set");

extern "C" int32_t eg_breed_validate(const eg_plan_set* parents, const eg_breed_opts* bo) {
  auto fail = [](const std::string& m) { set_error("eg_breed_validate: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(eg_plans_validate(parents));
  EG_TRY(validate_front_opts(fail, parents, bo));
  EG_TRY(check_launch_variants(fail, bo->launch_variants));
  if (bo->n_cuts < 0 || bo->n_cuts > EG_YEARS - 1) return fail("n_cuts = " + std::to_string(bo->n_cuts) + " (0.." + std::to_string(EG_YEARS - 1) + "; 0: every cut)");
  if (bo->n_cuts > 0 && !bo->cuts) return fail("NULL cuts with n_cuts = " + std::to_string(bo->n_cuts));
  for (int32_t i = 0; i < bo->n_cuts; ++i)
    if (bo->cuts[i] < 1 || bo->cuts[i] > EG_YEARS - 1)
      return fail("cuts[" + std::to_string(i) + "] = " + std::to_string(int(bo->cuts[i])) + " (a year index 1.." + std::to_string(EG_YEARS - 1) + ")");
  return EG_OK;
}

static const char* const kFn = "eg_breed_plans";

extern "C" int32_t eg_breed_plans(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const eg_plan_set* parents, const eg_breed_opts* bo, uint64_t seed,
                                  uint64_t episode_index, eg_plan_set** population, eg_breed_generation* generations, eg_breed_member* members,
                                  int32_t* n_generations, int32_t* stop_reason, eg_episode_out* out) {
  if (!c || !s || !s->weights || !s->deficit_weights || !population || !generations || !members || !n_generations || !stop_reason) {
    set_error(std::string(kFn) + ": bad argument"); return EG_ERR_BAD_ARG;
  }
  EG_TRY(plan_entry(c, s, o, kFn, [&] { return eg_breed_validate(parents, bo); }));
  const uint32_t L = bo->launch_variants == 0 ? uint32_t(EG_CROSS_MAX_VARIANTS) : uint32_t(bo->launch_variants);
  std::vector<uint8_t> cuts(bo->cuts, bo->cuts + bo->n_cuts);
  if (cuts.empty()) for (int y = 1; y < EG_YEARS; ++y) cuts.push_back(uint8_t(y));
  // the private archive, started empty (a call that failed may have left anything behind); generation 0: the parents' blocks go up, as
  // eg_evaluate_plan_crosses stages them; no block goes up after this
  EG_TRY(archive_begin(c, bo->cap, bo->objectives, bo->mode));
  EG_TRY(archive_upload(c, parents, 0));
  EG_HIP(c->d_plan_edit_in.reserve(size_t(EG_CROSS_MAX_VARIANTS) * 8));
  DevSnapshot S{};
  EG_TRY(stage_eval_snapshot(c, s, o, &S));
  std::vector<int32_t> off[2];
  parent_offsets(parents, off);
  int32_t n = parents->n_plans;
  int cur = 0;
  std::vector<eg_plan_cross> variants;
  std::vector<uint32_t> packed;
  Routing R;
  std::vector<uint8_t> rb;
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
      packed.assign(size_t(m) * 2, 0u); R.clear();
      for (uint32_t j = 0; j < m; ++j) {
        const eg_plan_cross& x = variants[first + j];
        pack_plan_cross(x, packed.data() + 2 * size_t(j));
        R.add(j, child_len(off[0], x));
      }
      const uint32_t n_short = R.finish();
      // (synchronous copies on the null stream: they wait for the previous chunk, whose kernels read what they overwrite)
      EG_HIP(hipMemcpy(c->d_plan_edit_in, packed.data(), size_t(m) * 8, hipMemcpyHostToDevice));
      EG_HIP(hipMemcpy(c->d_plan_index, R.idx.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice));
      EG_LAUNCH("k_plan_crosses", launch_plan_crosses(archive_array(c, cur), uint32_t(n), c->d_plan_edit_in, m, c->d_plans, nullptr));
      c->n_plan_blocks = m;
      EG_TRY(launch_plans(c, S, seed, episode_index, m, n_short, true));
      EG_TRY(archive_fold(c, m, uint64_t(first)));
    }
    EG_LAUNCH("k_breed_turnover", launch_breed_turnover(c->d_breed, 1 - cur, nullptr));
    EG_TRY(archive_read_generation(c, rb));
    BreedHeader h{};
    std::memcpy(&h, rb.data(), sizeof(h));
    if (h.n_held < 0 || h.n_held > bo->cap || h.n_valid < 0 || h.n_valid > int64_t(V) || (h.n_held == 0) != (h.n_valid == 0)) {
      set_error(at + "the device's readback header is corrupt"); return EG_ERR_INTERNAL;
    }
    G.n_kept = h.n_held; G.n_valid = h.n_valid; G.n_dropped = h.n_dropped;
    *n_generations = g + 1;
    if (h.n_held == 0) {      // no valid variant: the population of this generation stands in the current parent array
      *stop_reason = EG_BREED_EMPTY;
      return decode_device_blocks(archive_array(c, cur), n, nullptr, kFn, population);
    }
    std::vector<int32_t> next_off[2];
    next_off[0].assign(size_t(h.n_held) * 27, 0); next_off[1].assign(size_t(h.n_held) * 27, 0);
    slots.assign(size_t(h.n_held), 0);
    bool only_parents = h.n_held == n;
    long long before = -1;
    for (int32_t r = 0; r < h.n_held; ++r) {
      ParetoEntry e{};
      int32_t tab[2][28];
      bool ok = archive_row(rb, r, bo->cap, &e, tab) && e.index > before && e.index < (long long)V;
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
  for (int32_t r = 0; r < n; ++r) EG_TRY(archive_fetch_record(c, slots[size_t(r)], out, size_t(r)));
  return decode_device_blocks(archive_array(c, cur), n, nullptr, kFn, population);
}
