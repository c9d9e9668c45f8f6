// eg_refine.h — k_refine_pick: the step of a greedy plan refinement (include/eirgrid_hip.h eg_refine_plan) that stays on the device.
// One workgroup on the null stream behind a round's rollout grids.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_edits.h.
//
// A round evaluates n variants of the base plan (k_plan_edits wrote their blocks, the plan batch their records).  Variant j is a
// CANDIDATE when its record's status is EG_EP_OK and s_j = rm::rank_score(its 4 metrics, mode) is not NaN; the winner is the candidate
// with the largest s_j, ties to the lowest j.  The kernel
//   reads    status and metrics straight from the records (32 + 4 bytes of each 12 KB record), a thread a variant, striding by the
//            workgroup's width when there are more variants than threads — the trip count is the same for every thread;
//   reduces  (score, index) per wave with DPP row shifts and row broadcasts (the combine is idempotent, so a lane without a DPP source
//            combines with itself), then across the sixteen waves through ONE LDS exchange that every thread folds for itself;
//   counts   the variants that are no candidates, a ballot per trip;
//   writes   one RefineEntry (eg_internal.h): winner, its packed edit, score, metrics, the count, the list totals of the winner's block,
//            and what variant 0 scored;
//   copies   the winner's plan block over the base block when the winner is not variant 0 — 552 16-byte vector stores, one per thread
//            of the same workgroup — so that the next round's k_plan_edits finds its base where the host uploaded the first one.
// No scratch memory; every index read from memory or computed from one is clamped.
#pragma once

namespace refine {

constexpr int kThreads = 1024, kWaves = kThreads / kWave;
constexpr int kNoIndex = 0x7FFFFFFF;
static_assert(snap::kPlanStride % 16 == 0 && snap::kPlanStride / 16 <= (size_t)kThreads, "a 16-byte store per thread copies a plan block");

// does (sa, ja) rank before (sb, jb)?  (no candidate: -inf, kNoIndex)
__device__ __forceinline__ bool before(double sa, int ja, double sb, int jb) { return sa > sb || (sa == sb && ja < jb); }

// the best (score, index) of the wave, in every lane
__device__ __forceinline__ void wave_best(double& s, int& j) {
#define EG_DPP_BEST_STEP(ctrl, row_mask, bank_mask)                                                                         \
  {                                                                                                                          \
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(s), __double2loint(s), ctrl, row_mask, bank_mask, false);       \
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(s), __double2hiint(s), ctrl, row_mask, bank_mask, false);       \
    const int oj = __builtin_amdgcn_update_dpp(j, j, ctrl, row_mask, bank_mask, false);                                       \
    const double os = __hiloint2double(hi, lo);                                                                              \
    if (before(os, oj, s, j)) { s = os; j = oj; }                                                                            \
  }
  EG_DPP_BEST_STEP(0x111, 0xf, 0xf)   // row_shr:1
  EG_DPP_BEST_STEP(0x112, 0xf, 0xf)   // row_shr:2
  EG_DPP_BEST_STEP(0x113, 0xf, 0xf)   // row_shr:3
  EG_DPP_BEST_STEP(0x114, 0xf, 0xe)   // row_shr:4 bank_mask:0xe
  EG_DPP_BEST_STEP(0x118, 0xf, 0xc)   // row_shr:8 bank_mask:0xc
  EG_DPP_BEST_STEP(0x142, 0xa, 0xf)   // row_bcast:15 row_mask:0xa
  EG_DPP_BEST_STEP(0x143, 0xc, 0xf)   // row_bcast:31 row_mask:0xc
#undef EG_DPP_BEST_STEP
  s = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), 63), __builtin_amdgcn_readlane(__double2loint(s), 63));
  j = __builtin_amdgcn_readlane(j, 63);
}

}  // namespace refine

__global__ void __launch_bounds__(1024) k_refine_pick(DevOut O, uint32_t n, int mode, const uint2* __restrict__ edits, const uint8_t* __restrict__ pool,
                                                      uint8_t* __restrict__ base, RefineEntry* __restrict__ entry) {
  using namespace refine;
  __shared__ double s_score[kWaves];
  __shared__ int s_index[kWaves], s_fail[kWaves];
  __shared__ int s_base_ok;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  double best = -__builtin_huge_val();
  int best_j = kNoIndex, fails = 0;
  for (uint32_t j0 = 0; j0 < n; j0 += (uint32_t)kThreads) {      // (uniform: the ballot below wants every lane)
    const uint32_t j = j0 + (uint32_t)tid;
    bool cand = false;
    double s = 0.0;
    if (j < n) {
      const double* m = O.metrics(j);
      const double mm[4] = {m[0], m[1], m[2], m[3]};
      s = rm::rank_score(mm, mode);
      cand = *O.status(j) == EG_EP_OK && s == s;
      if (j == 0u) {      // what the base scores: the start of the trajectory, and whether there is one
        s_base_ok = cand ? 1 : 0;
        entry->base_ok = cand ? 1 : 0; entry->base_score = s;
#pragma unroll
        for (int k = 0; k < 4; ++k) entry->base_metrics[k] = mm[k];
      }
    }
    fails += __popcll(__ballot(j < n && !cand));
    if (cand && before(s, (int)j, best, best_j)) { best = s; best_j = (int)j; }      // (the reductions' order: a candidate that scores -inf is recorded as well)
  }
  wave_best(best, best_j);
  if (lane == 0) { s_score[wave] = best; s_index[wave] = best_j; s_fail[wave] = fails; }
  __syncthreads();
  best = -__builtin_huge_val(); best_j = kNoIndex; fails = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const double s = s_score[w];
    const int j = s_index[w];
    if (before(s, j, best, best_j)) { best = s; best_j = j; }
    fails += s_fail[w];
  }
  const bool base_ok = s_base_ok != 0;
  // (a candidate base is itself in the running, so there is a winner; the clamp is for a record that lies about it)
  const int winner = base_ok ? (best_j < 0 ? 0 : (best_j >= (int)n ? (int)n - 1 : best_j)) : -1;
  const uint32_t w = winner < 0 ? 0u : (uint32_t)winner;
  const uint8_t* blk = pool + (size_t)w * snap::kPlanStride;
  if (tid == 0) {
    const uint2 e = edits[w];
    const double* m = O.metrics(w);
    entry->winner = winner; entry->n_failed = fails;
    entry->edit[0] = e.x; entry->edit[1] = e.y;
    entry->score = base_ok ? best : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) entry->metrics[k] = m[k];
    entry->off26 = reinterpret_cast<const int32_t*>(blk + pedit::kOffOff)[EG_YEARS];
    entry->offd26 = reinterpret_cast<const int32_t*>(blk + pedit::kOffDOff)[EG_YEARS];
    entry->n = (int32_t)n;
  }
  if (winner > 0 && tid < (int)(snap::kPlanStride / 16)) reinterpret_cast<uint4*>(base)[tid] = reinterpret_cast<const uint4*>(blk)[tid];
}
