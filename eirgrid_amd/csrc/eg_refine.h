// eg_refine.h — what the pick of a refinement round reduces with (namespace refine): the order of two (score, index) pairs and the best
// pair of a wave.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_edits.h and before eg_refine_many.h, whose
// k_refine_pick_many is the one kernel that uses them.
//
// A round evaluates the variants of a base plan (their blocks written from the base block, their records by the plan batch).  Variant j is a
// CANDIDATE when its record's status is EG_EP_OK and s_j = rm::rank_score(its 4 metrics, mode) is not NaN; the winner is the candidate
// with the largest s_j, ties to the lowest j.  A thread holds the best pair of the variants it looked at; wave_best reduces the pairs of a
// wave with DPP row shifts and row broadcasts (the combine is idempotent, so a lane without a DPP source combines with itself), and the
// waves of a workgroup meet through ONE LDS exchange that every thread folds for itself.  No scratch memory.
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
