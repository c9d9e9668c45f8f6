// eg_repair.h — k_repair_pick_many: the pick of a repair round (include/eirgrid_hip.h eg_repair_plans; the host loop is eg_refine.cpp's, with
// the repair rule).  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_constraints.h: the kernel reads what k_plan_constraints left.
//
// A launch is a launch of eg_refine_plans_moves — SEGMENT s the variants [first_s, first_s + n_s) of one plan, its base block in slot_s —
// judged under the context's k constraints; behind the rollout grids and k_plan_constraints, on the null stream, workgroup s
//   reads    per variant of ITS segment the status and the 4 metrics from the record, the mask from `violated` and the k doubles of its
//            row of `excess`, a thread a variant, striding by the workgroup's width with the same trip count for every thread;
//   folds    V_j = sum over i of (NaN excess: +inf; excess > 0: w_i * excess; else +0.0), from +0.0 in constraint order, a multiplication
//            and an addition per constraint, each rounded once (the build forms no FMA);
//   reduces  the key (V ascending, score descending, index ascending) over the candidates — status EG_EP_OK or EG_EP_INFEASIBLE and a rank
//            score that is not NaN — per wave with the DPP steps of refine::wave_best and across the sixteen waves through one LDS
//            exchange that every thread folds for itself.  The base (variant 0) is in the running: the best key's V is the smallest V of
//            the segment, so the winner — the best candidate with V_j < V_0 — exists iff that V is below V_0, and then it IS the best key;
//   counts   the variants that are no candidates and the candidates with V == 0, a ballot each per trip;
//   writes   entry s (RepairEntry, eg_internal.h): winner -1 when the base is no candidate, 0 when V_0 == 0 or nothing lies below V_0;
//   copies   the winner's plan block over base block slot_s when winner > 0 — 552 16-byte vector stores, one per thread.
// Every index read from memory or computed from one is clamped; an empty segment (no host launch describes one) writes an entry that
// says so and copies nothing.  No thread returns ahead of the barrier.  No scratch memory, no atomics; LDS is the exchange alone.
// The kernel lives in a namespace of its own, `repair`: the resource tests select kernels by a substring of the mangled name, and neither
// `repair` nor k_repair_pick_many contains one of theirs (tests/test_repair_resources.py looks for the full name).
#pragma once

namespace repair {

using refine::kNoIndex;
using refine::kThreads;
using refine::kWaves;

// does (va, sa, ja) rank before (vb, sb, jb)?  (no candidate: +inf, -inf, kNoIndex)
__device__ __forceinline__ bool before(double va, double sa, int ja, double vb, double sb, int jb) {
  return va < vb || (va == vb && (sa > sb || (sa == sb && ja < jb)));
}

// the best (V, score, index) of the wave, in every lane: refine::wave_best's steps with the second key
__device__ __forceinline__ void wave_best(double& v, double& s, int& j) {
#define EG_DPP_PART(x, ctrl, row_mask, bank_mask) __builtin_amdgcn_update_dpp(x, x, ctrl, row_mask, bank_mask, false)
#define EG_DPP_REPAIR_STEP(ctrl, row_mask, bank_mask)                                                                                     \
  {                                                                                                                                        \
    const double ov = __hiloint2double(EG_DPP_PART(__double2hiint(v), ctrl, row_mask, bank_mask), EG_DPP_PART(__double2loint(v), ctrl, row_mask, bank_mask)); \
    const double os = __hiloint2double(EG_DPP_PART(__double2hiint(s), ctrl, row_mask, bank_mask), EG_DPP_PART(__double2loint(s), ctrl, row_mask, bank_mask)); \
    const int oj = EG_DPP_PART(j, ctrl, row_mask, bank_mask);                                                                              \
    if (before(ov, os, oj, v, s, j)) { v = ov; s = os; j = oj; }                                                                           \
  }
  EG_DPP_REPAIR_STEP(0x111, 0xf, 0xf)   // row_shr:1
  EG_DPP_REPAIR_STEP(0x112, 0xf, 0xf)   // row_shr:2
  EG_DPP_REPAIR_STEP(0x113, 0xf, 0xf)   // row_shr:3
  EG_DPP_REPAIR_STEP(0x114, 0xf, 0xe)   // row_shr:4 bank_mask:0xe
  EG_DPP_REPAIR_STEP(0x118, 0xf, 0xc)   // row_shr:8 bank_mask:0xc
  EG_DPP_REPAIR_STEP(0x142, 0xa, 0xf)   // row_bcast:15 row_mask:0xa
  EG_DPP_REPAIR_STEP(0x143, 0xc, 0xf)   // row_bcast:31 row_mask:0xc
#undef EG_DPP_REPAIR_STEP
#undef EG_DPP_PART
  v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
  s = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), 63), __builtin_amdgcn_readlane(__double2loint(s), 63));
  j = __builtin_amdgcn_readlane(j, 63);
}

// workgroup s: segment s of the launch's n_total variants, judged under k constraints with the weights w[0..k)
__global__ void __launch_bounds__(1024) k_repair_pick_many(DevOut O, const refine::Segment* __restrict__ segs, uint32_t n_total, int mode,
                                                           const uint2* __restrict__ edits, const uint8_t* __restrict__ pool, uint8_t* __restrict__ bases,
                                                           uint32_t n_bases, const uint32_t* __restrict__ violated, const double* __restrict__ excess, uint32_t k,
                                                           const double* __restrict__ weights, uint8_t* __restrict__ entries) {
  __shared__ double s_v[kWaves], s_score[kWaves], s_base_v;
  __shared__ int s_index[kWaves], s_fail[kWaves], s_feas[kWaves];
  __shared__ int s_base_ok;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const refine::Segment sg = segs[blockIdx.x];
  RepairEntry* entry = reinterpret_cast<RepairEntry*>(entries + (size_t)blockIdx.x * kRefineEntryStride);
  k = k > (uint32_t)EG_CONSTRAINTS_MAX ? (uint32_t)EG_CONSTRAINTS_MAX : k;
  // the segment inside the launch (uniform in the workgroup); an empty one runs no trip and leaves no candidate
  const uint32_t first = sg.first < n_total ? sg.first : n_total;
  const uint32_t n = n_bases == 0u ? 0u : (sg.count < n_total - first ? sg.count : n_total - first);
  const double inf = __builtin_huge_val();
  double best_v = inf, best_s = -inf;
  int best_j = kNoIndex, fails = 0, feas = 0;      // (variant indices relative to the segment)
  double base_v = 0.0, base_s = 0.0;               // (thread 0 keeps what the base came to)
  uint32_t base_mask = 0u;
  if (tid == 0) { s_base_ok = 0; s_base_v = 0.0; }      // (thread 0 alone writes them again, in its first trip)
  for (uint32_t j0 = 0; j0 < n; j0 += (uint32_t)kThreads) {      // (uniform: the ballots below want every lane)
    const uint32_t j = j0 + (uint32_t)tid;
    bool cand = false;
    double s = 0.0, v = 0.0;
    if (j < n) {
      const double* m = O.metrics(first + j);
      const double mm[4] = {m[0], m[1], m[2], m[3]};
      const int32_t st = *O.status(first + j);
      s = rm::rank_score(mm, mode);
      cand = (st == EG_EP_OK || st == EG_EP_INFEASIBLE) && s == s;
      const double* row = excess + (size_t)(first + j) * k;
      for (uint32_t i = 0; i < k; ++i) {      // in constraint order: a product and a sum per constraint, each rounded once
        const double e = row[i];
        const double t = e != e ? inf : (e > 0.0 ? weights[i] * e : 0.0);
        v = v + t;
      }
      if (j == 0u) {      // what the segment's base comes to
        s_base_ok = cand ? 1 : 0; s_base_v = v;
        base_v = v; base_s = s; base_mask = violated[first];
      }
    }
    fails += __popcll(__ballot(j < n && !cand));
    feas += __popcll(__ballot(cand && v == 0.0));
    if (cand && before(v, s, (int)j, best_v, best_s, best_j)) { best_v = v; best_s = s; best_j = (int)j; }
  }
  wave_best(best_v, best_s, best_j);
  if (lane == 0) { s_v[wave] = best_v; s_score[wave] = best_s; s_index[wave] = best_j; s_fail[wave] = fails; s_feas[wave] = feas; }
  __syncthreads();
  best_v = inf; best_s = -inf; best_j = kNoIndex; fails = 0; feas = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const double v = s_v[w], s = s_score[w];
    const int j = s_index[w];
    if (before(v, s, j, best_v, best_s, best_j)) { best_v = v; best_s = s; best_j = j; }
    fails += s_fail[w]; feas += s_feas[w];
  }
  const bool base_ok = s_base_ok != 0;
  const double v0 = s_base_v;
  // the winner: none below V_0 (or V_0 == 0: nothing lies below it) leaves the base; the clamp is for a record that lies
  const bool moves = base_ok && best_j > 0 && best_v < v0;
  const int winner = !base_ok ? -1 : (moves ? (best_j >= (int)n ? (int)n - 1 : best_j) : 0);
  if (n == 0u) {
    if (tid == 0) {
      entry->winner = -1; entry->n_failed = 0; entry->edit[0] = 0u; entry->edit[1] = 0u; entry->violation = 0.0; entry->score = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) entry->metrics[i] = 0.0;
      entry->violated = 0u; entry->n_feasible = 0; entry->off26 = 0; entry->offd26 = 0; entry->base_ok = 0; entry->n = 0;
      entry->base_violation = 0.0; entry->base_score = 0.0; entry->base_violated = 0u; entry->pad = 0u;
    }
  } else {
    const uint32_t w = first + (winner < 0 ? 0u : (uint32_t)winner);      // the winner among the launch's variants
    const uint8_t* blk = pool + (size_t)w * snap::kPlanStride;
    if (tid == 0) {
      const uint2 e = edits[w];
      const double* m = O.metrics(w);
      entry->winner = winner; entry->n_failed = fails;
      entry->edit[0] = e.x; entry->edit[1] = e.y;
      // (a base that is no candidate has no V and no score: zeros)
      entry->violation = !base_ok ? 0.0 : (winner > 0 ? best_v : base_v);
      entry->score = !base_ok ? 0.0 : (winner > 0 ? best_s : base_s);
#pragma unroll
      for (int i = 0; i < 4; ++i) entry->metrics[i] = m[i];
      entry->violated = base_ok ? violated[w] : 0u; entry->n_feasible = feas;
      entry->off26 = reinterpret_cast<const int32_t*>(blk + pblock::kOffOff)[EG_YEARS];
      entry->offd26 = reinterpret_cast<const int32_t*>(blk + pblock::kOffDOff)[EG_YEARS];
      entry->base_ok = base_ok ? 1 : 0; entry->n = (int32_t)n;
      entry->base_violation = base_ok ? base_v : 0.0; entry->base_score = base_ok ? base_s : 0.0;
      entry->base_violated = base_ok ? base_mask : 0u; entry->pad = 0u;
    }
    if (winner > 0 && tid < (int)(snap::kPlanStride / 16)) {
      uint8_t* base = bases + (size_t)(sg.slot < n_bases ? sg.slot : n_bases - 1u) * snap::kPlanStride;
      reinterpret_cast<uint4*>(base)[tid] = reinterpret_cast<const uint4*>(blk)[tid];
    }
  }
}

}  // namespace repair
