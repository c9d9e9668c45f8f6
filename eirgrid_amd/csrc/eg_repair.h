// eg_repair.h — k_repair_pick_many: the pick of a repair round (include/eirgrid_hip.h eg_repair_plans; the host loop is eg_refine.cpp's, with
// the repair rule).  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_constraints.h: the kernel reads what k_plan_constraints left.
//
// A launch is a launch of eg_refine_plans_moves judged under the context's k constraints; behind the rollout grids and k_plan_constraints
// a workgroup per segment runs eg_pick.h's pick_segment under the repair RULE, which
//   reads    per variant, besides what the body read, the k doubles of its row of `excess`, and for the entry the masks in `violated`;
//   folds    V_j = sum over i of (NaN excess: +inf; excess > 0: w_i * excess; else +0.0), from +0.0 in constraint order, a multiplication
//            and an addition per constraint, each rounded once (the build forms no FMA);
//   judges   a variant a candidate when its status is EG_EP_OK or EG_EP_INFEASIBLE and its rank score is not NaN, with the key
//            (V ascending, score descending, index ascending);
//   counts   the candidates with V == 0;
//   picks    the best candidate with V_j < V_0.  The base (variant 0) is in the running: the best key's V is the smallest V of the
//            segment, so that winner exists iff that V is below V_0, and then it IS the best key; else 0 (V_0 == 0, or nothing below V_0);
//   adds     to the entry (RepairEntry, eg_internal.h) the winner's V, score and mask, the count, and the base's — all of them zero when
//            the base is no candidate.
// k is clamped here.
// The kernel lives in a namespace of its own, `repair`: the resource tests select kernels by a substring of the mangled name, and neither
// `repair` nor k_repair_pick_many contains one of theirs (tests/test_repair_resources.py looks for the full name).
#pragma once

namespace repair {

// (V ascending, score descending, index ascending)
struct ViolationKey {
  double v, s; int j;
  static constexpr int kWords = 5;
  static __device__ __forceinline__ ViolationKey none() { return {__builtin_huge_val(), -__builtin_huge_val(), refine::kNoIndex}; }
  __device__ __forceinline__ bool before(const ViolationKey& o) const { return v < o.v || (v == o.v && (s > o.s || (s == o.s && j < o.j))); }
};

struct RepairRule {
  using Key = ViolationKey;
  using Entry = RepairEntry;
  const uint32_t* __restrict__ violated;
  const double* __restrict__ excess;
  uint32_t k;
  const double* __restrict__ weights;
  __device__ __forceinline__ bool judge(const refine::Variant& x, uint32_t w, int j, Key& key) const {
    const double* row = excess + (size_t)w * k;
    double v = 0.0;
    for (uint32_t i = 0; i < k; ++i) {      // in constraint order: a product and a sum per constraint, each rounded once
      const double e = row[i];
      const double t = e != e ? __builtin_huge_val() : (e > 0.0 ? weights[i] * e : 0.0);
      v = v + t;
    }
    key = {v, x.score, j};
    return (x.status == EG_EP_OK || x.status == EG_EP_INFEASIBLE) && x.score == x.score;
  }
  __device__ __forceinline__ bool counts(const Key& key) const { return key.v == 0.0; }
  __device__ __forceinline__ int winner(const Key& best, const Key& base) const { return best.j > 0 && best.v < base.v ? best.j : 0; }
  __device__ __forceinline__ void fill(Entry& e, const Key& best, const Key& base, const refine::Variant&, uint32_t first, uint32_t w, int counted) const {
    e.n_feasible = counted;
    if (!e.base_ok) return;      // (a base that is no candidate has no V and no score: zeros)
    const Key& won = e.winner > 0 ? best : base;
    e.violation = won.v; e.score = won.s; e.violated = violated[w];
    e.base_violation = base.v; e.base_score = base.s; e.base_violated = violated[first];
  }
};

// workgroup s: segment s of the launch's n_total variants, judged under k constraints with the weights w[0..k)
__global__ void __launch_bounds__(1024) k_repair_pick_many(DevOut O, const refine::Segment* __restrict__ segs, uint32_t n_total, int mode,
                                                           const uint2* __restrict__ edits, const uint8_t* __restrict__ pool, uint8_t* __restrict__ bases,
                                                           uint32_t n_bases, const uint32_t* __restrict__ violated, const double* __restrict__ excess, uint32_t k,
                                                           const double* __restrict__ weights, uint8_t* __restrict__ entries) {
  const RepairRule rule{violated, excess, k > (uint32_t)EG_CONSTRAINTS_MAX ? (uint32_t)EG_CONSTRAINTS_MAX : k, weights};
  refine::pick_segment(rule, O, segs, n_total, mode, edits, pool, bases, n_bases, entries);
}

}  // namespace repair
