// eg_refine_many.h — k_plan_edits_many and k_refine_pick_many: a refinement round in one launch, of one plan (include/eirgrid_hip.h
// eg_refine_plan) or of many (eg_refine_plans); the host loop of both is eg_refine.cpp.  Included by eg_rollout.hip (eg_rollout.o only)
// behind eg_pick.h.
//
// A launch holds the variants of its plans back to back: SEGMENT s is the variants [first_s, first_s + n_s) of one plan, whose base
// block is block slot_s of a buffer of base blocks (one per plan of the call, uploaded once).
//   k_plan_edits_many   variant j's block from base block slot[j] and edit j: byte for byte what write_lists builds for the edited plan
//                       in a zeroed block; one wave per variant, 8-byte words, every store of a wave 512 consecutive bytes; no LDS, no
//                       scratch memory; writes inside block j only.  It is eg_plan_edits.h's write_edited_block, the body of k_plan_edits,
//                       with the slot indirection (eg_plan_block.h base_at) and the two start clamps that body's flag switches on.
//   k_refine_pick_many  one workgroup per segment: eg_pick.h's pick_segment under the refine RULE.  Variant j is a CANDIDATE when its
//                       record's status is EG_EP_OK and s_j = rm::rank_score(its 4 metrics, mode) is not NaN; the key is (score descending,
//                       index ascending), so the largest score wins, ties to the lowest variant; a candidate that scores -inf is recorded
//                       as well, and a candidate base is itself in the running, so the best key IS the winner.  The entry (RefineEntry,
//                       eg_internal.h) adds the winner's score — 0.0 when the base is no candidate — and what the base scored, written
//                       whether it is a candidate or not.
// The two kernels live in a namespace of their own, `many`: scripts/kernel_resources.sh prints a kernel by what is left of its mangled
// name, and the test that pins k_plan_edits' resource line picks it by the word k_plan_edits at the start of that name.  Behind the
// namespace the names print as many17k_plan_edits_many / many18k_refine_pick_many, which such a pattern does not take for it
// (tests/test_refine_many_resources.py looks for the full names).
#pragma once

namespace many {

__global__ void __launch_bounds__(256) k_plan_edits_many(const uint8_t* __restrict__ bases, uint32_t n_bases, const uint32_t* __restrict__ slot,
                                                         const uint2* __restrict__ edits, uint32_t n, uint8_t* __restrict__ pool) {
  const pblock::Wave w = pblock::my_variant();
  if (w.j >= n || n_bases == 0u) return;
  pedit::write_edited_block<true>(pblock::base_at(bases, n_bases, slot[w.j]), pedit::unpack(edits[w.j]), pool + (size_t)w.j * snap::kPlanStride, w.lane);
}

// (score descending, index ascending)
struct ScoreKey {
  double s; int j;
  static constexpr int kWords = 3;
  static __device__ __forceinline__ ScoreKey none() { return {-__builtin_huge_val(), refine::kNoIndex}; }
  __device__ __forceinline__ bool before(const ScoreKey& o) const { return s > o.s || (s == o.s && j < o.j); }
};

struct RefineRule {
  using Key = ScoreKey;
  using Entry = RefineEntry;
  __device__ __forceinline__ bool judge(const refine::Variant& x, uint32_t, int j, Key& key) const {
    key = {x.score, j};
    return x.status == EG_EP_OK && x.score == x.score;
  }
  __device__ __forceinline__ bool counts(const Key&) const { return false; }
  __device__ __forceinline__ int winner(const Key& best, const Key&) const { return best.j; }
  __device__ __forceinline__ void fill(Entry& e, const Key& best, const Key&, const refine::Variant& x0, uint32_t, uint32_t, int) const {
    e.score = e.base_ok ? best.s : 0.0;
    e.base_score = x0.score;
#pragma unroll
    for (int i = 0; i < 4; ++i) e.base_metrics[i] = x0.m[i];
  }
};

// workgroup s: segment s of the launch's n_total variants
__global__ void __launch_bounds__(1024) k_refine_pick_many(DevOut O, const refine::Segment* __restrict__ segs, uint32_t n_total, int mode,
                                                           const uint2* __restrict__ edits, const uint8_t* __restrict__ pool, uint8_t* __restrict__ bases,
                                                           uint32_t n_bases, uint8_t* __restrict__ entries) {
  refine::pick_segment(RefineRule{}, O, segs, n_total, mode, edits, pool, bases, n_bases, entries);
}

}  // namespace many
