// eg_refine_many.h — k_plan_edits_many and k_refine_pick_many: a refinement round in one launch, of one plan (include/eirgrid_hip.h
// eg_refine_plan) or of many (eg_refine_plans); the host loop of both is eg_refine.cpp.  Included by eg_rollout.hip (eg_rollout.o only)
// behind eg_refine.h.
//
// A launch holds the variants of its plans back to back: SEGMENT s is the variants [first_s, first_s + n_s) of one plan, whose base
// block is block slot_s of a buffer of base blocks (one per plan of the call, uploaded once).
//   k_plan_edits_many   variant j's block from base block slot[j] and edit j: byte for byte what write_lists builds for the edited plan
//                       in a zeroed block; one wave per variant, 8-byte words, every store of a wave 512 consecutive bytes; no LDS, no
//                       scratch memory; writes inside block j only.  It is eg_plan_edits.h's write_edited_block, the body of k_plan_edits,
//                       with the slot indirection (eg_plan_block.h base_at) and the two start clamps that body's flag switches on.
//   k_refine_pick_many  one workgroup per segment, on the null stream behind the launch's rollout grids.  Workgroup s
//     reads    status and metrics of ITS variants straight from the records (32 + 4 bytes of each 12 KB record), a thread a variant,
//              striding by the workgroup's width when there are more variants than threads — the trip count is the same for every
//              thread; no record outside its segment;
//     reduces  (score, index relative to the segment) per wave and across the sixteen waves (eg_refine.h): the largest score wins, ties
//              to the lowest variant; a candidate that scores -inf is recorded as well, and a candidate base — the segment's first
//              variant — is itself in the running, so there is a winner (the clamp is for a record that lies about it);
//     counts   its variants that are no candidates, a ballot per trip;
//     writes   entry s of the launch's entries (RefineEntry, eg_internal.h): winner, its packed edit, score, metrics, the count, the
//              list totals of the winner's block, and what the base scored;
//     copies   the winner's plan block over base block slot_s when the winner is not the segment's variant 0 — 552 16-byte vector
//              stores, one per thread — so that the next round's k_plan_edits_many finds the plan's base where the host uploaded it.
// Every index read from memory or computed from one is clamped.
// The two kernels live in a namespace of their own, `many`: scripts/kernel_resources.sh prints a kernel by what is left of its mangled
// name, and the test that pins k_plan_edits' resource line picks it by the word k_plan_edits at the start of that name.  Behind the
// namespace the names print as many17k_plan_edits_many / many18k_refine_pick_many, which such a pattern does not take for it
// (tests/test_refine_many_resources.py looks for the full names).
#pragma once

namespace refine {

// what the host uploads per segment of a launch
struct Segment { uint32_t first, count, slot, pad; };
static_assert(sizeof(Segment) == 16, "segment table entry");

}  // namespace refine

namespace many {

__global__ void __launch_bounds__(256) k_plan_edits_many(const uint8_t* __restrict__ bases, uint32_t n_bases, const uint32_t* __restrict__ slot,
                                                         const uint2* __restrict__ edits, uint32_t n, uint8_t* __restrict__ pool) {
  const pblock::Wave w = pblock::my_variant();
  if (w.j >= n || n_bases == 0u) return;
  pedit::write_edited_block<true>(pblock::base_at(bases, n_bases, slot[w.j]), pedit::unpack(edits[w.j]), pool + (size_t)w.j * snap::kPlanStride, w.lane);
}

// workgroup s: segment s of the launch's n_total variants
__global__ void __launch_bounds__(1024) k_refine_pick_many(DevOut O, const refine::Segment* __restrict__ segs, uint32_t n_total, int mode,
                                                           const uint2* __restrict__ edits, const uint8_t* __restrict__ pool, uint8_t* __restrict__ bases,
                                                           uint32_t n_bases, uint8_t* __restrict__ entries) {
  using namespace refine;
  __shared__ double s_score[kWaves];
  __shared__ int s_index[kWaves], s_fail[kWaves];
  __shared__ int s_base_ok;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const Segment sg = segs[blockIdx.x];
  RefineEntry* entry = reinterpret_cast<RefineEntry*>(entries + (size_t)blockIdx.x * kRefineEntryStride);
  // the segment inside the launch (uniform in the workgroup)
  const uint32_t first = sg.first < n_total ? sg.first : n_total;
  const uint32_t n = sg.count < n_total - first ? sg.count : n_total - first;
  if (n == 0u || n_bases == 0u) {      // (no host launch describes one: an entry that says so, nothing copied)
    if (tid == 0) { entry->winner = -1; entry->n_failed = 0; entry->base_ok = 0; entry->n = 0; }
    return;
  }
  uint8_t* base = bases + (size_t)(sg.slot < n_bases ? sg.slot : n_bases - 1u) * snap::kPlanStride;
  double best = -__builtin_huge_val();
  int best_j = kNoIndex, fails = 0;      // (variant indices relative to the segment)
  for (uint32_t j0 = 0; j0 < n; j0 += (uint32_t)kThreads) {      // (uniform: the ballot below wants every lane)
    const uint32_t j = j0 + (uint32_t)tid;
    bool cand = false;
    double s = 0.0;
    if (j < n) {
      const double* m = O.metrics(first + j);
      const double mm[4] = {m[0], m[1], m[2], m[3]};
      s = rm::rank_score(mm, mode);
      cand = *O.status(first + j) == EG_EP_OK && s == s;
      if (j == 0u) {      // what the segment's base scores
        s_base_ok = cand ? 1 : 0;
        entry->base_ok = cand ? 1 : 0; entry->base_score = s;
#pragma unroll
        for (int k = 0; k < 4; ++k) entry->base_metrics[k] = mm[k];
      }
    }
    fails += __popcll(__ballot(j < n && !cand));
    if (cand && before(s, (int)j, best, best_j)) { best = s; best_j = (int)j; }
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
  const int winner = base_ok ? (best_j < 0 ? 0 : (best_j >= (int)n ? (int)n - 1 : best_j)) : -1;
  const uint32_t w = first + (winner < 0 ? 0u : (uint32_t)winner);      // the winner among the launch's variants
  const uint8_t* blk = pool + (size_t)w * snap::kPlanStride;
  if (tid == 0) {
    const uint2 e = edits[w];
    const double* m = O.metrics(w);
    entry->winner = winner; entry->n_failed = fails;
    entry->edit[0] = e.x; entry->edit[1] = e.y;
    entry->score = base_ok ? best : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) entry->metrics[k] = m[k];
    entry->off26 = reinterpret_cast<const int32_t*>(blk + pblock::kOffOff)[EG_YEARS];
    entry->offd26 = reinterpret_cast<const int32_t*>(blk + pblock::kOffDOff)[EG_YEARS];
    entry->n = (int32_t)n;
  }
  if (winner > 0 && tid < (int)(snap::kPlanStride / 16)) reinterpret_cast<uint4*>(base)[tid] = reinterpret_cast<const uint4*>(blk)[tid];
}

}  // namespace many
