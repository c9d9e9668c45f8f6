// eg_explore.h — k_explore_turnover: what turns the members that ENTERED the archive in a generation of a Pareto local search into the
// next generation's frontier without a trip through the host (include/eirgrid_hip.h eg_explore_plans; the loop is csrc/eg_explore.cpp).
// Included by eg_rollout.hip (eg_rollout.o only) behind eg_breed.h, whose buffer (eg_internal.h breed_at), k_breed_gather,
// breed::copy_block, readback row (breed::write_row) and tail (breed::last_to_finish) it shares.
//
// The archive of an exploration lives across generations: a member whose neighbourhood has been evaluated is never enumerated again, so
// after a generation only the entries that entered in it — index >= m_first, the number of the generation's first neighbour; indices
// only grow — become bases.  k_breed_gather has kept every new entry's block beside its record slot, chunk by chunk.
//   k_explore_turnover  once per generation, behind the last gather: entry r of the archive (they stand in ascending index) is NEW when
//                       its index is >= m_first; its POSITION is the number of new entries among r' < r, which every wave counts
//                       itself over the at most EG_PARETO_MAX entries with four ballots — no atomics for the position, no LDS.  A new
//                       entry's block is copied from its block slot to that position of the OTHER frontier array (k_plan_edits_many
//                       and k_plan_moves read this generation's bases from the one, and the gathers are done), and readback row
//                       `position` written: the entry (index = number, metrics, score, slot) and the block's two prefix-offset tables,
//                       from which the host enumerates and routes the next generation.  Workgroup 0 writes the header.  The archive
//                       state is left alone; the last workgroup to finish empties the counters, as k_breed_turnover does.
// ORDER is eg_breed.h's: the whole generation is one in-order queue on the null stream.
// A wave per entry; vector loads and stores only, 16 bytes a lane; no LDS.  Every index read from memory is clamped (a position is a
// count of at most r entries), and a workgroup writes only inside its own frontier position and readback row.
#pragma once

static_assert(sizeof(ExploreHeader) == kBreedHeaderBytes && EG_PARETO_MAX % kWave == 0, "explore readback layout");

// EG_PARETO_MAX workgroups of one wave: workgroup r looks at entry r
__global__ void __launch_bounds__(kWave) k_explore_turnover(const ParetoState* st, const uint8_t* __restrict__ blocks, uint8_t* __restrict__ next_frontier,
                                                            uint8_t* __restrict__ readback, BreedCounters* cnt, long long m_first) {
  const int lane = threadIdx.x & (kWave - 1), r = (int)blockIdx.x;
  const int held = pareto::clampi(st->n_held, 0, EG_PARETO_MAX);
  int before = 0, n_new = 0;
  bool mine = false;
  for (int i = 0; i < EG_PARETO_MAX; i += kWave) {
    const int q = i + lane;
    const unsigned long long b = __ballot(q < held && st->e[q].index >= m_first);
    n_new += __popcll(b);
    if (r >= i + kWave) before += __popcll(b);
    else if (r >= i) {
      before += __popcll(b & ((1ull << (r - i)) - 1ull));
      mine = (b >> (r - i) & 1ull) != 0ull;
    }
  }
  if (mine && r < held && before < EG_PARETO_MAX) {
    const int slot = pareto::clampi(st->e[r].slot, 0, EG_PARETO_MAX - 1);
    const uint8_t* src = blocks + (size_t)slot * snap::kPlanStride;
    breed::copy_block(next_frontier + (size_t)before * snap::kPlanStride, src, lane);
    breed::write_row(readback + kBreedHeaderBytes + (size_t)before * kBreedRowBytes, &st->e[r], src, lane);
  }
  if (r == 0 && lane == 0) {
    ExploreHeader h;
    h.n_held = held; h.n_new = n_new; h.n_dropped = st->n_dropped; h.n_valid = (long long)cnt->n_valid; h.pad = 0;
    *reinterpret_cast<ExploreHeader*>(readback) = h;
  }
  // the counters, for the next generation.  The state stays: the archive lives on
  if (breed::last_to_finish(cnt, lane) && lane == 0) { cnt->n_valid = 0ull; cnt->done = 0u; }
}
