// eg_plan_edits.h — k_plan_edits: the plan blocks of a plan-edit batch (include/eirgrid_hip.h eg_evaluate_plan_edits), written on the
// device from ONE base block and an 8-byte edit per variant, on the stream the plan launches use (the rollout grids follow it without a
// host synchronisation).  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_block.h, which holds what the kernel shares
// with the other block writers: the block layout, the wave's variant, the offset tables, the year masks and their store.
//
// Variant j is the base plan with edit j applied — delete, replace or insert ONE entry of one year's list of one of the two lists — and
// its block must be byte for byte what eg_plans.cpp write_lists builds for the edited plan in a zeroed block.  pedit's own:
//   lists    the edited list is the base list with the tail behind the edit point shifted by one byte.  A lane writes 8-byte words: the
//            base word, the word before it (insert) or behind it (delete) funnel-shifted in, the two selected bytewise at the edit
//            point.  Every store instruction of the wave writes 512 consecutive bytes; the base block (8.8 KB, read by every wave of
//            the grid) stays in cache.  The other list is copied.
//   offsets  entries behind the edited year move by one.
//   masks    only the edited year's can change, and a delete needs to know whether the action still occurs: that year's two edited
//            lists are read again (edited_entry).
// write_edited_block is the whole block from a base and an edit: k_plan_edits here and many::k_plan_edits_many (eg_refine_many.h) are
// thin kernels around it.  No LDS, no scratch memory, nothing but vector loads and stores; the host has validated every edit
// (eg_plan_edits_validate), the kernel clamps what it indexes with all the same and only ever writes inside block j.
#pragma once

namespace pedit {

using namespace pblock;

constexpr int kNone = 0, kDelete = 1, kReplace = 2, kInsert = 3;
// what the host packs per variant (eg_plans.cpp pack_edit): kind | list << 8 | year << 16 | action << 24, then pos
struct Edit { int kind, list, year, action, pos; };
__device__ __forceinline__ Edit unpack(uint2 w) {
  Edit e;
  e.kind = (int)(w.x & 0xFFu); e.list = (int)((w.x >> 8) & 1u); e.year = (int)((w.x >> 16) & 0xFFu); e.action = (int)(w.x >> 24);
  e.pos = (int)w.y;
  if (e.year >= EG_YEARS) e.year = EG_YEARS - 1;
  if (e.kind > kInsert) e.kind = kNone;
  return e;
}

// entry i of a flat list after the edit at flat position P (`src`: the base list; entries behind its capacity read as zero)
__device__ __forceinline__ int edited_entry(const uint8_t* src, int i, int kind, int P, int action) {
  if (kind == kInsert) return i == P ? action : (int)src[i > P ? i - 1 : i];
  if (kind == kDelete) { const int k = i >= P ? i + 1 : i; return k < (int)snap::kBestCap ? (int)src[k] : 0; }
  return (kind == kReplace && i == P) ? action : (int)src[i];
}

// the flat list `src` to `dst` with the edit applied (kNone: a copy), 8 bytes a lane and step
__device__ __forceinline__ void write_list(unsigned long long* dst, const unsigned long long* src, int lane, int kind, int P, int action) {
#pragma unroll
  for (int r = 0; r < kWords / kWave; ++r) {
    const int w = r * kWave + lane;
    const unsigned long long a = src[w];
    unsigned long long out = a;
    if (kind != kNone) {      // (uniform in the wave)
      unsigned long long moved = a;
      if (kind == kInsert) moved = (a << 8) | ((w > 0 ? src[w - 1] : 0ull) >> 56);
      if (kind == kDelete) moved = (a >> 8) | ((w + 1 < kWords ? src[w + 1] : 0ull) << 56);
      const int k = P - 8 * w;
      const unsigned long long keep = bytes_before(P, w);      // the bytes of this word in front of the edit point
      out = (a & keep) | (moved & ~keep);
      if (kind != kDelete && k >= 0 && k < 8) out = (out & ~(0xFFull << (8 * k))) | ((unsigned long long)action << (8 * k));
    }
    dst[w] = out;
  }
}

// block `blk` from the block `base` and the edit e; kGuardStarts: the mask stretch's starts are clamped as well
template <bool kGuardStarts>
__device__ __forceinline__ void write_edited_block(const uint8_t* __restrict__ base, const Edit e, uint8_t* __restrict__ blk, int lane) {
  const Base b = view(base);
  // the edit point in the flat list, and what the edit does to the length of the list
  const int P = clamp_flat((e.list ? b.doff : b.off)[e.year] + e.pos);
  const int delta = e.kind == kInsert ? 1 : (e.kind == kDelete ? -1 : 0);
  const int k0 = e.list == 0 ? e.kind : kNone, k1 = e.list == 1 ? e.kind : kNone;
  write_list(words(blk + kOffAct), words(b.act), lane, k0, P, e.action);
  write_list(words(blk + kOffDAct), words(b.dact), lane, k1, P, e.action);
  write_offsets(blk, b, lane, e.list, e.year, EG_YEARS, delta);
  // masks: the edited year's from its two lists as edited, the others copied
  Masks y = {0ull, 0ull};
  if (e.kind != kNone)
    y = year_masks<kGuardStarts>(b.off[e.year], b.off[e.year + 1] + (e.list == 0 ? delta : 0), b.doff[e.year], b.doff[e.year + 1] + (e.list == 1 ? delta : 0), lane,
                                 [=](int which, int i) { return which ? edited_entry(b.dact, i, k1, P, e.action) : edited_entry(b.act, i, k0, P, e.action); });
  write_masks(blk, b, lane, e.kind != kNone && lane == e.year, y);
}

}  // namespace pedit

__global__ void __launch_bounds__(256) k_plan_edits(const uint8_t* __restrict__ base, const uint2* __restrict__ edits, uint32_t n, uint8_t* __restrict__ pool) {
  const pblock::Wave w = pblock::my_variant();
  if (w.j >= n) return;
  pedit::write_edited_block<false>(base, pedit::unpack(edits[w.j]), pool + (size_t)w.j * snap::kPlanStride, w.lane);
}
