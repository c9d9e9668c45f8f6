// eg_plan_edits.h — k_plan_edits: the plan blocks of a plan-edit batch (include/eirgrid_hip.h eg_evaluate_plan_edits), written on the
// device from ONE base block and an 8-byte edit per variant, on the stream the plan launches use (the rollout grids follow it without a
// host synchronisation).  Included by eg_rollout.hip (eg_rollout.o only) behind eg_topk.h.
//
// Variant j is the base plan with edit j applied — delete, replace or insert ONE entry of one year's list of one of the two lists — and
// its block must be byte for byte what eg_plans.cpp write_lists builds for the edited plan in a zeroed block (snap::kPlanStride bytes:
// the masks of the 26 years, the prefix offsets of the two lists, the two flat lists, zeros behind their ends):
//   lists    the edited list is the base list with the tail behind the edit point shifted by one byte.  A lane writes 8-byte words: the
//            base word, the word before it (insert) or behind it (delete) funnel-shifted in, the two selected bytewise at the edit
//            point.  Every store instruction of the wave writes 512 consecutive bytes; the base block (8.8 KB, read by every wave of
//            the grid) stays in cache.  The other list is copied.
//   offsets  entries behind the edited year move by one.
//   masks    only the edited year's can change, and a delete needs to know whether the action still occurs: that year's two edited
//            lists are read again, a lane an entry (a stride of 64 for the years longer than that), and OR-ed across the wave.
// No LDS, no scratch memory, nothing but vector loads and stores; the host has validated every edit (eg_plan_edits_validate), the
// kernel clamps what it indexes with all the same and only ever writes inside block j.
#pragma once

namespace pedit {

constexpr int kNone = 0, kDelete = 1, kReplace = 2, kInsert = 3;
constexpr uint32_t kOffMask = 0, kOffDMask = snap::bestd_mask - snap::best_mask, kOffOff = snap::best_off - snap::best_mask,
                   kOffDOff = snap::bestd_off - snap::best_mask, kOffAct = snap::best_actions - snap::best_mask,
                   kOffDAct = snap::bestd_actions - snap::best_mask;
constexpr int kWords = (int)(snap::kBestCap / 8);      // 8-byte words of a flat list
static_assert(kOffAct % 8 == 0 && kOffDAct % 8 == 0 && snap::kBestCap % 512 == 0 && snap::kPlanStride == kOffDAct + snap::kBestCap, "plan block layout");

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

__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, o, kWave);
  return v;
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
      const int k = P - 8 * w;      // bytes of this word in front of the edit point
      const unsigned long long keep = k >= 8 ? ~0ull : (k <= 0 ? 0ull : (1ull << (8 * k)) - 1ull);
      out = (a & keep) | (moved & ~keep);
      if (kind != kDelete && k >= 0 && k < 8) out = (out & ~(0xFFull << (8 * k))) | ((unsigned long long)action << (8 * k));
    }
    dst[w] = out;
  }
}

}  // namespace pedit

// four variants per workgroup of 256, one wave each
__global__ void __launch_bounds__(256) k_plan_edits(const uint8_t* __restrict__ base, const uint2* __restrict__ edits, uint32_t n, uint8_t* __restrict__ pool) {
  using namespace pedit;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (j >= n) return;
  const Edit e = unpack(edits[j]);
  uint8_t* blk = pool + (size_t)j * snap::kPlanStride;
  const int32_t* off = reinterpret_cast<const int32_t*>(base + kOffOff);
  const int32_t* doff = reinterpret_cast<const int32_t*>(base + kOffDOff);
  const uint8_t* act = base + kOffAct;
  const uint8_t* dact = base + kOffDAct;
  // the edit point in the flat list, and what the edit does to the length of the list
  int P = (e.list ? doff : off)[e.year] + e.pos;
  P = P < 0 ? 0 : (P > (int)snap::kBestCap - 1 ? (int)snap::kBestCap - 1 : P);
  const int delta = e.kind == kInsert ? 1 : (e.kind == kDelete ? -1 : 0);
  const int k0 = e.list == 0 ? e.kind : kNone, k1 = e.list == 1 ? e.kind : kNone;
  write_list(reinterpret_cast<unsigned long long*>(blk + kOffAct), reinterpret_cast<const unsigned long long*>(act), lane, k0, P, e.action);
  write_list(reinterpret_cast<unsigned long long*>(blk + kOffDAct), reinterpret_cast<const unsigned long long*>(dact), lane, k1, P, e.action);
  // prefix offsets: lanes 0..27 the first list's, 32..59 the second's (entry 27 is padding)
  {
    const int l = lane & 31, which = lane >> 5;
    if (l < 28) {
      int v = (which ? doff : off)[l];
      if (which == e.list && l > e.year && l <= EG_YEARS) v += delta;
      reinterpret_cast<int32_t*>(blk + (which ? kOffDOff : kOffOff))[l] = v;
    }
  }
  // masks: the edited year's from its two lists as edited, the others copied
  unsigned long long m = 0ull, dm = 0ull;
  if (e.kind != kNone) {
    const int a0 = off[e.year], a1 = off[e.year + 1] + (e.list == 0 ? delta : 0);
    const int d0 = doff[e.year], d1 = doff[e.year + 1] + (e.list == 1 ? delta : 0);
    for (int i = a0 + lane; i < a1 && i < (int)snap::kBestCap; i += kWave) {
      const int a = edited_entry(act, i, k0, P, e.action);
      if (a < 64) m |= 1ull << a;
    }
    for (int i = d0 + lane; i < d1 && i < (int)snap::kBestCap; i += kWave) {
      const int a = edited_entry(dact, i, k1, P, e.action);
      if (a < 64) dm |= 1ull << a;
    }
    m = wave_or_u64(m | dm); dm = wave_or_u64(dm);
  }
  if (lane < EG_YEARS) {
    const unsigned long long* bm = reinterpret_cast<const unsigned long long*>(base + kOffMask);
    const unsigned long long* bdm = reinterpret_cast<const unsigned long long*>(base + kOffDMask);
    const bool mine = e.kind != kNone && lane == e.year;
    reinterpret_cast<unsigned long long*>(blk + kOffMask)[lane] = mine ? m : bm[lane];
    reinterpret_cast<unsigned long long*>(blk + kOffDMask)[lane] = mine ? dm : bdm[lane];
  }
}
