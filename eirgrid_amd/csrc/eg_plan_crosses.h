// eg_plan_crosses.h — k_plan_crosses: the plan blocks of a plan-cross batch (include/eirgrid_hip.h eg_evaluate_plan_crosses), written on
// the device from the parents' blocks and an 8-byte cross per variant, on the stream the plan launches use.  Included by eg_rollout.hip
// (eg_rollout.o only) behind eg_plan_moves.h; what it shares with the other block writers (layout, the wave's variant, bytes_before, bytes_at,
// clamp_len, the lane mapping of the offset tables, the mask store) is eg_plan_block.h's.
//
// Variant j is parent a with BOTH lists of the years from <= y < to replaced by parent b's lists of those years, and block j must be
// byte for byte what eg_plans.cpp write_lists builds for that child in a zeroed block.  With oA, oB the parents' prefix offsets of one list:
//   lists    A[0, oA[from]), then B[oB[from], oB[to]), then A[oA[to], oA[26]), then zeros up to the capacity: three byte-unaligned
//            segments.  A lane writes 8-byte words; an output word can hold bytes of all three (a middle segment shorter than 8 bytes),
//            so a lane forms up to three candidate words — A's word in place, B's bytes at the middle segment's shift, A's bytes at the
//            tail's shift, the latter two funnel-shifted from two aligned words each — and selects among them bytewise.  A candidate
//            is loaded only by the lanes whose word holds a byte of its segment; reads outside [0, kBestCap) count as zero.  Every store
//            instruction of the wave writes 512 consecutive bytes.  The two lists have offsets of their own, so their shifts differ.
//   offsets  y <= from: oA[y]; from < y <= to: oA[from] + oB[y] - oB[from]; to < y <= 26: oA[y] plus the difference of the two windows'
//            lengths; entry 27 stays the padding zero.
//   masks    a year's two lists come from one parent, so its two masks are that parent's, copied: nothing is recomputed.
// from == to or a == b: parent a's block, copied.  No LDS, no scratch memory, nothing but vector loads and stores; the host has validated
// every cross (eg_plan_crosses_validate), the kernel clamps what it indexes with all the same and only ever writes inside block j.
#pragma once

namespace pcross {

using namespace pblock;

// what the host packs per variant (eg_plans.cpp pack_plan_cross): a | b << 8 | from_year << 16 | to_year << 24, then zero
struct Cross { uint32_t a, b; int from, to; };
__device__ __forceinline__ Cross unpack_cross(uint2 w, uint32_t n_parents) {
  Cross x;
  x.a = w.x & 0xFFu; x.b = (w.x >> 8) & 0xFFu; x.to = (int)(w.x >> 24); x.from = (int)((w.x >> 16) & 0xFFu);
  if (x.a >= n_parents) x.a = n_parents - 1u;
  if (x.b >= n_parents) x.b = n_parents - 1u;
  if (x.to > EG_YEARS) x.to = EG_YEARS;
  if (x.from > x.to) x.from = x.to;
  return x;
}

// one flat list of the child: head [0, p0) of A in place, middle [p0, p1) from B's byte p0 + sB on, tail [p1, end) from A's byte
// p1 + sA on, zeros behind; 8 bytes a lane and step
__device__ __forceinline__ void write_crossed_list(unsigned long long* dst, const unsigned long long* A, const unsigned long long* B, int lane,
                                                   int p0, int p1, int end, int sB, int sA) {
#pragma unroll
  for (int r = 0; r < kWords / kWave; ++r) {
    const int w = r * kWave + lane;
    const unsigned long long head = bytes_before(p0, w), upto_mid = bytes_before(p1, w), upto_end = bytes_before(end, w);
    const unsigned long long mid = upto_mid & ~head, tail = upto_end & ~upto_mid;
    const unsigned long long h = head != 0ull ? A[w] : 0ull;
    const unsigned long long m = bytes_at(B, 8 * w + sB, mid != 0ull);
    const unsigned long long t = bytes_at(A, 8 * w + sA, tail != 0ull);
    dst[w] = (h & head) | (m & mid) | (t & tail);
  }
}

}  // namespace pcross

__global__ void __launch_bounds__(256) k_plan_crosses(const uint8_t* __restrict__ parents, uint32_t n_parents, const uint2* __restrict__ crosses, uint32_t n,
                                                      uint8_t* __restrict__ pool) {
  using namespace pcross;
  const Wave w = my_variant();
  const int lane = w.lane;
  if (w.j >= n || n_parents == 0u) return;
  const Cross x = unpack_cross(crosses[w.j], n_parents);
  const uint8_t* pa = parents + (size_t)x.a * snap::kPlanStride;
  const uint8_t* pb = parents + (size_t)x.b * snap::kPlanStride;
  uint8_t* blk = pool + (size_t)w.j * snap::kPlanStride;
  // (a rolled loop, one list's code run twice: with both bodies in one block hipcc 7.2's register allocator crashes under the
  //  iterative-ilp scheduler this file is built with.  The parents' parts are addressed by their offsets, not through pblock::view:
  //  with two views the kernel takes 72 vector registers instead of 65)
#pragma unroll 1
  for (int which = 0; which < 2; ++which) {
    const int32_t* oA = reinterpret_cast<const int32_t*>(pa + (which ? kOffDOff : kOffOff));
    const int32_t* oB = reinterpret_cast<const int32_t*>(pb + (which ? kOffDOff : kOffOff));
    // the child's three segments: [0, p0) A's head, [p0, p1) B's window, [p1, end) A's tail
    const int p0 = clamp_len(oA[x.from]), a_to = clamp_len(oA[x.to]), b_from = clamp_len(oB[x.from]);
    const int p1 = clamp_len(p0 + clamp_len(oB[x.to]) - b_from);
    const int end = clamp_len(p1 + clamp_len(oA[EG_YEARS]) - a_to);
    write_crossed_list(words(blk + (which ? kOffDAct : kOffAct)), words(pa + (which ? kOffDAct : kOffAct)), words(pb + (which ? kOffDAct : kOffAct)), lane,
                       p0, p1, end, b_from - p0, a_to - p1);
  }
  // prefix offsets: the formula above over the two parents' tables (entry 27 is padding: parent a's zero)
  write_offset_entries(blk, lane, [=](int which, int l) {
    const int32_t* oA = reinterpret_cast<const int32_t*>(pa + (which ? kOffDOff : kOffOff));
    const int32_t* oB = reinterpret_cast<const int32_t*>(pb + (which ? kOffDOff : kOffOff));
    uint32_t v = (uint32_t)oA[l];      // (unsigned: whatever the blocks hold, the sums wrap)
    if (l > x.from && l <= x.to) v = (uint32_t)oA[x.from] + (uint32_t)oB[l] - (uint32_t)oB[x.from];
    else if (l > x.to && l <= EG_YEARS) v += ((uint32_t)oB[x.to] - (uint32_t)oB[x.from]) - ((uint32_t)oA[x.to] - (uint32_t)oA[x.from]);
    return (int32_t)v;
  });
  // masks: year y's two are those of the parent its lists come from
  write_masks(blk, view((lane >= x.from && lane < x.to) ? pb : pa), lane, false, {0ull, 0ull});
}
