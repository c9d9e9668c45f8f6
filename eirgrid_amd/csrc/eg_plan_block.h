// eg_plan_block.h — what the kernels that write plan blocks share: k_plan_edits (eg_plan_edits.h), k_plan_edits_many (eg_refine_many.h),
// k_plan_moves (eg_plan_moves.h), k_plan_crosses (eg_plan_crosses.h) and k_plan_rewrites (eg_plan_rewrites.h).  Included by eg_rollout.hip (eg_rollout.o only) behind
// eg_pareto.h, ahead of eg_plan_edits.h.
//
// A plan block is what eg_plans.cpp write_lists builds in a zeroed block of snap::kPlanStride bytes: the masks of the 26 years (a plan
// list's and the deficit list's), the prefix offsets of the two lists (28 entries each, entry 27 padding), the two flat lists, zeros
// behind their ends.  A writer runs one wave per variant, four variants per workgroup of 256, and makes block j of the pool from a base
// block and 8 bytes that say what changes.  Its own header holds what is different: how the 8 bytes unpack and how a changed flat list
// is written (write_list, write_moved_list, write_crossed_list, write_window).  The rest is here:
//   shifts    bytes_at, 8 bytes of a flat list from any byte on, funnel-shifted from two aligned words (crosses, rewrites);
//   indexing  the wave's variant and lane; a variant's base block through a slot table, the slot clamped;
//   offsets   lanes 0..27 write the first list's table, 32..59 the second's: write_offset_entries, a lane an entry the caller
//             computes (crosses); write_offsets, a base's entries with the starts of a range of years of one list moved (edits: all
//             behind the edited year by the edit's delta; moves: those between the two years by one);
//   masks     year_masks reads a changed year's two stretches again, a lane an entry (a stride of 64 for the years longer than
//             that), through the caller's "entry i of list `which` as changed", and ORs across the wave; the deficit list's bits
//             enter both masks, as in write_lists.  write_masks stores a lane's own year's masks or the base's, copied.
// No LDS, no scratch memory, no barrier, no atomic; everything is __forceinline__ and folds into the kernel that calls it.  The callers'
// lambdas capture BY VALUE: with captures by reference the compiler allocates k_plan_edits' registers differently (29 scalar / 43 vector
// instead of the 31 / 42 that tests/test_refine_resources.py pins), for the same instructions but two.
#pragma once

namespace pblock {

constexpr uint32_t kOffMask = 0, kOffDMask = snap::bestd_mask - snap::best_mask, kOffOff = snap::best_off - snap::best_mask,
                   kOffDOff = snap::bestd_off - snap::best_mask, kOffAct = snap::best_actions - snap::best_mask,
                   kOffDAct = snap::bestd_actions - snap::best_mask;
constexpr int kWords = (int)(snap::kBestCap / 8);      // 8-byte words of a flat list
static_assert(kOffAct % 8 == 0 && kOffDAct % 8 == 0 && snap::kBestCap % 512 == 0 && snap::kPlanStride == kOffDAct + snap::kBestCap, "plan block layout");

// four variants per workgroup of 256, one wave each
struct Wave { int lane; uint32_t j; };
__device__ __forceinline__ Wave my_variant() { return {(int)(threadIdx.x & (kWave - 1)), blockIdx.x * 4u + (threadIdx.x >> 6)}; }

// base block `sl` of n_bases > 0
__device__ __forceinline__ const uint8_t* base_at(const uint8_t* bases, uint32_t n_bases, uint32_t sl) {
  return bases + (size_t)(sl < n_bases ? sl : n_bases - 1u) * snap::kPlanStride;
}

// the six parts of a base block
struct Base { const int32_t *off, *doff; const uint8_t *act, *dact; const unsigned long long *mask, *dmask; };
__device__ __forceinline__ Base view(const uint8_t* b) {
  return {reinterpret_cast<const int32_t*>(b + kOffOff), reinterpret_cast<const int32_t*>(b + kOffDOff), b + kOffAct, b + kOffDAct,
          reinterpret_cast<const unsigned long long*>(b + kOffMask), reinterpret_cast<const unsigned long long*>(b + kOffDMask)};
}
__device__ __forceinline__ const unsigned long long* words(const uint8_t* list) { return reinterpret_cast<const unsigned long long*>(list); }
__device__ __forceinline__ unsigned long long* words(uint8_t* list) { return reinterpret_cast<unsigned long long*>(list); }

__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, o, kWave);
  return v;
}

// a flat position, into the list
__device__ __forceinline__ int clamp_flat(int i) { return i < 0 ? 0 : (i > (int)snap::kBestCap - 1 ? (int)snap::kBestCap - 1 : i); }

// the bytes of word w in front of flat position k, as a byte mask
__device__ __forceinline__ unsigned long long bytes_before(int k, int w) {
  const int b = k - 8 * w;
  return b >= 8 ? ~0ull : (b <= 0 ? 0ull : (1ull << (8 * b)) - 1ull);
}

// a list length, into 0..kBestCap
__device__ __forceinline__ int clamp_len(int v) { return v < 0 ? 0 : (v > (int)snap::kBestCap ? (int)snap::kBestCap : v); }

// the 8 bytes of the flat list `src` from byte q on (q of either sign; bytes outside the list are zero); need == false: not loaded
__device__ __forceinline__ unsigned long long bytes_at(const unsigned long long* src, int q, bool need) {
  const int k = q >> 3, r = (q & 7) * 8;      // (an arithmetic shift: the word below a negative q)
  const unsigned long long lo = (need && k >= 0 && k < kWords) ? src[k] : 0ull;
  const unsigned long long hi = (need && r != 0 && k + 1 >= 0 && k + 1 < kWords) ? src[k + 1] : 0ull;
  return r == 0 ? lo : (lo >> r) | (hi << (64 - r));
}

// prefix offsets: lanes 0..27 the first list's, 32..59 the second's (entry 27 is padding); entry(which, l) is the lane's
template <class Entry>
__device__ __forceinline__ void write_offset_entries(uint8_t* blk, int lane, Entry entry) {
  const int l = lane & 31, which = lane >> 5;
  if (l < 28) reinterpret_cast<int32_t*>(blk + (which ? kOffDOff : kOffOff))[l] = entry(which, l);
}
// what year l's start moves by when those of the years in (lo, hi] move by d
__device__ __forceinline__ int range_shift(int l, int lo, int hi, int d) { return (l > lo && l <= hi) ? d : 0; }
// ... the base's tables, the starts of the years in (lo, hi] of list `list` moved by d
__device__ __forceinline__ void write_offsets(uint8_t* blk, const Base& b, int lane, int list, int lo, int hi, int d) {
  write_offset_entries(blk, lane, [=](int which, int l) { return (which ? b.doff : b.off)[l] + (which == list ? range_shift(l, lo, hi, d) : 0); });
}

// the two masks of a year whose stretches of the changed lists are [a0, a1) and [d0, d1): entry(which, i) is entry i of list `which`
// as changed.  The ends are clamped to the capacity, the starts to zero where kGuardStarts says so; the result is in every lane
struct Masks { unsigned long long m, dm; };
template <bool kGuardStarts, class Entry>
__device__ __forceinline__ Masks year_masks(int a0, int a1, int d0, int d1, int lane, Entry entry) {
  if (kGuardStarts) { a0 = a0 < 0 ? 0 : a0; d0 = d0 < 0 ? 0 : d0; }
  unsigned long long m = 0ull, dm = 0ull;
  for (int i = a0 + lane; i < a1 && i < (int)snap::kBestCap; i += kWave) {
    const int a = entry(0, i);
    if (a < 64) m |= 1ull << a;
  }
  for (int i = d0 + lane; i < d1 && i < (int)snap::kBestCap; i += kWave) {
    const int a = entry(1, i);
    if (a < 64) dm |= 1ull << a;
  }
  m = wave_or_u64(m | dm); dm = wave_or_u64(dm);
  return {m, dm};
}

// the masks of the 26 years, a lane a year: (m, dm) where `mine`, the base's otherwise
__device__ __forceinline__ void write_masks(uint8_t* blk, const Base& b, int lane, bool mine, Masks y) {
  if (lane < EG_YEARS) {
    reinterpret_cast<unsigned long long*>(blk + kOffMask)[lane] = mine ? y.m : b.mask[lane];
    reinterpret_cast<unsigned long long*>(blk + kOffDMask)[lane] = mine ? y.dm : b.dmask[lane];
  }
}

}  // namespace pblock
