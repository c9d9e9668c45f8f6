// eg_plan_moves.h — k_plan_moves: the plan blocks of a plan-move batch (include/eirgrid_hip.h eg_evaluate_plan_moves) and of the move
// variants of a refinement launch (eg_refine_plans_moves), written on the device from a base block and an 8-byte move per variant, on
// the stream the plan launches use.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_refine_many.h.
//
// Variant j is its base plan with ONE entry of one of the two lists taken out of its year and put back into another year (or elsewhere
// in the same one).  Both lists keep their lengths, and block j must be byte for byte what eg_plans.cpp write_lists builds for the
// moved plan in a zeroed block:
//   lists    S: the flat position of the entry, D: the flat position it lands on, counted after the removal.  The bytes strictly
//            between S and D shift by one toward S, byte D takes the entry, everything outside [min(S, D), max(S, D)] is the base's.  A
//            lane writes 8-byte words: the base word, its neighbour on D's side funnel-shifted in, the two selected bytewise at the two
//            edges.  Every store instruction of the wave writes 512 consecutive bytes.  The other list is copied.
//   offsets  to_year > year: the years in (year, to_year] start one entry earlier; to_year < year: those in (to_year, year] one later.
//   masks    only the two years' can change, and the source year loses the action's bit only when no other entry of its two lists
//            carries it: the two years' lists as moved are read again, a lane an entry (a stride of 64 for the years longer than
//            that), and OR-ed across the wave; the deficit list's bits enter both masks, as in write_lists.
// The base comes through a slot table as in k_plan_edits_many (slot == NULL: base block 0), so the kernel serves a refinement launch
// over many plans; there it runs BEHIND k_plan_edits_many, which has written a base copy into the blocks of the move variants, and a
// variant whose packed word does not carry kTag is not this kernel's: its block is left alone.
// No LDS, no scratch memory, nothing but vector loads and stores; the host has validated every move (eg_plan_moves_validate), the
// kernel clamps what it indexes with all the same and only ever writes inside block j.
#pragma once

namespace pmove {

using namespace pedit;      // the block layout (kOff*, kWords) and wave_or_u64

// what the host packs per variant (eg_plans.cpp pack_plan_move): kTag | list << 8 | year << 16 | to_year << 24, then pos | to_pos << 16.
// kTag sits where an edit has its kind and is no kind: pedit::unpack reads such a variant as "none".
constexpr uint32_t kTag = kPlanMoveTag;
static_assert(kTag > (uint32_t)kInsert && kTag < 256u, "the tag is no edit kind");
struct Move { int list, year, to_year, pos, to_pos; };
__device__ __forceinline__ Move unpack_move(uint2 w) {
  Move m;
  m.list = (int)((w.x >> 8) & 1u); m.year = (int)((w.x >> 16) & 0xFFu); m.to_year = (int)(w.x >> 24);
  m.pos = (int)(w.y & 0xFFFFu); m.to_pos = (int)(w.y >> 16);
  if (m.year >= EG_YEARS) m.year = EG_YEARS - 1;
  if (m.to_year >= EG_YEARS) m.to_year = EG_YEARS - 1;
  return m;
}
__device__ __forceinline__ int clamp_flat(int i) { return i < 0 ? 0 : (i > (int)snap::kBestCap - 1 ? (int)snap::kBestCap - 1 : i); }

// entry i of a flat list after the move S -> D (`src`: the base list, `entry` = src[S]; 0 <= i, S, D < kBestCap)
__device__ __forceinline__ int moved_entry(const uint8_t* src, int i, int S, int D, int entry) {
  if (i == D) return entry;
  if (S < D && i >= S && i < D) return (int)src[i + 1];
  if (S > D && i > D && i <= S) return (int)src[i - 1];
  return (int)src[i];
}

// the bytes of word w in front of flat position k, as a byte mask
__device__ __forceinline__ unsigned long long bytes_before(int k, int w) {
  const int b = k - 8 * w;
  return b >= 8 ? ~0ull : (b <= 0 ? 0ull : (1ull << (8 * b)) - 1ull);
}

// the flat list `src` to `dst` with the move S -> D applied (moved == false: a copy), 8 bytes a lane and step
__device__ __forceinline__ void write_moved_list(unsigned long long* dst, const unsigned long long* src, int lane, bool moved, int S, int D, int entry) {
  // the bytes that take their neighbour's value: [S, D) from behind, or (D, S] from in front
  const int lo = S < D ? S : D + 1, hi = S < D ? D : S + 1;
#pragma unroll
  for (int r = 0; r < kWords / kWave; ++r) {
    const int w = r * kWave + lane;
    const unsigned long long a = src[w];
    unsigned long long out = a;
    if (moved) {      // (uniform in the wave)
      const unsigned long long shifted = S < D ? (a >> 8) | ((w + 1 < kWords ? src[w + 1] : 0ull) << 56) : (a << 8) | ((w > 0 ? src[w - 1] : 0ull) >> 56);
      const unsigned long long take = bytes_before(hi, w) & ~bytes_before(lo, w);
      out = (a & ~take) | (shifted & take);
      const int k = D - 8 * w;
      if (k >= 0 && k < 8) out = (out & ~(0xFFull << (8 * k))) | ((unsigned long long)entry << (8 * k));
    }
    dst[w] = out;
  }
}

}  // namespace pmove

// four variants per workgroup of 256, one wave each
__global__ void __launch_bounds__(256) k_plan_moves(const uint8_t* __restrict__ bases, uint32_t n_bases, const uint32_t* __restrict__ slot,
                                                    const uint2* __restrict__ moves, uint32_t n, uint8_t* __restrict__ pool) {
  using namespace pmove;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (j >= n || n_bases == 0u) return;
  const uint2 word = moves[j];
  if ((word.x & 0xFFu) != kTag) return;      // (uniform in the wave) an edit's variant: k_plan_edits_many has written its block
  const uint32_t sl = slot ? slot[j] : 0u;
  const uint8_t* base = bases + (size_t)(sl < n_bases ? sl : n_bases - 1u) * snap::kPlanStride;
  const Move mv = unpack_move(word);
  uint8_t* blk = pool + (size_t)j * snap::kPlanStride;
  const int32_t* off = reinterpret_cast<const int32_t*>(base + kOffOff);
  const int32_t* doff = reinterpret_cast<const int32_t*>(base + kOffDOff);
  const uint8_t* act = base + kOffAct;
  const uint8_t* dact = base + kOffDAct;
  const int32_t* loff = mv.list ? doff : off;
  // where the entry sits and where it lands, the latter counted after the removal
  const int S = clamp_flat(loff[mv.year] + mv.pos);
  const int D = clamp_flat(loff[mv.to_year] + mv.to_pos - (mv.to_year > mv.year ? 1 : 0));
  const int entry = (int)(mv.list ? dact : act)[S];
  write_moved_list(reinterpret_cast<unsigned long long*>(blk + kOffAct), reinterpret_cast<const unsigned long long*>(act), lane, mv.list == 0, S, D, entry);
  write_moved_list(reinterpret_cast<unsigned long long*>(blk + kOffDAct), reinterpret_cast<const unsigned long long*>(dact), lane, mv.list == 1, S, D, entry);
  // prefix offsets: lanes 0..27 the first list's, 32..59 the second's (entry 27 is padding); what year l's start moves by
  const int l = lane & 31, which = lane >> 5;
  if (l < 28) {
    int v = (which ? doff : off)[l];
    if (which == mv.list) v += (l > mv.year && l <= mv.to_year) ? -1 : ((l > mv.to_year && l <= mv.year) ? 1 : 0);
    reinterpret_cast<int32_t*>(blk + (which ? kOffDOff : kOffOff))[l] = v;
  }
  // masks: the two years' from their two lists as moved (a lane below 26 keeps its own year's), the others copied
  unsigned long long keep_m = 0ull, keep_dm = 0ull;
  bool mine = false;
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    const int y = t == 0 ? mv.year : mv.to_year;
    if (t == 1 && y == mv.year) break;      // (uniform)
    // year y's stretch of the moved list: its base stretch with the starts shifted as the offsets above are
    const int s0 = (y > mv.year && y <= mv.to_year) ? -1 : ((y > mv.to_year && y <= mv.year) ? 1 : 0);
    const int s1 = (y + 1 > mv.year && y + 1 <= mv.to_year) ? -1 : ((y + 1 > mv.to_year && y + 1 <= mv.year) ? 1 : 0);
    int a0 = off[y] + (mv.list == 0 ? s0 : 0), d0 = doff[y] + (mv.list == 1 ? s0 : 0);
    const int a1 = off[y + 1] + (mv.list == 0 ? s1 : 0), d1 = doff[y + 1] + (mv.list == 1 ? s1 : 0);
    a0 = a0 < 0 ? 0 : a0; d0 = d0 < 0 ? 0 : d0;
    unsigned long long m = 0ull, dm = 0ull;
    for (int i = a0 + lane; i < a1 && i < (int)snap::kBestCap; i += kWave) {
      const int a = mv.list == 0 ? moved_entry(act, i, S, D, entry) : (int)act[i];
      if (a < 64) m |= 1ull << a;
    }
    for (int i = d0 + lane; i < d1 && i < (int)snap::kBestCap; i += kWave) {
      const int a = mv.list == 1 ? moved_entry(dact, i, S, D, entry) : (int)dact[i];
      if (a < 64) dm |= 1ull << a;
    }
    m = wave_or_u64(m | dm); dm = wave_or_u64(dm);
    if (lane == y) { keep_m = m; keep_dm = dm; mine = true; }
  }
  if (lane < EG_YEARS) {
    const unsigned long long* bm = reinterpret_cast<const unsigned long long*>(base + kOffMask);
    const unsigned long long* bdm = reinterpret_cast<const unsigned long long*>(base + kOffDMask);
    reinterpret_cast<unsigned long long*>(blk + kOffMask)[lane] = mine ? keep_m : bm[lane];
    reinterpret_cast<unsigned long long*>(blk + kOffDMask)[lane] = mine ? keep_dm : bdm[lane];
  }
}
