// eg_plan_moves.h — k_plan_moves: the plan blocks of a plan-move batch (include/eirgrid_hip.h eg_evaluate_plan_moves) and of the move
// variants of a refinement launch (eg_refine_plans_moves), written on the device from a base block and an 8-byte move per variant, on
// the stream the plan launches use.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_refine_many.h; what it shares with the
// other block writers (layout, the wave's variant and base, offset tables, year masks and their store) is eg_plan_block.h's.
//
// Variant j is its base plan with ONE entry of one of the two lists taken out of its year and put back into another year (or elsewhere
// in the same one).  Both lists keep their lengths, and block j must be byte for byte what eg_plans.cpp write_lists builds for the
// moved plan in a zeroed block.  pmove's own:
//   lists    S: the flat position of the entry, D: the flat position it lands on, counted after the removal.  The bytes strictly
//            between S and D shift by one toward S, byte D takes the entry, everything outside [min(S, D), max(S, D)] is the base's.  A
//            lane writes 8-byte words: the base word, its neighbour on D's side funnel-shifted in, the two selected bytewise at the two
//            edges.  Every store instruction of the wave writes 512 consecutive bytes.  The other list is copied.
//   offsets  to_year > year: the years in (year, to_year] start one entry earlier; to_year < year: those in (to_year, year] one later.
//   masks    only the two years' can change, and the source year loses the action's bit only when no other entry of its two lists
//            carries it: the two years' lists as moved are read again (moved_entry), a year a trip.
// The base comes through a slot table as in k_plan_edits_many (slot == NULL: base block 0), so the kernel serves a refinement launch
// over many plans; there it runs BEHIND k_plan_edits_many, which has written a base copy into the blocks of the move variants, and a
// variant whose packed word does not carry kTag is not this kernel's: its block is left alone.
// No LDS, no scratch memory, nothing but vector loads and stores; the host has validated every move (eg_plan_moves_validate), the
// kernel clamps what it indexes with all the same and only ever writes inside block j.
#pragma once

namespace pmove {

using namespace pedit;      // kInsert, and eg_plan_block.h through it

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

// entry i of a flat list after the move S -> D (`src`: the base list, `entry` = src[S]; 0 <= i, S, D < kBestCap)
__device__ __forceinline__ int moved_entry(const uint8_t* src, int i, int S, int D, int entry) {
  if (i == D) return entry;
  if (S < D && i >= S && i < D) return (int)src[i + 1];
  if (S > D && i > D && i <= S) return (int)src[i - 1];
  return (int)src[i];
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

__global__ void __launch_bounds__(256) k_plan_moves(const uint8_t* __restrict__ bases, uint32_t n_bases, const uint32_t* __restrict__ slot,
                                                    const uint2* __restrict__ moves, uint32_t n, uint8_t* __restrict__ pool) {
  using namespace pmove;
  const Wave w = my_variant();
  const int lane = w.lane;
  if (w.j >= n || n_bases == 0u) return;
  const uint2 word = moves[w.j];
  if ((word.x & 0xFFu) != kTag) return;      // (uniform in the wave) an edit's variant: k_plan_edits_many has written its block
  const Base b = view(base_at(bases, n_bases, slot ? slot[w.j] : 0u));
  const Move mv = unpack_move(word);
  uint8_t* blk = pool + (size_t)w.j * snap::kPlanStride;
  const int32_t* loff = mv.list ? b.doff : b.off;
  // where the entry sits and where it lands, the latter counted after the removal
  const int S = clamp_flat(loff[mv.year] + mv.pos);
  const int D = clamp_flat(loff[mv.to_year] + mv.to_pos - (mv.to_year > mv.year ? 1 : 0));
  const int entry = (int)(mv.list ? b.dact : b.act)[S];
  write_moved_list(words(blk + kOffAct), words(b.act), lane, mv.list == 0, S, D, entry);
  write_moved_list(words(blk + kOffDAct), words(b.dact), lane, mv.list == 1, S, D, entry);
  // the years in (lo, hi] of the moved list start d entries later
  const int lo = mv.year < mv.to_year ? mv.year : mv.to_year, hi = mv.year < mv.to_year ? mv.to_year : mv.year, d = mv.to_year > mv.year ? -1 : 1;
  write_offsets(blk, b, lane, mv.list, lo, hi, d);
  // masks: the two years' from their two lists as moved (a lane below 26 keeps its own year's), the others copied
  Masks keep = {0ull, 0ull};
  bool mine = false;
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    const int y = t == 0 ? mv.year : mv.to_year;
    if (t == 1 && y == mv.year) break;      // (uniform)
    // year y's stretch of the moved list: its base stretch with the starts shifted as the offsets above are
    const int s0 = range_shift(y, lo, hi, d), s1 = range_shift(y + 1, lo, hi, d);
    const Masks ym = year_masks<true>(
        b.off[y] + (mv.list == 0 ? s0 : 0), b.off[y + 1] + (mv.list == 0 ? s1 : 0), b.doff[y] + (mv.list == 1 ? s0 : 0), b.doff[y + 1] + (mv.list == 1 ? s1 : 0), lane,
        [=](int which, int i) { return which == mv.list ? moved_entry(which ? b.dact : b.act, i, S, D, entry) : (int)(which ? b.dact : b.act)[i]; });
    if (lane == y) { keep = ym; mine = true; }
  }
  write_masks(blk, b, lane, mine, keep);
}
