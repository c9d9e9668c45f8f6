// eg_plan_rewrites.h — k_plan_rewrites: the plan blocks of a plan-rewrite batch (include/eirgrid_hip.h eg_evaluate_plan_rewrites), written on
// the device from the plans' blocks, the action maps (64 bytes each) and an 8-byte rewrite per variant, on the stream the plan launches
// use.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_crosses.h; what it shares with the other block writers (layout, the
// wave's variant, bytes_before, bytes_at, the lane mapping of the offset tables, year_masks, the mask store) is eg_plan_block.h's.
//
// Variant j is plan `plan` with every entry e of the years from <= y < to of the selected lists replaced by to[e], or taken out where
// to[e] is the drop value, and block j must be byte for byte what eg_plans.cpp write_lists builds for that child in a zeroed block.  It is
// the first writer whose output length depends on the entries' VALUES.  With o the plan's prefix offsets of one selected list, s0 =
// o[from], s1 = o[to], K the entries of the window that are kept and D = s1 - s0 - K those dropped:
//   lists    head [0, s0) in place; window [s0, s0 + K), the source stretch [s0, s1) mapped and compacted; tail [s0 + K, o[26] - D) from
//            source byte s1 on; zeros up to the capacity.
//            The window is a stream compaction: per step a lane takes the 8-byte word k of the source (512 bytes a wave), looks every byte
//            up in the map — lane l holds to[l], so a look-up is a wave shuffle; every lane runs every step — packs the bytes it keeps, and
//            an inclusive wave scan of the kept counts plus the steps' running base gives the lane its destination.  It stores its kept
//            bytes ONE BY ONE: they start at any byte and a word store would cover bytes that belong to other lanes.
//            Head, tail and zeros are written as in k_plan_crosses, 8-byte words with the tail funnel-shifted (bytes_at) — but ONLY the
//            words that hold no byte of the window.  The words in between are all window, but for the first and the last of them: their
//            bytes outside the window are stored one by one as well, by the lanes 0..7 (the first word) and 8..15 (the last).
//            ONE STORE PER BYTE: every byte of block j is stored by exactly one store instruction of one lane.  Two stores to one byte from
//            different lanes or instructions land in an order nobody controls; a word over a boundary would race the window's bytes.
//   offsets  y <= from: o[y]; from < y <= to: s0 + the kept entries of [s0, o[y]) — taken in the step that holds source byte o[y], from the
//            scan and the kept bits of the lane that holds it, by two shuffles; behind the last step it is K —; y > to: o[y] - D.
//   masks    a year of the window: its two source stretches mapped again through year_masks (the map read from memory there: the stretch
//            loop diverges, and a shuffle reads no inactive lane); a dropped entry is 0xFF and falls out of year_masks' a < 64.  A year
//            outside the window keeps the plan's.
// Nothing the kernel wrote is read back.  A list that is not selected, lists == 0 or from == to: an empty window, and the plan's block
// copied.  No LDS, no scratch memory, no atomic, nothing but vector loads and stores; the host has validated every rewrite and map
// (eg_plan_rewrites_validate), the kernel clamps what it indexes with all the same and only ever writes inside block j: a window byte
// goes to s0 + (kept bytes in front of it) < s1 <= kBestCap.
#pragma once

namespace prewrite {

using namespace pblock;

constexpr uint32_t kDrop = 0xFFu;      // EG_REWRITE_DROP
constexpr uint32_t kMapStride = 64;    // a map on the device: to[0..60], then three drop bytes

// what the host packs per variant (eg_plans.cpp pack_plan_rewrite): plan | map << 16, then from_year | to_year << 8 | lists << 16
struct Rewrite { uint32_t plan, map; int from, to, lists; };
__device__ __forceinline__ Rewrite unpack_rewrite(uint2 w, uint32_t n_plans, uint32_t n_maps) {
  Rewrite x;
  x.plan = w.x & 0xFFFFu; x.map = w.x >> 16; x.from = (int)(w.y & 0xFFu); x.to = (int)((w.y >> 8) & 0xFFu); x.lists = (int)((w.y >> 16) & 3u);
  if (x.plan >= n_plans) x.plan = n_plans - 1u;
  if (x.map >= n_maps) x.map = n_maps - 1u;
  if (x.to > EG_YEARS) x.to = EG_YEARS;
  if (x.from > x.to) x.from = x.to;
  return x;
}

// the inclusive prefix sums of v over the wave
__device__ __forceinline__ int wave_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

// The window [s0, s1) of the flat list `src`, mapped and compacted, to dst + s0 on (mapv: the lane's map entry).  Returns K, the bytes
// kept; *before: the kept bytes in front of source byte q (s0 <= q <= s1), -1 where no step held q (then it is K)
__device__ __forceinline__ int write_window(uint8_t* dst, const unsigned long long* src, int lane, int s0, int s1, uint32_t mapv, int q, int* before) {
  const int k0 = s0 >> 3;
  const int steps = s1 > s0 ? (s1 - 8 * k0 + 511) >> 9 : 0;
  int run = 0, seen = -1;
  for (int r = 0; r < steps; ++r) {
    const int k = k0 + r * kWave + lane;
    const unsigned long long v = k < kWords ? src[k] : 0ull;
    unsigned long long kept = 0ull;
    uint32_t bits = 0u;
    int c = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint32_t e = (uint32_t)(v >> (8 * b)) & 0xFFu;
      const uint32_t t = (uint32_t)__shfl((int)mapv, (int)(e & 63u), kWave);
      const int pos = 8 * k + b;
      if (pos >= s0 && pos < s1 && e < 64u && t != kDrop) { kept |= (unsigned long long)t << (8 * c); bits |= 1u << b; ++c; }
    }
    const int incl = wave_scan(c, lane), excl = incl - c;
    // the kept bytes in front of q, where this step holds it
    const int rel = q - (8 * k0 + r * 512);
    const int owner_excl = __shfl(excl, (rel >> 3) & (kWave - 1), kWave);
    const uint32_t owner_bits = (uint32_t)__shfl((int)bits, (rel >> 3) & (kWave - 1), kWave);
    if (rel >= 0 && rel < 512) seen = run + owner_excl + __popc(owner_bits & ((1u << (rel & 7)) - 1u));
    uint8_t* d = dst + s0 + run + excl;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < c) d[i] = (uint8_t)(kept >> (8 * i));
    run += __shfl(incl, kWave - 1, kWave);
  }
  *before = seen;
  return run;
}

// what is not window of one flat list of the child: head [0, s0) in place, tail [p1, end) from the source's byte p1 + D on, zeros behind;
// the window is [s0, p1).  8 bytes a lane and step for the words without a window byte; single bytes in the window's first and last word
__device__ __forceinline__ void write_around_window(uint8_t* dst, const uint8_t* src, int lane, int s0, int p1, int end, int D) {
  const unsigned long long* A = words(src);
#pragma unroll
  for (int r = 0; r < kWords / kWave; ++r) {
    const int w = r * kWave + lane;
    const unsigned long long head = bytes_before(s0, w), upto_win = bytes_before(p1, w), upto_end = bytes_before(end, w);
    const unsigned long long win = upto_win & ~head, tail = upto_end & ~upto_win;
    const unsigned long long h = head != 0ull ? A[w] : 0ull;
    const unsigned long long t = bytes_at(A, 8 * w + D, tail != 0ull);
    if (win == 0ull) words(dst)[w] = (h & head) | (t & tail);
  }
  if (p1 > s0 && lane < 16) {
    const int first = s0 >> 3, last = (p1 - 1) >> 3;
    const int pos = 8 * (lane < 8 ? first : last) + (lane & 7);
    if ((lane < 8 || last != first) && (pos < s0 || pos >= p1) && pos < (int)snap::kBestCap) {
      int v = 0;
      if (pos < s0) v = src[pos];
      else if (pos < end) v = src[clamp_flat(pos + D)];
      dst[pos] = (uint8_t)v;
    }
  }
}

}  // namespace prewrite

__global__ void __launch_bounds__(256) k_plan_rewrites(const uint8_t* __restrict__ plans, uint32_t n_plans, const uint8_t* __restrict__ maps, uint32_t n_maps,
                                                       const uint2* __restrict__ rewrites, uint32_t n, uint8_t* __restrict__ pool) {
  using namespace prewrite;
  const Wave w = my_variant();
  const int lane = w.lane;
  if (w.j >= n || n_plans == 0u || n_maps == 0u) return;
  const Rewrite x = unpack_rewrite(rewrites[w.j], n_plans, n_maps);
  const uint8_t* pa = plans + (size_t)x.plan * snap::kPlanStride;
  const uint8_t* mp = maps + (size_t)x.map * kMapStride;
  uint8_t* blk = pool + (size_t)w.j * snap::kPlanStride;
  const uint32_t mapv = mp[lane];      // lane l holds to[l]
  const int l = lane & 31;             // the offset entry this lane writes, of list lane >> 5 (eg_plan_block.h write_offset_entries)
  int32_t my_off = 0;
#pragma unroll 1
  for (int which = 0; which < 2; ++which) {
    const int32_t* o = reinterpret_cast<const int32_t*>(pa + (which ? kOffDOff : kOffOff));
    const uint8_t* src = pa + (which ? kOffDAct : kOffAct);
    uint8_t* dst = blk + (which ? kOffDAct : kOffAct);
    const bool sel = ((x.lists >> which) & 1) != 0;
    const int to = sel ? x.to : x.from;      // (a list that is not selected: an empty window)
    const int s0 = clamp_len(o[x.from]);
    int s1 = clamp_len(o[to]), len = clamp_len(o[EG_YEARS]);
    s1 = s1 < s0 ? s0 : s1; len = len < s1 ? s1 : len;
    const int32_t ol = o[l < 28 ? l : 27];
    int q = clamp_len(ol);
    q = q < s0 ? s0 : (q > s1 ? s1 : q);
    int before = -1;
    const int K = write_window(dst, words(src), lane, s0, s1, mapv, q, &before);
    const int D = (s1 - s0) - K;
    write_around_window(dst, src, lane, s0, s0 + K, len - D, D);
    if ((lane >> 5) == which) {
      uint32_t v = (uint32_t)ol;      // (unsigned: whatever the block holds, the sums wrap)
      if (l > x.from && l <= to) v = (uint32_t)(s0 + (before < 0 ? K : before));
      else if (l > to && l <= EG_YEARS) v -= (uint32_t)D;
      my_off = (int32_t)v;
    }
  }
  write_offset_entries(blk, lane, [=](int, int) { return my_off; });
  // masks: a year of the window from its two stretches of the source, mapped again; the others are the plan's
  const Base b = view(pa);
  const int lists = x.lists;
  Masks mine = {0ull, 0ull};
  const int y0 = lists != 0 ? x.from : 0, y1 = lists != 0 ? x.to : 0;
  for (int y = y0; y < y1; ++y) {
    const Masks m = year_masks<true>(b.off[y], b.off[y + 1], b.doff[y], b.doff[y + 1], lane, [=](int which, int i) {
      const int e = (which ? b.dact : b.act)[i];
      if (((lists >> which) & 1) == 0) return e;
      return e < 64 ? (int)mp[e] : (int)kDrop;
    });
    if (lane == y) mine = m;
  }
  write_masks(blk, b, lane, lane >= y0 && lane < y1, mine);
}
