// eg_build_constraints.h — k_build_constraints: the build constraints of a context (include/eirgrid_hip.h eg_build_constraints_set) judged
// over the n records of a plan batch TOGETHER WITH its row constraints: it runs in place of k_plan_constraints when at least one build
// constraint is set, so a record gets one mask, one excess row and one demotion.  Included by eg_rollout.hip (eg_rollout.o only) behind
// eg_repair.h.
//
// A wave per variant, four variants per workgroup of 256 (pblock::my_variant), k_plan_constraints' shape.  Per wave: its 26 x 19 bins of
// uint32_t (1 976 bytes of LDS) are zeroed; with k_rows > 0 the variant's 546 yearly doubles are staged by pcons::stage_rows
// (eg_plan_constraints.h: k_plan_constraints' staging); the two lists of what the episode built — gen_pack[n_gens], off_pack[n_offsets], the counts clamped to 0..4 096 — are walked with 8-byte
// loads, four entries a lane, the entries at or behind the count masked by index (a load never leaves the list's 8 192 bytes), and every
// entry with a class and a year in range adds 1 to bin [year][class] with an LDS integer atomic: integer adds commute, so the bins do not
// depend on the order.  Behind a workgroup barrier lane i < k_rows folds row constraint i (pcons::excess_of, the one definition), lane
// k_rows <= i < k folds build constraint i - k_rows out of the bins in the order the header defines: per year (EG_AGG_EVERY) or for the
// window's integer totals (EG_AGG_SUM) s = +0.0, then s = s + weight[q] * (double)count for q = 0..18, a product and a sum each rounded
// once (the build forms no FMA).  The canonical NaN, the ballot that makes the mask and the stores are pcons::store_judgment, the one
// definition behind both kernels.
// No wave returns ahead of a barrier: a wave without a variant and a record that failed skip loads, atomics and fold, not the barriers.
// No scratch memory, no global atomic; the kernel writes bytes rec::status .. +4 of record j and rows j of the two side buffers, nothing
// else.  The host has validated every constraint; the kernel clamps the counts, the windows and k all the same.
#pragma once

namespace bcons {

constexpr int kBins = EG_YEARS * EG_BUILD_CLASSES;      // 494 counters of a wave
constexpr int kGenClasses = 15, kOffsetClasses = 4;
static_assert(kGenClasses + kOffsetClasses == EG_BUILD_CLASSES && kGenClasses == EG_N_TYPES, "the classes are the generator types, then the four offsets");
static_assert(rec::gen_pack % 8 == 0 && rec::off_pack % 8 == 0 && rec::stride % 8 == 0, "the lists are read in 8-byte words");
static_assert(EG_MAX_GENS % 4 == 0 && EG_MAX_OFFSETS % 4 == 0, "a list is whole 8-byte words");

// what the host uploads per constraint: eg_build_constraint, 168 bytes — aggregate, op, from_year, to_year, pad[4]; bound; weight[19]
struct Packed { uint32_t head, pad; double bound; double weight[EG_BUILD_CLASSES]; };
static_assert(sizeof(Packed) == 168 && sizeof(eg_build_constraint) == 168, "eg_build_constraint is part of the C ABI");

// one list of a record into the bins: entries i < count of `list`, class base + (pk & 15) where that nibble is below `classes`
__device__ __forceinline__ void count_list(uint32_t* bins, const uint16_t* list, int count, int cap, int base, int classes, int lane) {
  count = count < 0 ? 0 : (count > cap ? cap : count);
  const uint2* words = reinterpret_cast<const uint2*>(list);
  for (int w = lane; w * 4 < count; w += kWave) {
    const uint2 two = words[w];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const uint32_t pk = ((h < 2 ? two.x : two.y) >> ((h & 1) * 16)) & 0xFFFFu;
      const int q = (int)(pk & 15u), y = (int)((pk >> 4) & 31u);
      if (w * 4 + h < count && q < classes && y < EG_YEARS) atomicAdd(&bins[y * EG_BUILD_CLASSES + base + q], 1u);
    }
  }
}

// the excess of one build constraint over the bins c[26][19] (in LDS)
__device__ __forceinline__ double excess_of(const uint32_t* c, const Packed* p) {
  const uint32_t head = p->head;
  int from = (int)((head >> 16) & 0xFFu), to = (int)(head >> 24);
  const bool sum = (head & 0xFFu) == EG_AGG_SUM, ge = ((head >> 8) & 0xFFu) == EG_OP_GE;
  to = to < 1 ? 1 : (to > EG_YEARS ? EG_YEARS : to);
  from = from >= to ? to - 1 : from;
  const double bound = p->bound;
  double w[EG_BUILD_CLASSES];
#pragma unroll
  for (int q = 0; q < EG_BUILD_CLASSES; ++q) w[q] = p->weight[q];
  if (sum) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < EG_BUILD_CLASSES; ++q) {
      uint32_t m = 0u;
      for (int y = from; y < to; ++y) m += c[y * EG_BUILD_CLASSES + q];
      s = s + w[q] * (double)m;
    }
    return ge ? bound - s : s - bound;
  }
  double e = 0.0;
  for (int y = from; y < to; ++y) {
    const uint32_t* at = c + y * EG_BUILD_CLASSES;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < EG_BUILD_CLASSES; ++q) s = s + w[q] * (double)at[q];
    const double x = ge ? bound - s : s - bound;
    if (y == from || (e == e && (x != x || x > e))) e = x;
  }
  return e;
}

}  // namespace bcons

__global__ void __launch_bounds__(256) k_build_constraints(DevOut o, uint32_t n, const pcons::Packed* __restrict__ rows_cons, uint32_t k_rows,
                                                           const bcons::Packed* __restrict__ build_cons, uint32_t k_builds,
                                                           uint32_t* __restrict__ violated, double* __restrict__ excess) {
  __shared__ double rows[4][pcons::kRows];
  __shared__ uint32_t bins[4][bcons::kBins];
  const pblock::Wave w = pblock::my_variant();
  const int lane = w.lane;
  double* v = rows[threadIdx.x >> 6];
  uint32_t* c = bins[threadIdx.x >> 6];
  k_rows = k_rows > EG_CONSTRAINTS_MAX ? EG_CONSTRAINTS_MAX : k_rows;
  k_builds = k_builds > EG_CONSTRAINTS_MAX - k_rows ? EG_CONSTRAINTS_MAX - k_rows : k_builds;
  const uint32_t k = k_rows + k_builds;
  const bool live = w.j < n;
  const bool ok = live && *o.status(live ? w.j : 0u) == EG_EP_OK;      // (the same word in every lane of the wave)
  for (int i = lane; i < bcons::kBins; i += kWave) c[i] = 0u;
  if (ok && k_rows > 0u) pcons::stage_rows(v, o, w.j, lane);
  __syncthreads();      // (the zeros stand before the first add)
  if (ok) {
    bcons::count_list(c, o.gen_pack(w.j), *o.n_gens(w.j), EG_MAX_GENS, 0, bcons::kGenClasses, lane);
    bcons::count_list(c, o.off_pack(w.j), *o.n_offsets(w.j), EG_MAX_OFFSETS, bcons::kGenClasses, bcons::kOffsetClasses, lane);
  }
  __syncthreads();
  const bool mine = (uint32_t)lane < k;
  pcons::store_judgment(o, live, ok, mine, [=] {
    return (uint32_t)lane < k_rows ? pcons::excess_of(v, rows_cons[lane]) : bcons::excess_of(c, build_cons + ((uint32_t)lane - k_rows));
  }, k, lane, w.j, violated, excess);
}
