// eg_plan_constraints.h — k_plan_constraints: the plan constraints of a context (include/eirgrid_hip.h eg_plan_constraints_set) judged over the
// n records of a plan batch, behind the batch's rollout grids on the stream they ran on; and the two pieces of a judgment that
// k_build_constraints (eg_build_constraints.h) shares with it: pcons::stage_rows, the staging of a record's yearly rows, and
// pcons::store_judgment, everything behind the fold.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_rewrites.h.
//
// A wave per variant, four variants per workgroup of 256 (pblock::my_variant).  The variant's 26 x 21 yearly rows — 546 doubles, one
// contiguous stretch of its record — come in with nine coalesced 8-byte loads a lane and are staged in the wave's own 4 368 bytes of LDS;
// behind one workgroup barrier lane i < k folds constraint i over its window, year by year, in the order the header defines (the
// build forms no FMA; a subtraction or an addition a year, each rounded once).  One ballot makes the mask.  Lane 0 stores the mask and,
// where it is not zero, the status; the lanes < k store the excess row, a NaN as the canonical quiet NaN.  A record that did not end
// EG_EP_OK keeps its status and gets mask 0 and a row of NaNs.
// No wave returns ahead of the barrier: a wave without a variant (the last workgroup's tail) and a record that failed skip the loads and
// the stores, not the barrier.  No scratch memory, no atomic, nothing but vector loads and stores; the kernel writes bytes rec::status
// .. +4 of record j and rows j of the two side buffers, nothing else.  The host has validated every constraint
// (eg_plan_constraints_validate); the kernel clamps column and window all the same, so what it indexes LDS with stays inside the
// wave's rows whatever the buffer holds.
// The staging is stage_rows, the canonical NaN, the ballot and the three stores are store_judgment: the kernel itself is the status
// test, the barrier and the fold between them.
#pragma once

namespace pcons {

constexpr int kRows = EG_YEARS * EG_YEARLY_FIELDS;                   // 546 doubles of a record's yearly rows
constexpr int kLoads = (kRows + kWave - 1) / kWave;                  // 9 loads a lane
constexpr unsigned long long kQuietNaN = 0x7FF8000000000000ull;      // what a NaN excess is stored as

// what the host uploads per constraint: eg_plan_constraint, 16 bytes — column, aggregate, op, from_year, to_year, pad[3]; bound
struct Packed { uint32_t head, to; double bound; };
static_assert(sizeof(Packed) == 16 && sizeof(eg_plan_constraint) == 16, "eg_plan_constraint is part of the C ABI");

// the excess of one constraint over the rows v (26 x 21 doubles, in LDS)
__device__ __forceinline__ double excess_of(const double* v, const Packed& p) {
  int col = (int)(p.head & 0xFFu), from = (int)(p.head >> 24), to = (int)(p.to & 0xFFu);
  const bool sum = ((p.head >> 8) & 0xFFu) == EG_AGG_SUM, ge = ((p.head >> 16) & 0xFFu) == EG_OP_GE;
  col = col > EG_YEARLY_FIELDS - 1 ? EG_YEARLY_FIELDS - 1 : col;
  to = to < 1 ? 1 : (to > EG_YEARS ? EG_YEARS : to);
  from = from >= to ? to - 1 : from;
  const double bound = p.bound;
  const double* at = v + from * EG_YEARLY_FIELDS + col;
  if (sum) {
    double s = at[0];
    for (int y = from + 1; y < to; ++y) { at += EG_YEARLY_FIELDS; s = s + at[0]; }
    return ge ? bound - s : s - bound;
  }
  double e = ge ? bound - at[0] : at[0] - bound;
  for (int y = from + 1; y < to; ++y) {
    at += EG_YEARLY_FIELDS;
    const double x = ge ? bound - at[0] : at[0] - bound;
    if (e == e && (x != x || x > e)) e = x;
  }
  return e;
}

// record j's 546 yearly doubles into the wave's rows v: nine coalesced loads a lane, then nine stores
// (the lane is masked here, where the bounds are tested: the compiler folds the ninth test as it did when the loops stood in the kernel)
__device__ __forceinline__ void stage_rows(double* v, const DevOut& o, uint32_t j, int lane) {
  lane &= kWave - 1;
  const double* src = o.yearly(j);
  double r[kLoads];
#pragma unroll
  for (int i = 0; i < kLoads; ++i) r[i] = lane + i * kWave < kRows ? src[lane + i * kWave] : 0.0;
#pragma unroll
  for (int i = 0; i < kLoads; ++i) if (lane + i * kWave < kRows) v[lane + i * kWave] = r[i];
}

// the judgment of record j from the fold on: lane `lane` of the wave holds constraint `lane` of k (mine: lane < k), live: j < n, ok: the
// record ended EG_EP_OK.  Where ok && mine the lane's excess is fold(), a NaN as the canonical quiet NaN; everywhere else that NaN.  One
// ballot makes the mask, the lanes < k store the excess row, lane 0 the mask and, where it is not zero, the demotion.
// (fold is a closure that captures by value, and mine comes by reference: with either the other way the same statements compile to
//  other machine code than they did inside the kernels — profiles/r17_constraints_identity.txt)
template <class Fold>
__device__ __forceinline__ void store_judgment(const DevOut& o, bool live, bool ok, const bool& mine, Fold fold, uint32_t k, int lane, uint32_t j,
                                               uint32_t* __restrict__ violated, double* __restrict__ excess) {
  double e = __longlong_as_double((long long)kQuietNaN);
  if (ok && mine) {
    e = fold();
    if (e != e) e = __longlong_as_double((long long)kQuietNaN);
  }
  const uint32_t mask = (uint32_t)__ballot(ok && mine && !(e <= 0.0));
  if (live) {
    if (mine) excess[(size_t)j * k + (uint32_t)lane] = e;
    if (lane == 0) {
      violated[j] = mask;
      if (mask != 0u) *o.status(j) = EG_EP_INFEASIBLE;
    }
  }
}

}  // namespace pcons

__global__ void __launch_bounds__(256) k_plan_constraints(DevOut o, uint32_t n, const pcons::Packed* __restrict__ cons, uint32_t k, uint32_t* __restrict__ violated,
                                                          double* __restrict__ excess) {
  using namespace pcons;
  __shared__ double rows[4][kRows];
  const pblock::Wave w = pblock::my_variant();
  const int lane = w.lane;
  double* v = rows[threadIdx.x >> 6];
  k = k > EG_CONSTRAINTS_MAX ? EG_CONSTRAINTS_MAX : k;
  const bool live = w.j < n;
  const bool ok = live && *o.status(live ? w.j : 0u) == EG_EP_OK;      // (the same word in every lane of the wave)
  if (ok) stage_rows(v, o, w.j, lane);
  __syncthreads();
  const bool mine = (uint32_t)lane < k;
  store_judgment(o, live, ok, mine, [=] { return excess_of(v, cons[lane]); }, k, lane, w.j, violated, excess);
}
