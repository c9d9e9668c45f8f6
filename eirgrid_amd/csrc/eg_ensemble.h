// eg_ensemble.h — k_ensemble_keep, k_ensemble_commit: a plan batch judged over R draw streams (include/eirgrid_hip.h eg_plan_streams_set;
// eg_streams.cpp, eg_plans.cpp launch_plans).  Included by eg_rollout.hip (eg_rollout.o only) behind eg_build_constraints.h.
//
// With R >= 2 streams set a plan batch runs R passes, stream R-1 first and stream 0 last, each the whole batch as it runs without
// streams — rollout grids, long-plan chunks, the constraint kernel.  Behind every pass k_ensemble_keep, a thread a variant, copies what
// the pass left of a record's metrics[4] and status into slab r of the context's store (ens::Kept, 40 bytes; entry (r, j) is slabs[r * n
// + j]).  Behind the last pass the records hold stream 0's episode and k_ensemble_commit runs once: a wave a variant, four variants per
// workgroup of 256 (pblock::my_variant), a lane a stream.
//   load      lane r < R loads entry (r, j) and computes s_r = rm::rank_score(m_r, mode);
//   rank      the lanes that come before a lane in the order "a NaN score first, then the smaller score, then the lower r" are counted in
//             one uniform loop of R readlane broadcasts of s; the same loop folds score_sum, score_min and score_max in ascending r;
//   tail sum  the lanes of rank < tail are one ballot; a uniform loop over its set bits, ascending, starts each sum from the first
//             selected stream's value and adds the others with plain double adds (a tree would change the bits), then divides by tail;
//   counters  n_ok, n_infeasible, the first stream that did not end EG_EP_OK and the worst stream are ballots;
//   stores    lane 0 writes the record's metrics and status (36 bytes) and the eg_ensemble_row (128 bytes), vector stores in plain C++.
// No LDS, no scratch memory, no atomic, no barrier: a wave without a variant (the last workgroup's tail) returns at once.  No index is
// read from memory; R and tail are clamped to 1..EG_STREAMS_MAX and 1..R all the same, so a lane's entry lies inside the R slabs.
#pragma once

namespace ens {

struct Kept { double m[4]; int32_t status, pad; };      // what a pass leaves of a record
static_assert(sizeof(Kept) == 40 && sizeof(eg_ensemble_row) == 128 && EG_STREAMS_MAX == kWave, "a lane a stream; the store is 40 bytes a variant and stream");

}  // namespace ens

__global__ void __launch_bounds__(256) k_ensemble_keep(DevOut o, uint32_t n, ens::Kept* __restrict__ slab) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const double* m = o.metrics(j);
  ens::Kept k;
  k.m[0] = m[0]; k.m[1] = m[1]; k.m[2] = m[2]; k.m[3] = m[3];
  k.status = *o.status(j); k.pad = 0;
  slab[j] = k;
}

__global__ void __launch_bounds__(256) k_ensemble_commit(DevOut o, uint32_t n, const ens::Kept* __restrict__ slabs, uint32_t R, uint32_t tail, int mode,
                                                         eg_ensemble_row* __restrict__ rows) {
  const pblock::Wave w = pblock::my_variant();
  if (w.j >= n) return;      // (the whole wave: j is the wave's)
  const int lane = w.lane;
  R = R < 1u ? 1u : (R > (uint32_t)EG_STREAMS_MAX ? (uint32_t)EG_STREAMS_MAX : R);
  tail = tail < 1u ? 1u : (tail > R ? R : tail);
  const bool mine = (uint32_t)lane < R;
  const ens::Kept* e = slabs + (size_t)(mine ? lane : 0) * n + w.j;
  const double m0 = e->m[0], m1 = e->m[1], m2 = e->m[2], m3 = e->m[3];
  const int st = e->status;
  const double mm[4] = {m0, m1, m2, m3};
  const double s = rm::rank_score(mm, mode);
  const bool s_nan = s != s;
  // the streams that come before this lane's, and the three folds over the scores, stream by stream
  int before = 0;
  double s_sum = 0.0, s_min = 0.0, s_max = 0.0;
  bool any = false;
  for (int q = 0; q < (int)R; ++q) {
    const double sq = readlane_f64(s, q);
    const bool q_nan = sq != sq;
    before += q_nan ? (!s_nan || q < lane) : (!s_nan && (sq < s || (sq == s && q < lane)));
    s_sum = q == 0 ? sq : s_sum + sq;
    if (!q_nan) {
      if (!any || sq < s_min) s_min = sq;
      if (!any || sq > s_max) s_max = sq;
      any = true;
    }
  }
  if (!any) { s_min = __longlong_as_double(0x7FF8000000000000ll); s_max = s_min; }
  // the mean of the tail: the selected streams in ascending r
  unsigned long long sel = __ballot(mine && before < (int)tail);
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  for (bool first = true; sel != 0ull; first = false, sel &= sel - 1ull) {
    const int q = __ffsll((long long)sel) - 1;
    const double a0 = readlane_f64(m0, q), a1 = readlane_f64(m1, q), a2 = readlane_f64(m2, q), a3 = readlane_f64(m3, q);
    c0 = first ? a0 : c0 + a0; c1 = first ? a1 : c1 + a1; c2 = first ? a2 : c2 + a2; c3 = first ? a3 : c3 + a3;
  }
  const double d = (double)tail;
  c0 = c0 / d; c1 = c1 / d; c2 = c2 / d; c3 = c3 / d;
  const unsigned long long ok = __ballot(mine && st == EG_EP_OK), infeasible = __ballot(mine && st == EG_EP_INFEASIBLE), bad = __ballot(mine && st != EG_EP_OK);
  const unsigned long long worst = __ballot(mine && before == 0);
  const int status = bad == 0ull ? EG_EP_OK : __builtin_amdgcn_readlane(st, __ffsll((long long)bad) - 1);
  const double n0 = readlane_f64(m0, 0), n1 = readlane_f64(m1, 0), n2 = readlane_f64(m2, 0), n3 = readlane_f64(m3, 0);
  if (lane == 0) {
    double* m = o.metrics(w.j);
    m[0] = c0; m[1] = c1; m[2] = c2; m[3] = c3;
    *o.status(w.j) = status;
    eg_ensemble_row row;
    row.nominal[0] = n0; row.nominal[1] = n1; row.nominal[2] = n2; row.nominal[3] = n3;
    row.committed[0] = c0; row.committed[1] = c1; row.committed[2] = c2; row.committed[3] = c3;
    row.score_min = s_min; row.score_max = s_max; row.score_sum = s_sum;
    row.n_ok = __popcll(ok); row.n_infeasible = __popcll(infeasible); row.n_failed = (int)R - __popcll(ok) - __popcll(infeasible);
    row.worst_stream = __ffsll((long long)worst) - 1;
    row.status = status;
#pragma unroll
    for (int i = 0; i < 5; ++i) row.pad[i] = 0;
    rows[w.j] = row;
  }
}
