// eg_update_kernels.h — the kernels of eg_rollout.hip that are not rollouts: single placement searches, the statistics and the best
// pick of a finished batch, the reference's best_result fold, and the batch update on the device.  Included by eg_rollout.hip at the
// end of its anonymous namespace, behind eg_explore.h, inside `#ifndef EG_TU_THROUGHPUT`: eg_rollout.o only.  Needs from eg_rollout.hip
// place_search (k_place), chunk_reduce (k_place_xy), load_state, load_stats_params and episode_update_stats (k_update_stats), sm,
// load_static_tables, wave_sync and EG_QR; and eg_detpow.h and eg_reduced_math.h (every formula of the update, shared with the
// host's eg_policy.cpp).
//
//   k_place, k_place_xy                        one placement search: over the episode tables; with the reference's own signature
//   stalled_tables_year, k_stalled_tables      the stalled sampler's tables of a snapshot
//   k_update_stats                             the statistics of a finished batch without running it again
//   k_pick_best                                the best episode of a batch, its record copied behind the statistics
//   fold_impact, fold_windows, k_fold_best     the reference's best_result, folded speculatively 1024 results at a time
//   k_fold_pack, k_fold_gathered               the same fold over the ranks of a group
//   chacha12_block, k_apply_update             the batch update in one 1024-thread workgroup, the policy left in the snapshot buffer
//
// Reference (relative to the reference's aiSimulator/src/):
//   placement      gpu/metal_location_search.rs:96-176
//   stalled tables ai/learning/weights/sampling.rs:190-220
//   best_result    core/multi_simulation.rs:384, :611-620, :821-905; ai/metrics/scoring.rs:46-85
//   update         core/multi_simulation.rs:494-508, ai/learning/weights/learning.rs (restated in eg_policy.cpp: eg_policy_apply_reduced)
#pragma once

// ---- B2: a single placement search, for parity tests of the arg-max --------------------------------------------
__global__ void __launch_bounds__(kWave) k_place(DevTables T, int type, int yi, const uint16_t* __restrict__ cells,
                                                 int n_extra, int32_t* out_cell, double* out_score) {
  const int lane = threadIdx.x;
  for (int g = lane; g < n_extra; g += kWave) sm.gcell[g] = cells[g];
  load_static_tables<true>(T, lane, true);      // (the factor table as two planes, as the lean grid holds it)
  __syncthreads();
  double score = 0.0;
  PrefixCache pc0 = {0.0, -1, 0};
  int nchunks = 0;
  const int cell = place_search<0, false, true>(T, lane, yi, type, n_extra, &score, nullptr, pc0, []() {}, nchunks);
  if (lane == 0) { *out_cell = cell; *out_score = score; }
}

// ---- B2 with the reference's own signature: generators at arbitrary coordinates, a size penalty --------------------
// MetalLocationSearch::find_suitable_location (metal_location_search.rs:96-176) for the ctx's settlements (populations of
// year `yi`) and existing plant — that part of every candidate's product is the host table te, in the reference's order —
// times, for each of the caller's generators in list order, distance / radius when closer than the radius (sqrt and division
// are IEEE correctly rounded here as in the reference), times the coast factor, times 1 - size_penalty * 0.1.  All 2601
// distinct candidates are evaluated (no generator sits on the 1 km grid, so nothing of the rollout's tables applies);
// first maximum in (i, j) order = highest score, ties to the lowest cell.
__global__ void __launch_bounds__(kWave) k_place_xy(DevTables T, int type, int yi, const double* __restrict__ gx, const double* __restrict__ gy,
                                                    int n, double radius, double size_term, int32_t* out_cell, double* out_score) {
  const int lane = threadIdx.x;
  const int rc = T.rclass()[type], v = T.variant()[type];
  const PsRec* __restrict__ list = T.ps() + (size_t)(yi * kMaxVariants + v) * kPsStride;
  (void)rc;
  double best = 0.0; int best_c = kCells;
  for (int r = lane; r < kCells; r += kWave) {
    const PsRec c = list[r];
    const int ci = (int)c.cell / kGrid, cj = (int)c.cell - ci * kGrid;
    const double x = (double)ci * 1000.0, y = (double)cj * 1000.0;
    double score = c.te;
    for (int g = 0; g < n; ++g) {
      const double dx = x - gx[g], dy = y - gy[g];
      const double distance = __builtin_sqrt(dx * dx + dy * dy);
      if (distance < radius) score = score * (distance / radius);
    }
    score = score * c.cf;            // 1.0 for the types without the coast term (x * 1.0 == x)
    score = score * size_term;
    if (score > best || (score == best && score > 0.0 && (int)c.cell < best_c)) { best = score; best_c = (int)c.cell; }
  }
  const ChunkBest b = chunk_reduce<false>(best, best_c, 0.0);
  if (lane == 0) { *out_cell = b.score > 0.0 ? b.cell : -1; *out_score = b.score; }
}

// Stalled sampler tables of a freshly uploaded snapshot (sampling.rs:190-220 on the un-nudged rows): per year the
// weights in stable descending order raised to the power (shared eg_detpow), the permutation and the table-order sum.
// One workgroup per year; runs on the stream right behind the snapshot copy.
// (one wave per year; `s_w`, `s_scaled`: 64 doubles of LDS each, the wave's own)
__device__ __forceinline__ void stalled_tables_year(uint8_t* snap_base, int y, int lane, uint32_t stall, double* s_w, double* s_scaled) {
  const double stagnation = rm::dmind((double)stall / 1000.0, 3.0);
  const double power = 1.0 + (2.0 * stagnation);
  double* row = reinterpret_cast<double*>(snap_base + snap::pol) + y * snap::kPolRow;
  const double* w = row;
  double* scaled = reinterpret_cast<double*>(snap_base + snap::scaled) + y * 64;
  uint8_t* perm = snap_base + snap::scaled_perm + y * 64;
  const double mine = lane < EG_N_ACTIONS ? w[lane] : 0.0;
  wave_sync();
  s_w[lane] = mine;
  wave_sync();
  if (lane < EG_N_ACTIONS) {
    int rank = 0;
    for (int b = 0; b < EG_N_ACTIONS; ++b) { const double o = s_w[b]; rank += (o > mine || (o == mine && b < lane)) ? 1 : 0; }
    const double v = eg_detpow(mine, power);
    s_scaled[rank] = v; scaled[rank] = v; perm[rank] = (uint8_t)lane;
  }
  // (the table-order sum of the powered weights is not kept: weighted_pick forms it from the table it is handed — a lane adding 61
  //  LDS words one after the other was 4 of k_apply_update's microseconds in every stalled update; slot kPolScaledTotal stays 0)
}
__global__ void __launch_bounds__(kWave) k_stalled_tables(uint8_t* snap_base) {
  __shared__ double s_w[64], s_scaled[64];
  const uint32_t stall = reinterpret_cast<const DevState*>(snap_base + snap::state)->stall;
  if (stall <= 500u) return;
  stalled_tables_year(snap_base, blockIdx.x, threadIdx.x, stall, s_w, s_scaled);
}

// statistics of a finished batch without re-running it (same accumulation as the k_rollout epilogue)
__global__ void __launch_bounds__(kWave) k_update_stats(DevOut O, DevSnapshot S_in, uint32_t n, long long* stats) {
  const uint32_t e = blockIdx.x;
  if (e >= n) return;
  DevSnapshot S = S_in; StatsParams P;
  load_state(S); load_stats_params(S, P);
  episode_update_stats(O, S, P, e, threadIdx.x, stats);
}

// best episode of the batch: highest score, ties to the lowest index; its metrics and action lists are copied behind
// the statistics so that one transfer carries everything the host-side update needs
__global__ void __launch_bounds__(1024) k_pick_best(DevOut O, uint32_t n, unsigned long long first_index, UpdateCandidate* cand) {
  __shared__ double s_score[1024];
  __shared__ int s_idx[1024];
  const int tid = threadIdx.x;
  double best = -1.0; int best_i = -1;
  for (uint32_t i = tid; i < n; i += 1024) {
    const double sc = O.score_list[i];
    if (sc > best) { best = sc; best_i = (int)i; }      // ascending i per thread: first maximum
  }
  s_score[tid] = best; s_idx[tid] = best_i;
  __syncthreads();
  for (int w = 512; w >= 1; w >>= 1) {
    if (tid < w) {
      const double o = s_score[tid + w]; const int oi = s_idx[tid + w];
      if (oi >= 0 && (o > s_score[tid] || (o == s_score[tid] && (s_idx[tid] < 0 || oi < s_idx[tid])))) { s_score[tid] = o; s_idx[tid] = oi; }
    }
    __syncthreads();
  }
  const int win = s_idx[0];
  if (tid == 0) { cand->score = win >= 0 ? s_score[0] : -1.0; cand->index = win >= 0 ? (long long)(first_index + (unsigned long long)win) : -1ll; }
  if (win < 0) return;
  if (tid < 4) cand->metrics[tid] = O.metrics(win)[tid];
  if (tid < EG_YEARS) { cand->n_run[tid] = O.n_run(win)[tid]; cand->n_def[tid] = O.n_def(win)[tid]; }
  for (int i = tid; i < EG_RUN_CAP; i += 1024) cand->run_log[i] = O.run_log(win)[i];
  for (int i = tid; i < EG_DEF_CAP; i += 1024) cand->def_log[i] = O.def_log(win)[i];
}

// ---- the reference's `best_result` (core/multi_simulation.rs:384, :613-620): which run is summarised and exported ------
// After its parallel section the reference folds the results in iteration order:
//     best_result = None;  for result in results { if best_result.map_or(true, |best|
//         evaluate_action_impact(result.metrics -> best.metrics, optimization_mode) > 0.0) { best_result = Some(result) } }
// with the arguments as written — `result` is the "current state" and `best` the "new state", so a result takes over when
// the held one is an IMPROVEMENT on it.  That is the run multi_simulation.rs:821-905 prints and exports, and it is not the
// policy's best strategy (score_metrics, strategy.rs:19-258).  The fold is sequentially dependent but a result rarely takes
// over (the held run drifts towards the worst: a running extreme), so it is evaluated speculatively: 1024 results at a time
// against the held run, the FIRST that takes over (lowest index) becomes the held run and the rest of the window is
// examined again — the sequential fold's answer, in n / 1024 + (take-overs) rounds.  Failed episodes are skipped (in the
// reference a failed iteration ends the run, multi_simulation.rs:611).  The winner's whole record is kept behind the state.
__device__ __forceinline__ double fold_impact(const double* cur, const double* nxt, int cost_only) {      // scoring.rs:46-85
  State c, x;
  c.net = cur[0]; c.opinion = cur[1]; c.balance = 0.0; c.cost = cur[2];      // metrics_to_action_result, multi_simulation.rs:55-62
  x.net = nxt[0]; x.opinion = nxt[1]; x.balance = 0.0; x.cost = nxt[2];
  if (cost_only) { const double cost_change = x.cost - c.cost; return -cost_change / dmax(dabs(c.cost), 1.0); }      // scoring.rs:52-58
  return evaluate_impact(c, x);
}
// The speculative windows, shared by k_fold_best (one context) and k_fold_gathered (the ranks of a group): `n` results in index order,
// `load(i, m)` gives result i's metrics (false: a failed episode, skipped).  The held run is s_best / s_has (in LDS, read and left
// there); s_win ends as the position (0 .. n-1) of the last take-over, -1 when the held run stays.
template <typename Load>
__device__ __forceinline__ void fold_windows(uint32_t n, int cost_only, Load load, double* s_best, int& s_has, int& s_first, int& s_win) {
  constexpr int kPer = 8;      // results per thread and tile, in registers
  const int tid = threadIdx.x;
  for (uint32_t tile = 0; tile < n; tile += kPer * 1024u) {
    double m[kPer][4]; bool ok[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const uint32_t i = tile + (uint32_t)k * 1024u + (uint32_t)tid;
      ok[k] = i < n && load(i, m[k]);
      if (!ok[k]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) m[k][j] = 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {      // window k: results tile + 1024 k + [0, 1024), in index order = thread order
      int from = 0;
      for (;;) {
        double b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = s_best[j];
        const bool take = tid >= from && ok[k] && (s_has == 0 || fold_impact(m[k], b, cost_only) > 0.0);
        if (take) atomicMin(&s_first, tid);
        __syncthreads();
        const int f = s_first;
        __syncthreads();      // everybody has read it
        if (f == 0x7FFFFFFF) break;
        if (tid == f) {
#pragma unroll
          for (int j = 0; j < 4; ++j) s_best[j] = m[k][j];
          s_has = 1; s_win = (int)(tile + (uint32_t)k * 1024u) + f; s_first = 0x7FFFFFFF;
        }
        from = f + 1;
        __syncthreads();
      }
    }
  }
  __syncthreads();
}
__global__ void __launch_bounds__(1024) k_fold_best(DevOut O, uint32_t n, unsigned long long first_index, int cost_only, uint8_t* fold) {
  __shared__ double s_best[4];
  __shared__ int s_has, s_first, s_win;
  const int tid = threadIdx.x;
  FoldState* st = reinterpret_cast<FoldState*>(fold);
  if (tid < 4) s_best[tid] = st->metrics[tid];
  if (tid == 0) { s_has = st->has; s_win = -1; s_first = 0x7FFFFFFF; }
  __syncthreads();
  fold_windows(n, cost_only, [&](uint32_t i, double* m) {
    if (*O.status(i) != EG_EP_OK) return false;
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = O.metrics(i)[j];
    return true;
  }, s_best, s_has, s_first, s_win);
  const int win = s_win;
  if (win < 0) return;      // the held run stays
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(O.base + (size_t)win * rec::stride);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(fold + kFoldRecord);
  for (int i = tid; i < (int)(rec::stride / 8); i += 1024) dst[i] = src[i];
  if (tid == 0) {
    for (int j = 0; j < 4; ++j) st->metrics[j] = s_best[j];
    st->index = (long long)(first_index + (unsigned long long)win); st->has = 1;
  }
}

// ---- the same fold over the ranks of a group (eg_group.cpp eg_group_step) -------------------------------------------------
// k_fold_pack runs behind a rank's rollout: what fold_impact reads of each result of the shard, 32 bytes apart (in the records
// they are rec::stride = 41.6 KB apart), written into the block that travels behind the rank's update packet.  With n == 0 it
// makes the packet an empty shard's message instead: eg_device_rollout(n = 0) does not touch the packet, which still holds the
// previous step's candidate — that must not reach the update again.
__global__ void __launch_bounds__(256) k_fold_pack(DevOut O, uint32_t n, uint8_t* packet, FoldEntry* block) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (n == 0) {
    long long* stats = reinterpret_cast<long long*>(packet);
    for (uint32_t k = threadIdx.x; k < (uint32_t)EG_STATS_LEN; k += 256u) stats[k] = 0;
    if (threadIdx.x == 0) {
      UpdateCandidate* c = reinterpret_cast<UpdateCandidate*>(packet + 8 * EG_STATS_LEN);
      c->score = -1.0; c->index = -1ll;
    }
    return;
  }
  if (i >= n) return;
  FoldEntry e;
  e.ok = *O.status(i) == EG_EP_OK ? 1 : 0; e.pad = 0;
  const double* m = O.metrics(i);
  e.net = e.ok ? m[0] : 0.0; e.opinion = e.ok ? m[1] : 0.0; e.cost = e.ok ? m[2] : 0.0;
  block[i] = e;
}
// k_fold_gathered runs on every rank over the gathered blocks of all ranks, in rank order = global index order: the same
// windows and the same fold_impact as k_fold_best, so the state it leaves is the same on every rank and the same as one
// context's fold over the whole step.  The winner's record is copied only by the rank whose shard held it, from its own records,
// and tagged there (index, step); no record crosses devices.
__global__ void __launch_bounds__(1024) k_fold_gathered(const uint8_t* gathered, unsigned long long slot_stride, int n_ranks, uint32_t n_global,
                                                       unsigned long long first_index, DevOut O, uint32_t own_first, uint32_t own_n, int cost_only,
                                                       uint32_t step, uint8_t* fold) {
  __shared__ double s_best[4];
  __shared__ int s_has, s_first, s_win;
  const int tid = threadIdx.x;
  GroupFoldState* st = reinterpret_cast<GroupFoldState*>(fold);
  if (tid < 4) s_best[tid] = st->metrics[tid];
  if (tid == 0) { s_has = st->has; s_win = -1; s_first = 0x7FFFFFFF; }
  __syncthreads();
  // parallel.shard_range: the first `rem` ranks hold base + 1 results, the others base
  const uint32_t base = n_global / (uint32_t)n_ranks, rem = n_global % (uint32_t)n_ranks, big = rem * (base + 1u);
  fold_windows(n_global, cost_only, [&](uint32_t i, double* m) {
    const uint32_t r = i < big ? i / (base + 1u) : rem + (i - big) / base;
    const uint32_t j = i < big ? i - r * (base + 1u) : (i - big) - (r - rem) * base;
    const FoldEntry* e = reinterpret_cast<const FoldEntry*>(gathered + (size_t)r * slot_stride + EG_PACKET_BYTES) + j;
    if (e->ok == 0) return false;
    m[0] = e->net; m[1] = e->opinion; m[2] = e->cost; m[3] = 0.0;
    return true;
  }, s_best, s_has, s_first, s_win);
  const int win = s_win;
  if (win < 0) return;      // the held run stays
  if ((uint32_t)win >= own_first && (uint32_t)win - own_first < own_n) {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(O.base + (size_t)((uint32_t)win - own_first) * rec::stride);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(fold + kFoldRecord);
    for (int i = tid; i < (int)(rec::stride / 8); i += 1024) dst[i] = src[i];
    if (tid == 0) { st->tag_index = (long long)(first_index + (unsigned long long)win); st->tag_step = step; }
  }
  if (tid == 0) {
    for (int j = 0; j < 4; ++j) st->metrics[j] = s_best[j];
    st->index = (long long)(first_index + (unsigned long long)win); st->has = 1; st->step = step;
  }
}

// ---- on-device batch update (eg_policy_apply_reduced, eg_policy.cpp, restated for one 1024-thread workgroup) -----------
// The policy lives in the snapshot buffer; this kernel consumes the (all-reduced) statistics and the candidate records
// of a batch and leaves the buffer as eg_upload_snapshot would have written it after the host update: weights, row
// sums, best lists / offsets / masks, scalars (derive_state) — the same bits, because every formula comes from
// eg_reduced_math.h.  The stalled sampler tables follow in k_stalled_tables.  The statistics are zeroed for the next batch.
__device__ void chacha12_block(const uint32_t* key, unsigned long long counter, uint32_t* out) {
  uint32_t s[16], x[16];
  s[0] = 0x61707865u; s[1] = 0x3320646eu; s[2] = 0x79622d32u; s[3] = 0x6b206574u;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[4 + i] = key[i];
  s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = 0u; s[15] = 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    EG_QR(x[0], x[4], x[8], x[12]) EG_QR(x[1], x[5], x[9], x[13]) EG_QR(x[2], x[6], x[10], x[14]) EG_QR(x[3], x[7], x[11], x[15])
    EG_QR(x[0], x[5], x[10], x[15]) EG_QR(x[1], x[6], x[11], x[12]) EG_QR(x[2], x[7], x[8], x[13]) EG_QR(x[3], x[4], x[9], x[14])
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

// `packets` = n_packets update packets, packet_stride bytes apart (one per rank, in rank order; the gathered copies when N > 1):
// the statistics are summed here (integers: any order gives the same sum), the candidate records sit behind them.
__global__ void __launch_bounds__(1024) k_apply_update(uint8_t* snap_base, const uint8_t* packets, int n_cands, unsigned long long packet_stride, long long* zero_stats,
                                                      unsigned long long noise_seed, const uint8_t* out_base, const double* score_list, uint32_t n_local,
                                                      unsigned long long first_index, int local_pick, uint32_t* list_len_out) {
  constexpr int NA = EG_N_ACTIONS, ND = EG_N_DEFICIT, Y = EG_YEARS;
  constexpr int kMainDraws = Y * NA, kDefDraws = Y * ND, kBlocks = (2 * (kMainDraws + kDefDraws) + 15) / 16;
  __shared__ uint32_t s_noise[kBlocks * 16];
  __shared__ uint32_t s_key[8];
  __shared__ DevState st;
  __shared__ int s_winner, s_improved, s_randomized_main, s_owned;
  __shared__ __align__(16) uint8_t s_best[snap::kBestCap]; __shared__ __align__(16) uint8_t s_bestd[snap::kBestCap];      // the best lists as they were before this update
  __shared__ int s_off[2][Y + 1];
  __shared__ double s_ln_boost;
  __shared__ rm::DeficitContrast s_dc;
  __shared__ int s_prefix[2][Y + 1];
  const int tid = threadIdx.x;
#ifdef EG_STAMPS
  __shared__ unsigned long long dbg_t[16];      // diagnostic: phase boundaries (100 MHz counter), see scripts/apply_phases.py
  if (tid == 0) dbg_t[0] = wall_clock64();
#endif
  double* pol = reinterpret_cast<double*>(snap_base + snap::pol);
  int32_t* best_off = reinterpret_cast<int32_t*>(snap_base + snap::best_off);
  int32_t* bestd_off = reinterpret_cast<int32_t*>(snap_base + snap::bestd_off);
  uint8_t* best_actions = snap_base + snap::best_actions;
  uint8_t* bestd_actions = snap_base + snap::bestd_actions;
  DevState* gstate = reinterpret_cast<DevState*>(snap_base + snap::state);

  // serial pieces run on different waves side by side: state + winner + "is it an improvement" on wave 1, the noise key on
  // wave 0
  const uint8_t* cands = packets + 8 * EG_STATS_LEN;      // record r at cands + r * packet_stride
  auto stat = [&](int i) {
    long long v = 0;
    for (int r = 0; r < n_cands; ++r) v += reinterpret_cast<const long long*>(packets + (size_t)r * packet_stride)[i];
    return v;
  };
  // Everything the contrast steps read is requested now and lands while the serial pieces run: the old best lists go to
  // LDS (the steps walk them per table entry), each thread's table entries and statistics into its registers.
  constexpr int kPen = 8, kMild = 8 + Y * NA, kDcnt = 8 + 2 * Y * NA;
  {
    const uint32_t* b4 = reinterpret_cast<const uint32_t*>(best_actions); const uint32_t* d4 = reinterpret_cast<const uint32_t*>(bestd_actions);
    reinterpret_cast<uint32_t*>(s_best)[tid] = b4[tid]; reinterpret_cast<uint32_t*>(s_bestd)[tid] = d4[tid];      // kBestCap = 4 x 1024 bytes
    if (tid <= Y) { s_off[0][tid] = best_off[tid]; s_off[1][tid] = bestd_off[tid]; }
  }
  double w_in[2] = {0.0, 0.0}, pen_in[2] = {0.0, 0.0}, dw_in = 0.0; long long dcnt_in = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + 1024 * k;
    if (i < Y * NA) { const int y = i / NA, a = i - y * NA; w_in[k] = pol[y * snap::kPolRow + a]; pen_in[k] = (double)stat(kPen + i) + (double)stat(kMild + i); }
  }
  if (tid < Y * ND) { const int y = tid / ND, sl = tid - y * ND; dw_in = pol[y * snap::kPolRow + snap::kPolDw + sl]; dcnt_in = stat(kDcnt + tid); }
  if (local_pick) {
    // One GPU: the candidate record of the packet is made here instead of by k_pick_best (a launch of 5.5 us per step).
    // The rollout epilogue left the batch's best score in statistics slot 3; the best episode is the lowest index that
    // holds it (highest score, ties to the lowest index), its metrics and lists are copied behind the statistics.
    UpdateCandidate* cw = reinterpret_cast<UpdateCandidate*>(const_cast<uint8_t*>(cands));
    const DevOut O{const_cast<uint8_t*>(out_base), const_cast<double*>(score_list)};
    const unsigned long long key = reinterpret_cast<const unsigned long long*>(packets)[3];
    if (tid == 0) s_winner = 0x7FFFFFFF;
    __syncthreads();
    if (key != 0ull)      // (from the back-to-back copy of the scores: one per 12 KB record cost 25 us at 16 384 episodes)
      for (uint32_t base = 0; base < n_local; base += 16u * 1024u) {
        double sc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { const uint32_t i = base + (uint32_t)k * 1024u + (uint32_t)tid; sc[k] = i < n_local ? O.score_list[i] : -1.0; }
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (sc[k] >= 0.0 && (unsigned long long)__double_as_longlong(sc[k]) + 1ull == key) atomicMin(&s_winner, (int)(base + (uint32_t)k * 1024u + (uint32_t)tid));
      }
    __syncthreads();
    const int win = s_winner != 0x7FFFFFFF ? s_winner : -1;
    if (tid == 0) { cw->score = win >= 0 ? *O.score(win) : -1.0; cw->index = win >= 0 ? (long long)(first_index + (unsigned long long)win) : -1ll; }
    if (win >= 0) {
      if (tid < 4) cw->metrics[tid] = O.metrics(win)[tid];
      if (tid < EG_YEARS) { cw->n_run[tid] = O.n_run(win)[tid]; cw->n_def[tid] = O.n_def(win)[tid]; }
      // (four bytes a thread: the lists start at multiples of four in the record and in the packet)
      static_assert(rec::run_log % 4 == 0 && rec::def_log % 4 == 0 && rec::stride % 4 == 0 && offsetof(UpdateCandidate, run_log) % 4 == 0 &&
                    offsetof(UpdateCandidate, def_log) % 4 == 0 && EG_RUN_CAP % 4 == 0 && EG_DEF_CAP % 4 == 0, "word copies of the winner's lists");
      for (int i = tid; i < EG_RUN_CAP / 4; i += 1024) reinterpret_cast<uint32_t*>(cw->run_log)[i] = reinterpret_cast<const uint32_t*>(O.run_log(win))[i];
      for (int i = tid; i < EG_DEF_CAP / 4; i += 1024) reinterpret_cast<uint32_t*>(cw->def_log)[i] = reinterpret_cast<const uint32_t*>(O.def_log(win))[i];
    }
    __syncthreads();      // the record is in place for every thread of this workgroup
  }
  if (tid == 64) {
    st = *gstate;
    // the batch's candidate: highest score, ties to the lowest global index (eg_policy_apply_packet)
    int win = -1; double ws = 0.0; long long wi = 0;
    for (int r = 0; r < n_cands; ++r) {
      const UpdateCandidate* c = reinterpret_cast<const UpdateCandidate*>(cands + (size_t)r * packet_stride);
      if (c->index < 0) continue;
      if (win < 0 || c->score > ws || (c->score == ws && c->index < wi)) { win = r; ws = c->score; wi = c->index; }
    }
    s_winner = win;
    bool improved = false;
    if (win >= 0 && stat(0) > 0) {
      const UpdateCandidate* c = reinterpret_cast<const UpdateCandidate*>(cands + (size_t)win * packet_stride);
      improved = !st.has_best || rm::score(c->metrics) > rm::score(st.best_metrics);
    }
    s_improved = improved ? 1 : 0;
  }
  // the two transcendental-heavy scalars of the contrast steps depend on the old state and the episode count only: each is
  // evaluated once, on a wave of its own, beside the pieces above (every thread used to evaluate them for itself)
  if (tid == 128) s_ln_boost = rm::contrast_ln_boost(gstate->learning_rate, gstate->stall);
  if (tid == 192) s_dc = rm::deficit_contrast(gstate->learning_rate, gstate->stall + (uint32_t)stat(0));   // the stall counter after a batch without improvement
  if (tid == 0) {
    unsigned long long state = noise_seed;      // rand_core seed_from_u64 (HostRng)
    for (int i = 0; i < 8; ++i) {
      state = state * 6364136223846793005ull + 11634580027462260723ull;
      const uint32_t x = (uint32_t)(((state >> 18) ^ state) >> 27), rot = (uint32_t)(state >> 59);
      s_key[i] = (x >> rot) | (x << ((32u - rot) & 31u));
    }
  }
  __syncthreads();
#ifdef EG_STAMPS
  if (tid == 0) dbg_t[1] = wall_clock64();
#endif
  const long long n_ok = stat(0), n_qual = stat(2);
  const bool contrast = st.has_best && st.has_lists && n_qual > 0;
  const bool randomize_main = contrast && st.stall > 1200u;
  // the noise stream is only needed beyond 1200 stalled episodes; the deficit table may need it even if the main one
  // did not (its stall counter is the updated one), so the blocks are made whenever either could
  const bool maybe_noise = st.stall + (uint32_t)n_ok > 1200u;
  if (maybe_noise && tid < kBlocks) chacha12_block(s_key, (unsigned long long)tid, s_noise + 16 * tid);
  __syncthreads();
#ifdef EG_STAMPS
  if (tid == 0) dbg_t[2] = wall_clock64();
#endif
  auto draw = [&](int j) {      // j-th gen::<f64>() of the stream
    const unsigned long long v = ((unsigned long long)s_noise[2 * j + 1] << 32) | s_noise[2 * j];
    return (double)(v >> 11) * (1.0 / 9007199254740992.0);
  };

  // ---- apply_contrast_learning over the batch ----
  if (contrast) {
    const double ln_boost = s_ln_boost;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const int i = tid + 1024 * k2;
      if (i >= Y * NA) break;
      const int y = i / NA, a = i - y * NA;
      int occ = 0;
      for (int k = s_off[0][y]; k < s_off[0][y + 1]; ++k) occ += s_best[k] == a ? 1 : 0;
      for (int k = s_off[1][y]; k < s_off[1][y + 1]; ++k) occ += s_bestd[k] == a ? 1 : 0;
      double w = rm::nudge(w_in[k2], (double)n_qual * (double)occ * ln_boost, pen_in[k2] / 4294967296.0);
      if (randomize_main) w = rm::noise(w, draw(i));
      pol[y * snap::kPolRow + a] = w;
    }
  }
  __syncthreads();
#ifdef EG_STAMPS
  if (tid == 0) dbg_t[3] = wall_clock64();
#endif

  // ---- update_best_strategy with the batch's candidate ----
  if (tid == 0) {
    const bool improved = s_improved != 0;
    st.iteration_count += (uint32_t)n_ok;
    st.failed_total += (uint32_t)stat(1);
    s_randomized_main = randomize_main ? 1 : 0;
    if (improved) {
      const UpdateCandidate* c = reinterpret_cast<const UpdateCandidate*>(cands + (size_t)s_winner * packet_stride);
      DevImprovement* log = reinterpret_cast<DevImprovement*>(snap_base + snap::imp_log) + (st.n_improvements % snap::kImpLogCap);
      log->score = rm::score(c->metrics); log->iteration = st.iteration_count; log->pad = 0;
      for (int k = 0; k < 4; ++k) { log->metrics[k] = c->metrics[k]; st.best_metrics[k] = c->metrics[k]; }
      st.n_improvements += 1;
      st.has_best = 1; st.has_lists = 1; st.stall = 0;
      int a = 0, b = 0;
      for (int y = 0; y < Y; ++y) { s_prefix[0][y] = a; s_prefix[1][y] = b; a += c->n_run[y]; b += c->n_def[y]; }
      s_prefix[0][Y] = a; s_prefix[1][Y] = b;
      const long long local = c->index - (long long)first_index;
      s_owned = (out_base && local >= 0 && local < (long long)n_local) ? 1 : 0;
      *reinterpret_cast<uint32_t*>(snap_base + snap::best_rec_state) = s_owned ? 1u : 2u;
    } else st.stall += (uint32_t)n_ok;
    st.improved_last = improved ? 1 : 0;
  }
  __syncthreads();
#ifdef EG_STAMPS
  if (tid == 0) dbg_t[4] = wall_clock64();
#endif
  const bool improved = s_improved != 0;
  if (improved) {      // the candidate's lists become the best lists; the main weights of this moment are kept beside them
    const UpdateCandidate* c = reinterpret_cast<const UpdateCandidate*>(cands + (size_t)s_winner * packet_stride);
    const int nr = s_prefix[0][Y], nd = s_prefix[1][Y];
    for (int i = tid; i < nr && i < (int)snap::kBestCap; i += 1024) best_actions[i] = c->run_log[i];
    for (int i = tid; i < nd && i < (int)snap::kBestCap; i += 1024) bestd_actions[i] = c->def_log[i];
    if (tid <= Y) { best_off[tid] = s_prefix[0][tid]; bestd_off[tid] = s_prefix[1][tid]; }
    if (tid < Y) {
      unsigned long long m = 0, dm = 0;
      for (int k = s_prefix[0][tid]; k < s_prefix[0][tid + 1]; ++k) if (c->run_log[k] < 64) m |= 1ull << c->run_log[k];
      for (int k = s_prefix[1][tid]; k < s_prefix[1][tid + 1]; ++k) if (c->def_log[k] < 64) { m |= 1ull << c->def_log[k]; dm |= 1ull << c->def_log[k]; }
      reinterpret_cast<unsigned long long*>(snap_base + snap::best_mask)[tid] = m;
      reinterpret_cast<unsigned long long*>(snap_base + snap::bestd_mask)[tid] = dm;
    }
    double* best_w = reinterpret_cast<double*>(snap_base + snap::best_w);
    for (int i = tid; i < Y * NA; i += 1024) { const int y = i / NA, a = i - y * NA; best_w[i] = pol[y * snap::kPolRow + a]; }
    // the whole record of the winning episode (yearly rows, action list, placements) stays with the policy when the
    // episode ran here (eg_fetch_best_run; the run the reference exports is another one, see k_fold_best)
    if (s_owned) {
      const unsigned long long* src = reinterpret_cast<const unsigned long long*>(out_base + (size_t)(c->index - (long long)first_index) * rec::stride);
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(snap_base + snap::best_rec);
      for (int i = tid; i < (int)(rec::stride / 8); i += 1024) dst[i] = src[i];
    }
  }

  // ---- apply_deficit_contrast_learning: the same factor for every episode (it depends on the stall counter only) ----
  if (!improved && st.has_best && st.has_lists) {
    const rm::DeficitContrast dc = s_dc;      // st.stall is the old counter + n_ok here (no improvement)
    if (dc.active) {
      const bool randomize = st.stall > 1200u;
      const int first_draw = s_randomized_main ? kMainDraws : 0;
      for (int i = tid; i < Y * ND; i += 1024) {      // (Y * ND < 1024: one entry per thread, the one requested at the start)
        const int y = i / ND, sl = i - y * ND;
        int occ = 0;
        for (int k = s_off[1][y]; k < s_off[1][y + 1]; ++k) {
          const int a = s_bestd[k];
          const int slot = (a < kFirstOffset && a % 3 == 0) ? c_deficit_slot[a / 3] : (a == kNothing ? 14 : -1);
          occ += slot == sl ? 1 : 0;
        }
        double w = rm::nudge(dw_in, (double)n_ok * (double)occ * dc.ln_boost, (double)dcnt_in * dc.ln_pen);
        if (randomize) w = rm::noise(w, draw(first_draw + i));
        pol[y * snap::kPolRow + snap::kPolDw + sl] = w;
      }
    }
  }
  __syncthreads();
#ifdef EG_STAMPS
  if (tid == 0) dbg_t[5] = wall_clock64();
#endif

  // ---- what eg_upload_snapshot derives: row sums in table order, scalars ----
  // (the rows come to LDS with one load per thread and entry; a thread a year then adds its 61 + 14 entries in table order from
  //  there — summed straight from global memory, 75 dependent-latency loads per thread, this was 10 of the kernel's 22 us)
  __shared__ double s_scratch[2 * 16 * 64];      // [26][76] here; the stalled sampler's per-wave tables further down
  {
    constexpr int kPer = NA + 14 + 1;      // 76: a row's main weights, its first 14 deficit weights, padding
    for (int i = tid; i < Y * (NA + 14); i += 1024) {
      const int y = i / (NA + 14), k = i - y * (NA + 14);
      s_scratch[y * kPer + k] = pol[y * snap::kPolRow + (k < NA ? k : snap::kPolDw + (k - NA))];
    }
    __syncthreads();
    if (tid < Y) {
      const double* r = s_scratch + tid * kPer;
      double a = 0.0, b = 0.0;
      for (int i = 0; i < NA; ++i) a += r[i];
      for (int i = 0; i < 14; ++i) b += r[NA + i];
      double* row = pol + tid * snap::kPolRow;
      row[snap::kPolTotMain] = a; row[snap::kPolTotDeficit] = b;      // the count row is never nudged: its sum stays
    }
  }
  // (derive_state in its four parts, a wave each, beside the row sums of wave 0; the state goes out behind the next barrier)
  if (tid == 64) rm::derive_state_score(st);
  if (tid == 128) rm::derive_state_heur(st);
  if (tid == 192) rm::derive_state_contrast(st);
  if (tid == 256) rm::derive_state_rest(st);
  // the length of the best list goes to a pinned host word: the host plans its launches by it (which replay variant is the long
  // pole, whether a field pool is needed) without ever waiting for the device
  // (only when the list has changed — an improvement —: a store to host memory is a PCIe write the kernel's end waits for)
  if (tid == 65 && list_len_out && s_improved != 0) {
    const uint32_t len = st.has_lists ? (uint32_t)s_prefix[0][Y] : 0u;
    __hip_atomic_store(list_len_out, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // this rank's statistics buffer is ready for the next batch's epilogue (when it is also `packets`, every read of it
  // happened before the barriers above)
  __syncthreads();
  if (tid == 64) *gstate = st;
#ifdef EG_STAMPS
  if (tid == 0) dbg_t[6] = wall_clock64();
#endif
  for (int i = tid; i < EG_STATS_LEN; i += 1024) zero_stats[i] = 0;
  // the stalled sampler's tables of the rows as they are now (k_stalled_tables's work: a launch of its own — 5 us and a dependency gap
  // behind every update, for something that only happens beyond 500 iterations without improvement — until round 3): a wave a year
  if (st.stall > 500u) {
    static_assert(Y * (NA + 15) <= 2 * 16 * 64, "one LDS buffer serves the row sums and the stalled tables");
    double* s_sw = s_scratch + (tid >> 6) * 64; double* s_ss = s_scratch + 16 * 64 + (tid >> 6) * 64;      // (the barrier above is behind the row sums)
    for (int y = tid >> 6; y < Y; y += 16) stalled_tables_year(snap_base, y, tid & 63, st.stall, s_sw, s_ss);
  }
#ifdef EG_STAMPS
  __syncthreads();      // the unused statistics slots 4..7 carry the phase durations out (after the zeroing above)
  if (tid == 0) {
    const unsigned long long t_end = wall_clock64();
    zero_stats[4] = (long long)(dbg_t[2] - dbg_t[0]);      // (best pick,) state, winner, noise key, noise blocks
    zero_stats[5] = (long long)(dbg_t[4] - dbg_t[2]);      // contrast step on the main table + best-strategy bookkeeping
    zero_stats[6] = (long long)(dbg_t[5] - dbg_t[4]);      // list copies / deficit contrast
    zero_stats[7] = (long long)(t_end - dbg_t[5]);         // row sums, derive_state, zeroing
  }
#endif
}
