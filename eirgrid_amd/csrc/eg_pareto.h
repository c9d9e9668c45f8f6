// eg_pareto.h — the Pareto archive of a run's outcomes (include/eirgrid_hip.h eg_pareto_track), folded behind a batch on the null stream
// where the best_result and top-K folds run.  Included by eg_rollout.hip (eg_rollout.o only) behind eg_topk.h.
//
// Five launches, none of which touches a record of the batch except to read it.  In every comparison a point is ORIENTED: opinion and
// reliability negated, inactive metrics replaced by 0.0, so that "lower or equal everywhere" is "at least as good" and an inactive metric
// is equal in every pair.  Point a BEATS point b when a <= b in every coordinate and (a != b somewhere, or a's global index is lower, or
// the indices are equal and a stands earlier in the list): a dominates b, or is the same point with the better claim to represent it.
//   1. k_pareto_filter    one thread per episode, the held points as a broadcast table in LDS: an episode that is invalid, or that a
//                         held point beats, ends here — in the steady state almost every one.  A flag per episode, a count per block.
//   2. k_pareto_compact   the LIST: the held entries, then the survivors compacted in index order with their rank scores.
//   3. k_pareto_dominate  list entry i against every entry j, tile by tile through LDS, a thread per i, the tiles dealt to kSplit blocks:
//                         beaten entries are marked dead.  What stays alive is front(held u batch): beats is transitive, so it does not
//                         matter that a dead j still kills.
//   4. k_pareto_rank      only when more than cap entries are alive: every alive entry's place by rank score (descending, ties to the lower
//                         index), counted the same way.  The capacity rule "keep score" (ParetoState::pad == 0).
//   4'. k_pareto_spread   in k_pareto_rank's place under the capacity rule "keep spread" (ParetoState::pad == kParetoKeepSpread), again only
//                         when more than cap entries are alive: greedy farthest-point selection on the normalised front, one workgroup,
//                         cap rounds of "update a minimum, take an arg-max".  The rank it leaves is the round an entry was picked in.
//   5. k_pareto_finalize  the alive entries of rank < cap (at most cap) gathered, sorted by global index, given slots — held entries keep
//                         theirs, new ones take the lowest free — and written to the state; the records of new entries copied, a
//                         block per record.  Every block derives the same entries and slots; block 0 alone writes the state.
// Nothing between the batch and the final front is sized by cap: the list holds n + EG_PARETO_MAX entries, an antichain batch keeps
// them all alive until the one truncation in step 4.  Why that matters: front(A u B) = front(front(A) u front(B)), so fronts of parts
// compose exactly — but a part's front cut to its cap best-scoring points may have lost the one point that beats a high-scoring point of
// another part, and the merge would then keep a dominated point.
#pragma once

namespace pareto {

constexpr int kBlock = 256;      // threads per workgroup of every kernel here = episodes per chunk = list entries per tile
constexpr int kSplit = 4;        // blocks that share the tiles of one i-range (k_pareto_dominate, k_pareto_rank)
constexpr int kCopyBlocks = 32;  // workgroups of k_pareto_finalize
static_assert(kBlock == (int)kParetoChunk && EG_PARETO_MAX <= kBlock, "a held entry per thread");

__device__ __forceinline__ void oriented(const double* m, int mask, double v[4]) {
  v[0] = (mask & 1) ? m[0] : 0.0; v[1] = (mask & 2) ? -m[1] : 0.0; v[2] = (mask & 4) ? m[2] : 0.0; v[3] = (mask & 8) ? -m[3] : 0.0;
}
// a (global index ai, earlier in the list when `a_first`) against b
__device__ __forceinline__ bool beats(const double* a, long long ai, bool a_first, const double* b, long long bi) {
  const bool le = a[0] <= b[0] && a[1] <= b[1] && a[2] <= b[2] && a[3] <= b[3];
  const bool eq = a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
  return le && (!eq || ai < bi || (ai == bi && a_first));
}
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
// the sum of v over the workgroup (kBlock threads), in every thread; `s`: kBlock / kWave + 1 words of LDS
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, kWave);
  __syncthreads();      // (s may still be read from an earlier sum)
  if ((threadIdx.x & (kWave - 1)) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned t = 0;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) t += s[w];
  return t;
}
__device__ __forceinline__ uint32_t list_len(const ParetoWork& W) {
  const uint32_t m = W.head[0], cap = W.cap_n + (uint32_t)EG_PARETO_MAX;
  return m < cap ? m : cap;
}
__device__ __forceinline__ double rank_key(double s) { return s == s ? s : -__builtin_huge_val(); }      // a NaN score ranks last

}  // namespace pareto

__global__ void __launch_bounds__(pareto::kBlock) k_pareto_filter(DevOut O, uint32_t n, unsigned long long first_index, const ParetoState* st, ParetoWork W) {
  __shared__ double s_v[EG_PARETO_MAX][4];
  __shared__ long long s_idx[EG_PARETO_MAX];
  __shared__ unsigned s_sum[pareto::kBlock / kWave + 1];
  const int tid = threadIdx.x;
  const int held = pareto::clampi(st->n_held, 0, EG_PARETO_MAX), mask = st->objectives;
  if (tid < held) { pareto::oriented(st->e[tid].metrics, mask, s_v[tid]); s_idx[tid] = st->e[tid].index; }
  __syncthreads();
  const uint32_t e = blockIdx.x * (uint32_t)pareto::kBlock + (uint32_t)tid;
  bool live = false;
  if (e < n && e < W.cap_n && *O.status(e) == EG_EP_OK) {
    const double* mm = O.metrics(e);
    const double m[4] = {mm[0], mm[1], mm[2], mm[3]};
    if (m[0] == m[0] && m[1] == m[1] && m[2] == m[2] && m[3] == m[3]) {
      double v[4];
      pareto::oriented(m, mask, v);
      const long long idx = (long long)(first_index + e);
      live = true;
      for (int j = 0; j < held && live; ++j) live = !pareto::beats(s_v[j], s_idx[j], true, v, idx);      // (every lane reads the same words)
    }
  }
  if (e < n && e < W.cap_n) W.flag[e] = live ? 1 : 0;
  const unsigned c = pareto::block_sum(live ? 1u : 0u, s_sum);
  if (tid == 0 && blockIdx.x < (W.cap_n + pareto::kBlock - 1u) / pareto::kBlock) W.blk[blockIdx.x] = c;
}

__global__ void __launch_bounds__(pareto::kBlock) k_pareto_compact(DevOut O, uint32_t n, unsigned long long first_index, const ParetoState* st, ParetoWork W) {
  __shared__ unsigned s_sum[pareto::kBlock / kWave + 1];
  __shared__ unsigned s_wave[pareto::kBlock / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int held = pareto::clampi(st->n_held, 0, EG_PARETO_MAX), mode = st->mode;
  unsigned before = 0;
  for (uint32_t b = (uint32_t)tid; b < blockIdx.x; b += (uint32_t)pareto::kBlock) before += W.blk[b];
  before = pareto::block_sum(before, s_sum);
  const uint32_t e = blockIdx.x * (uint32_t)pareto::kBlock + (uint32_t)tid;
  const bool live = e < n && e < W.cap_n && W.flag[e] != 0;
  const unsigned long long b = __ballot(live);
  if (lane == 0) s_wave[wave] = (unsigned)__popcll(b);
  __syncthreads();
  unsigned off = 0, total = 0;
  for (int w = 0; w < pareto::kBlock / kWave; ++w) { const unsigned c = s_wave[w]; off += w < wave ? c : 0u; total += c; }
  const uint32_t cap_list = W.cap_n + (uint32_t)EG_PARETO_MAX;
  if (live) {
    const uint32_t p = (uint32_t)held + before + off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (p < cap_list) {
      const double* mm = O.metrics(e);
      const double m[4] = {mm[0], mm[1], mm[2], mm[3]};
#pragma unroll
      for (int j = 0; j < 4; ++j) W.m[4 * (size_t)p + j] = m[j];
      W.score[p] = rm::rank_score(m, mode);
      W.index[p] = (long long)(first_index + e);
      W.src[p] = -1 - (int32_t)e;
      W.alive[p] = 1; W.rank[p] = 0u;
    }
  }
  if (blockIdx.x == 0 && tid < held) {
    const ParetoEntry& h = st->e[tid];
#pragma unroll
    for (int j = 0; j < 4; ++j) W.m[4 * (size_t)tid + j] = h.metrics[j];
    W.score[tid] = h.score; W.index[tid] = h.index; W.src[tid] = pareto::clampi(h.slot, 0, EG_PARETO_MAX - 1);
    W.alive[tid] = 1; W.rank[tid] = 0u;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) W.head[0] = (uint32_t)held + before + total;
}

__global__ void __launch_bounds__(pareto::kBlock) k_pareto_dominate(const ParetoState* st, ParetoWork W) {
  __shared__ double s_v[pareto::kBlock][4];
  __shared__ long long s_idx[pareto::kBlock];
  const int tid = threadIdx.x;
  const uint32_t M = pareto::list_len(W), i0 = blockIdx.x * (uint32_t)pareto::kBlock;
  if (i0 >= M) return;
  const int mask = st->objectives;
  const uint32_t i = i0 + (uint32_t)tid;
  const bool have = i < M;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  long long idx = 0;
  if (have) { pareto::oriented(W.m + 4 * (size_t)i, mask, v); idx = W.index[i]; }
  bool dead = !have;
  const uint32_t tiles = (M + pareto::kBlock - 1u) / pareto::kBlock;
  for (uint32_t t = blockIdx.y; t < tiles; t += (uint32_t)pareto::kSplit) {
    const uint32_t j0 = t * (uint32_t)pareto::kBlock, j = j0 + (uint32_t)tid;
    if (j < M) { pareto::oriented(W.m + 4 * (size_t)j, mask, s_v[tid]); s_idx[tid] = W.index[j]; }
    __syncthreads();
    const int cnt = (int)(M - j0 < (uint32_t)pareto::kBlock ? M - j0 : (uint32_t)pareto::kBlock);
    for (int q = 0; q < cnt && !dead; ++q) dead = pareto::beats(s_v[q], s_idx[q], j0 + (uint32_t)q < i, v, idx);
    __syncthreads();
  }
  if (have && dead) W.alive[i] = 0;      // (the blocks of an i-range store the same value)
}

__global__ void __launch_bounds__(pareto::kBlock) k_pareto_rank(const ParetoState* st, ParetoWork W) {
  __shared__ double s_key[pareto::kBlock];
  __shared__ long long s_idx[pareto::kBlock];
  __shared__ unsigned char s_alive[pareto::kBlock];
  __shared__ unsigned s_sum[pareto::kBlock / kWave + 1];
  const int tid = threadIdx.x;
  const uint32_t M = pareto::list_len(W), i0 = blockIdx.x * (uint32_t)pareto::kBlock;
  if (i0 >= M) return;
  unsigned c = 0;
  for (uint32_t j = (uint32_t)tid; j < M; j += (uint32_t)pareto::kBlock) c += W.alive[j] ? 1u : 0u;
  const unsigned front = pareto::block_sum(c, s_sum);
  if (front <= (unsigned)pareto::clampi(st->cap, 1, EG_PARETO_MAX)) return;
  const uint32_t i = i0 + (uint32_t)tid;
  const bool mine = i < M && W.alive[i] != 0;
  const double key = mine ? pareto::rank_key(W.score[i]) : 0.0;
  const long long idx = mine ? W.index[i] : 0;
  unsigned ahead = 0;
  const uint32_t tiles = (M + pareto::kBlock - 1u) / pareto::kBlock;
  for (uint32_t t = blockIdx.y; t < tiles; t += (uint32_t)pareto::kSplit) {
    const uint32_t j0 = t * (uint32_t)pareto::kBlock, j = j0 + (uint32_t)tid;
    s_alive[tid] = j < M && W.alive[j] != 0 ? 1 : 0;
    if (j < M) { s_key[tid] = pareto::rank_key(W.score[j]); s_idx[tid] = W.index[j]; }
    __syncthreads();
    const int cnt = (int)(M - j0 < (uint32_t)pareto::kBlock ? M - j0 : (uint32_t)pareto::kBlock);
    if (mine)
      for (int q = 0; q < cnt; ++q) {
        const bool first = s_key[q] > key || (s_key[q] == key && (s_idx[q] < idx || (s_idx[q] == idx && j0 + (uint32_t)q < i)));
        ahead += (s_alive[q] && first) ? 1u : 0u;
      }
    __syncthreads();
  }
  if (mine && ahead) atomicAdd(&W.rank[i], ahead);
}

// ---- the capacity rule "keep spread" (include/eirgrid_hip.h EG_PARETO_KEEP_SPREAD) ---------------------------------------------------
// Farthest-point selection among the alive entries A of the list.  u_i: entry i's oriented coordinates, each normalised to [0, 1] over
// A ((v - lo) / (hi - lo); 0.0 where hi - lo is not a finite number > 0).  d2(i, j) = ((e0*e0 + e1*e1) + e2*e2) + e3*e3, e = u_i - u_j,
// every operation rounded on its own (the file is built with -ffp-contract=off).  s_0 is the first entry in the order of preference of
// k_pareto_rank; then cap - 1 times: the entry not yet picked whose smallest d2 to a picked one (`mind`) is largest, ties by the order
// of preference.  W.rank[s_r] = r, every other alive entry's rank is ~0u.
// One workgroup.  The c-th alive entry (its place in the list: W.pos[c]) belongs to thread c % kSpreadBlock, which keeps its first
// entry in registers and the others' u and mind in W.u / W.mind; a round is every thread's pass over its entries (min with the distance
// to the last pick, the best of them), a wave-level arg-max, a Pick per wave in LDS, ONE barrier (the Picks alternate between two
// rows), and the same arg-max over the waves' Picks in every wave: the pick's coordinates come out of LDS with it.  The arg-max
// reduces one key at a time over the lanes still tied (wave_first) on the DPP path; the picks' places are kept in LDS and their ranks
// written behind the last round.
namespace pareto {

constexpr int kSpreadBlock = 1024;
constexpr int kSpreadWaves = kSpreadBlock / kWave;
static_assert(kSpreadWaves <= kWave && (kSpreadBlock & (kSpreadBlock - 1)) == 0, "the waves' picks are reduced by one wave, a lane each; an entry's owner is c & (kSpreadBlock - 1)");

struct Cand { double d, key; long long idx; uint32_t pos, c; };      // d: mind (< 0: no candidate); c: the entry is the c-th alive one
struct Pick { Cand b; double u[4]; };
__device__ __forceinline__ bool before(const Cand& a, const Cand& b) {
  return a.d > b.d || (a.d == b.d && (a.key > b.key || (a.key == b.key && (a.idx < b.idx || (a.idx == b.idx && a.pos < b.pos)))));
}
__device__ __forceinline__ double dist2(const double* a, const double* b) {
  const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2], e3 = a[3] - b[3];
  return ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
}
// Wave-level reductions of a 64-bit value on the DPP path (no LDS, a few cycles a step where a ds_bpermute shuffle costs its LDS round
// trip; a round of k_pareto_spread is a chain of them).  dpp64<ctrl, rows>(x): lane l's copy of x from the lane the control names,
// in the rows of the mask; a lane without a source, or outside the mask, keeps its own x — so op(x, dpp64(x)) leaves it unchanged.
// The steps: row_shr 1, 2, 4, 8 make lane 15 of every row of 16 the row's result; row_bcast:15 carries it into the next row (rows 1, 3),
// row_bcast:31 lane 31's into rows 2 and 3: lane 63 holds the wave's result, read back as a scalar.
template <int kCtrl, int kRows> __device__ __forceinline__ long long dpp64(long long x) {
  const int lo = __builtin_amdgcn_update_dpp((int)x, (int)x, kCtrl, kRows, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(x >> 32), (int)(x >> 32), kCtrl, kRows, 0xf, false);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
template <int kCtrl, int kRows> __device__ __forceinline__ double dpp64(double x) { return __longlong_as_double(dpp64<kCtrl, kRows>(__double_as_longlong(x))); }
__device__ __forceinline__ long long last_lane(long long x) {
  const int lo = __builtin_amdgcn_readlane((int)x, kWave - 1), hi = __builtin_amdgcn_readlane((int)(x >> 32), kWave - 1);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double last_lane(double x) { return __longlong_as_double(last_lane(__double_as_longlong(x))); }
template <typename T, typename Op> __device__ __forceinline__ T wave_reduce(T x, Op op) {
  x = op(x, dpp64<0x111, 0xf>(x));      // row_shr:1
  x = op(x, dpp64<0x112, 0xf>(x));      // row_shr:2
  x = op(x, dpp64<0x114, 0xf>(x));      // row_shr:4
  x = op(x, dpp64<0x118, 0xf>(x));      // row_shr:8
  x = op(x, dpp64<0x142, 0xa>(x));      // row_bcast:15
  x = op(x, dpp64<0x143, 0xc>(x));      // row_bcast:31
  return last_lane(x);
}
__device__ __forceinline__ double wave_max(double x) { return wave_reduce(x, [](double a, double b) { return b > a ? b : a; }); }
__device__ __forceinline__ double wave_min(double x) { return wave_reduce(x, [](double a, double b) { return b < a ? b : a; }); }
__device__ __forceinline__ long long wave_min(long long x) { return wave_reduce(x, [](long long a, long long b) { return b < a ? b : a; }); }
// The lane whose candidate stands before every other lane's (-1: no lane has one), the same value in every lane.  The lanes still in
// the running are narrowed a key at a time; a key is only reduced while more than one lane is left.
__device__ __forceinline__ int wave_first(const Cand& b) {
  const double d = wave_max(b.d);
  if (d < 0.0) return -1;
  bool in = b.d == d;
  unsigned long long m = __ballot(in);
  if (__popcll(m) > 1) {
    const double key = wave_max(in ? b.key : -__builtin_huge_val());
    in = in && b.key == key;
    m = __ballot(in);
    if (__popcll(m) > 1) {
      const long long idx = wave_min(in ? b.idx : 0x7fffffffffffffffll);
      in = in && b.idx == idx;
      m = __ballot(in);
      if (__popcll(m) > 1) {
        const long long pos = wave_min(in ? (long long)b.pos : 0x7fffffffffffffffll);
        m = __ballot(in && (long long)b.pos == pos);
      }
    }
  }
  return __ffsll((long long)m) - 1;
}

}  // namespace pareto

__global__ void __launch_bounds__(pareto::kSpreadBlock) k_pareto_spread(const ParetoState* st, ParetoWork W) {
  using pareto::Cand; using pareto::Pick; using pareto::kSpreadBlock; using pareto::kSpreadWaves;
  __shared__ Pick s_pick[2][kSpreadWaves];
  __shared__ double s_lo[kSpreadWaves][4], s_hi[kSpreadWaves][4];
  __shared__ unsigned s_cnt[kSpreadWaves];
  __shared__ uint32_t s_sel[EG_PARETO_MAX];      // s_sel[r]: the place in the list of round r's pick
  const uint32_t tid = threadIdx.x;
  const int lane = (int)(tid & (kWave - 1)), wave = (int)(tid >> 6);
  const uint32_t M = pareto::list_len(W);
  const uint32_t cap = (uint32_t)pareto::clampi(st->cap, 1, EG_PARETO_MAX);
  const int mask = st->objectives;
  const double inf = __builtin_huge_val();

  // the alive entries' places, in the order of the list
  uint32_t A = 0;
  for (uint32_t j0 = 0; j0 < M; j0 += (uint32_t)kSpreadBlock) {
    const uint32_t j = j0 + tid;
    const bool live = j < M && W.alive[j] != 0;
    const unsigned long long b = __ballot(live);
    __syncthreads();      // (s_cnt may still be read for the tile before)
    if (lane == 0) s_cnt[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSpreadWaves; ++w) { const unsigned c = s_cnt[w]; off += w < wave ? c : 0u; total += c; }
    if (live) W.pos[A + off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = j;      // (< A + total <= M: inside the list)
    A += total;
  }
  if (A <= cap) return;
  __syncthreads();      // (W.pos: written by other threads of the workgroup)

  // the range of every coordinate over A
  double lo[4] = {inf, inf, inf, inf}, hi[4] = {-inf, -inf, -inf, -inf};
#pragma unroll 1
  for (uint32_t c = tid; c < A; c += (uint32_t)kSpreadBlock) {
    double v[4];
    pareto::oriented(W.m + 4 * (size_t)W.pos[c], mask, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo[k] = v[k] < lo[k] ? v[k] : lo[k]; hi[k] = v[k] > hi[k] ? v[k] : hi[k]; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { lo[k] = pareto::wave_min(lo[k]); hi[k] = pareto::wave_max(hi[k]); }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { s_lo[wave][k] = lo[k]; s_hi[wave][k] = hi[k]; }
  }
  __syncthreads();
  double range[4];
  bool on[4];
#pragma unroll 1
  for (int w = 0; w < kSpreadWaves; ++w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double a = s_lo[w][k], b = s_hi[w][k]; lo[k] = a < lo[k] ? a : lo[k]; hi[k] = b > hi[k] ? b : hi[k]; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    range[k] = hi[k] - lo[k];
    on[k] = range[k] > 0.0 && range[k] < inf;
  }

  // normalised coordinates; mind = +inf, so that round 0 is decided by the order of preference alone and the first min is d2 itself
  Cand mine; mine.d = -1.0; mine.key = 0.0; mine.idx = 0; mine.pos = 0u; mine.c = tid;
  double mu[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (uint32_t c = tid; c < A; c += (uint32_t)kSpreadBlock) {
    const uint32_t pos = W.pos[c];
    double v[4], u[4];
    pareto::oriented(W.m + 4 * (size_t)pos, mask, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = on[k] ? (v[k] - lo[k]) / range[k] : 0.0;
    W.rank[pos] = ~0u;
    if (c == tid) {
#pragma unroll
      for (int k = 0; k < 4; ++k) mu[k] = u[k];
      mine.d = inf; mine.key = pareto::rank_key(W.score[pos]); mine.idx = W.index[pos]; mine.pos = pos;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) W.u[4 * (size_t)c + k] = u[k];
      W.mind[c] = inf;
    }
  }

  double pu[4] = {0.0, 0.0, 0.0, 0.0};      // the last pick's coordinates
  uint32_t done = 0;                        // rounds completed = picks in s_sel
#pragma unroll 1
  for (uint32_t r = 0; r < cap; ++r) {
    if (r > 0 && mine.d >= 0.0) { const double d2 = pareto::dist2(mu, pu); mine.d = d2 < mine.d ? d2 : mine.d; }
    Cand b = mine;
    // (its other entries one at a time; loading four ahead of their stores was measured and is slower: 5.0 against 4.4 ms for 16 384 alive)
#pragma unroll 1
    for (uint32_t c = tid + (uint32_t)kSpreadBlock; c < A; c += (uint32_t)kSpreadBlock) {
      double d = W.mind[c];
      if (d < 0.0) continue;      // picked
      if (r > 0) {
        const double u[4] = {W.u[4 * (size_t)c], W.u[4 * (size_t)c + 1], W.u[4 * (size_t)c + 2], W.u[4 * (size_t)c + 3]};
        const double d2 = pareto::dist2(u, pu);
        if (d2 < d) { d = d2; W.mind[c] = d; }
      }
      if (d >= b.d) {      // (the keys are read only for an entry that may stand first)
        Cand x; x.d = d; x.pos = W.pos[c]; x.c = c; x.key = pareto::rank_key(W.score[x.pos]); x.idx = W.index[x.pos];
        if (pareto::before(x, b)) b = x;
      }
    }
    Pick* row = s_pick[r & 1u];
    const int win = pareto::wave_first(b);
    if (win < 0) { if (lane == 0) row[wave].b.d = -1.0; }
    else if (lane == win) {
      Pick& p = row[wave];
      p.b = b;
#pragma unroll
      for (int k = 0; k < 4; ++k) p.u[k] = b.c == tid ? mu[k] : W.u[4 * (size_t)b.c + k];
    }
    __syncthreads();      // (the only barrier of a round: the next round writes the other row, and nobody passes its barrier before all have read this one)
    Cand x; x.d = -1.0; x.key = 0.0; x.idx = 0; x.pos = 0u; x.c = 0u;
    if (lane < kSpreadWaves) { x.d = row[lane].b.d; if (x.d >= 0.0) x = row[lane].b; }
    const int w = pareto::wave_first(x);      // (the same in every wave: the order is total)
    if (w < 0) break;                         // (never: more than cap entries are alive, so every round has a candidate)
    const Pick& p = row[w];
    const uint32_t pc = p.b.c, ppos = p.b.pos;
    if (pc >= A || ppos >= M) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) pu[k] = p.u[k];
    if (pc == tid) mine.d = -1.0;      // its owner marks the pick
    else if ((pc & (uint32_t)(kSpreadBlock - 1)) == tid) W.mind[pc] = -1.0;
    if (tid == 0) s_sel[r] = ppos;
    done = r + 1u;
  }
  // (the ranks last and in one go: a store to global memory inside a round would be waited for at the round's barrier)
  __syncthreads();
  if (tid < done) W.rank[s_sel[tid]] = tid;
}

namespace pareto {
struct FinalLds {
  ParetoEntry in[EG_PARETO_MAX], out[EG_PARETO_MAX];      // `slot` of a new entry: -1 - its episode of the batch
  uint32_t pos[EG_PARETO_MAX];
  int32_t episode[EG_PARETO_MAX];                          // of out[r]: -1 = held (the record stays where it is)
  unsigned sum[kBlock / kWave + 1];
  int n;
};
}  // namespace pareto

__global__ void __launch_bounds__(pareto::kBlock) k_pareto_finalize(ParetoState* st, ParetoWork W, DevOut O, uint32_t n) {
  __shared__ pareto::FinalLds L;
  const int tid = threadIdx.x;
  const uint32_t M = pareto::list_len(W);
  const int cap = pareto::clampi(st->cap, 1, EG_PARETO_MAX);
  if (tid == 0) L.n = 0;
  unsigned c = 0;
  for (uint32_t j = (uint32_t)tid; j < M; j += (uint32_t)pareto::kBlock) c += W.alive[j] ? 1u : 0u;
  const unsigned front = pareto::block_sum(c, L.sum);      // (its barriers order L.n = 0 before the adds below)
  for (uint32_t j = (uint32_t)tid; j < M; j += (uint32_t)pareto::kBlock) {
    if (!W.alive[j] || (front > (unsigned)cap && W.rank[j] >= (unsigned)cap)) continue;
    const int p = atomicAdd(&L.n, 1);
    if (p >= cap) continue;      // (ranks are distinct: never more than cap)
    ParetoEntry& x = L.in[p];
#pragma unroll
    for (int k = 0; k < 4; ++k) x.metrics[k] = W.m[4 * (size_t)j + k];
    x.score = W.score[j]; x.index = W.index[j]; x.slot = W.src[j]; x.pad = 0;
    L.pos[p] = j;
  }
  __syncthreads();
  const int kept = L.n < cap ? L.n : cap;
  if (tid < kept) {      // ascending global index (then place in the list): the order of the state, whatever order the adds came in
    int r = 0;
    for (int q = 0; q < kept; ++q)
      r += (L.in[q].index < L.in[tid].index || (L.in[q].index == L.in[tid].index && L.pos[q] < L.pos[tid])) ? 1 : 0;
    L.out[r] = L.in[tid];
  }
  __syncthreads();
  if (tid == 0) {      // slots: held entries keep theirs, new ones take the lowest free
    unsigned long long used[EG_PARETO_MAX / 64] = {0ull, 0ull, 0ull, 0ull};
    static_assert(EG_PARETO_MAX == 256, "four words of slots");
    for (int r = 0; r < kept; ++r) {
      const int s = L.out[r].slot;
      L.episode[r] = s < 0 ? -1 - s : -1;
      if (s >= 0) {
        const int sc = s < cap ? s : cap - 1;
        L.out[r].slot = sc;
        if (sc < 64) used[0] |= 1ull << sc; else if (sc < 128) used[1] |= 1ull << (sc - 64); else if (sc < 192) used[2] |= 1ull << (sc - 128); else used[3] |= 1ull << (sc - 192);
      }
    }
    for (int r = 0; r < kept; ++r) {
      if (L.episode[r] < 0) continue;
      int f = -1;
      if (~used[0]) { f = __ffsll((long long)~used[0]) - 1; used[0] |= 1ull << f; }
      else if (~used[1]) { f = __ffsll((long long)~used[1]) - 1; used[1] |= 1ull << f; f += 64; }
      else if (~used[2]) { f = __ffsll((long long)~used[2]) - 1; used[2] |= 1ull << f; f += 128; }
      else if (~used[3]) { f = __ffsll((long long)~used[3]) - 1; used[3] |= 1ull << f; f += 192; }
      L.out[r].slot = f < 0 || f >= cap ? cap - 1 : f;      // (kept <= cap entries and cap slots: a free one below cap exists)
    }
  }
  __syncthreads();
  uint8_t* slots = reinterpret_cast<uint8_t*>(st) + kParetoRecords;
  for (int r = (int)blockIdx.x; r < kept; r += (int)gridDim.x) {
    const int ep = L.episode[r];
    if (ep < 0 || (uint32_t)ep >= n) continue;
    const uint4* src = reinterpret_cast<const uint4*>(O.base + (size_t)ep * rec::stride);
    uint4* dst = reinterpret_cast<uint4*>(slots + (size_t)L.out[r].slot * rec::stride);
    for (int w = tid; w < (int)(rec::stride / 16); w += pareto::kBlock) dst[w] = src[w];
  }
  if (blockIdx.x != 0) return;
  if (tid < kept) st->e[tid] = L.out[tid];
  if (tid == 0) {
    st->n_held = kept;
    if (front > (unsigned)cap) st->n_dropped += (long long)(front - (unsigned)cap);
  }
}
