// eg_topk.h — the top-K archive of distinct scenarios (include/eirgrid_hip.h eg_top_k_track), folded behind a batch on the null
// stream where the best_result fold runs.  Included by eg_rollout.hip (eg_rollout.o only) behind the other non-rollout kernels.
//
// Three launches, none of which touches a record of the batch except to read it:
//   1. k_topk_keys    one wave per episode: the rank score (the statistics epilogue's when it ran, else rm::rank_score of the metrics)
//                     and — only for an episode that can still enter, i.e. beats the archive's k-th entry when the archive is full — the
//                     64-bit key of its action record.  The replay episodes of the best strategy enter every batch, and their action
//                     logs are the longest: spread over one wave each, their keys take one memory round trip, not a workgroup's loop.
//   2. k_topk_select  one workgroup per chunk of kTopKChunk episodes: the chunk's top-k distinct entries (a duplicate is an entry with
//                     the identity of an entry of lower index), compacted in index order so that the loops run over the survivors only.
//   3. k_topk_merge   one workgroup: the held entries plus every chunk's block, again top-k distinct; held records stay in their slots,
//                     the records of new entries are copied into free ones.
// Why per-chunk (and per-rank) top-k lists are enough: take a scenario Z of the final archive and the chunk that holds its earliest
// occurrence.  Every entry ranked above Z inside that chunk (higher score, or the same score and a lower index there) ranks above Z
// globally as well — its earliest global index is at most its index in the chunk — so if Z were not among the chunk's k best distinct
// entries, k distinct scenarios would rank above it and it could not be in the archive.  The same holds for the filter of step 1: an
// entry of the archive that comes from this batch ranks above the held k-th entry.
#pragma once

namespace topk {

constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, kWave);
  return v;
}
__device__ __forceinline__ bool same_bits(const double* a, const double* b) {
  return __double_as_longlong(a[0]) == __double_as_longlong(b[0]) && __double_as_longlong(a[1]) == __double_as_longlong(b[1]) &&
         __double_as_longlong(a[2]) == __double_as_longlong(b[2]) && __double_as_longlong(a[3]) == __double_as_longlong(b[3]);
}

// The key of episode e's action record (one wave, every lane returns it): the byte string n_act[26] (int32, little-endian) ++
// act_log[0 .. A), A = sum n_act, zero-padded to whole 8-byte words w_i; key = sum_i splitmix64(w_i + i * kGolden).  n_act is 104 bytes
// = words 0..12, and rec::n_act / rec::act_log are 8-byte aligned, so word 13 + j is act_log's j-th aligned word.
__device__ unsigned long long episode_key(const DevOut& O, uint32_t e, int lane) {
  static_assert(rec::n_act % 8 == 0 && rec::act_log % 8 == 0 && EG_YEARS * 4 == 13 * 8 && EG_ACT_CAP % 8 == 0, "key layout");
  const unsigned long long* na = reinterpret_cast<const unsigned long long*>(O.n_act(e));
  const unsigned long long w = lane < 13 ? na[lane] : 0ull;
  int a = lane < 13 ? (int)(uint32_t)w + (int)(uint32_t)(w >> 32) : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, kWave);
  const int A = a < 0 ? 0 : (a > EG_ACT_CAP ? EG_ACT_CAP : a);      // (an episode that ended OK never exceeds the capacity)
  unsigned long long h = lane < 13 ? splitmix64(w + (unsigned long long)lane * kGolden) : 0ull;
  const unsigned long long* al = reinterpret_cast<const unsigned long long*>(O.act_log(e));
  const int nw = (A + 7) >> 3;
  for (int j = lane; j < nw; j += kWave) {
    unsigned long long x = al[j];
    const int rem = A - 8 * j;
    if (rem < 8) x &= (1ull << (8 * rem)) - 1ull;      // the padding: bytes behind the log are zero, whatever the record holds there
    h += splitmix64(x + (unsigned long long)(13 + j) * kGolden);
  }
  return wave_sum_u64(h);
}

}  // namespace topk

// 1. four episodes per workgroup of 256, one wave each.  Score -inf: the episode cannot enter (failed, NaN, or not above the k-th) — and so
//    an episode whose rank score IS -inf never enters: only scores above -inf can (include/eirgrid_hip.h, "failures").
__global__ void __launch_bounds__(256) k_topk_keys(DevOut O, uint32_t n, unsigned long long first_index, int mode, int use_list,
                                                   const TopKState* st, double* c_score, unsigned long long* c_key) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (e >= n) return;
  double s = -__builtin_huge_val();
  unsigned long long key = 0ull;
  if (*O.status(e) == EG_EP_OK) {
    const double sc = use_list ? O.score_list[e] : rm::rank_score(O.metrics(e), mode);
    bool pass = sc == sc;
    const int k = st->k;
    if (st->n_held >= k) {      // full: only what ranks above the k-th entry (ties: a lower global index) can still enter
      const double ks = st->e[k - 1].score;
      const long long ki = st->e[k - 1].index;
      pass = sc > ks || (sc == ks && (long long)(first_index + e) < ki);
    }
    if (pass) {      // (uniform in the wave: every lane read the same words)
      s = sc;
      key = topk::episode_key(O, e, lane);
    }
  }
  if (lane == 0) { c_score[e] = s; c_key[e] = key; }
}

// 2. one workgroup per chunk of kTopKChunk consecutive episodes: the candidates compacted in index order, then per candidate
//    (a) duplicate? — an earlier candidate of the chunk with the same score, key and metrics bits (the replay episodes find the
//        chunk's first replay after a few steps), (b) rank among the non-duplicates; ranks below k go to the chunk's block.
__global__ void __launch_bounds__(1024) k_topk_select(DevOut O, uint32_t n, unsigned long long first_index, const double* c_score,
                                                      const unsigned long long* c_key, int k, TopKBlock* blocks) {
  __shared__ double s_score[kTopKChunk];
  __shared__ unsigned long long s_key[kTopKChunk];
  __shared__ double s_m[kTopKChunk][4];
  __shared__ int s_pos[kTopKChunk];
  __shared__ unsigned char s_dup[kTopKChunk];
  __shared__ int s_wave[kTopKChunk / kWave];
  __shared__ int s_count;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const uint32_t i = blockIdx.x * kTopKChunk + (uint32_t)tid;
  const double sc = i < n ? c_score[i] : -__builtin_huge_val();
  const bool cand = i < n && sc > -__builtin_huge_val();
  const unsigned long long b = __ballot(cand);
  if (lane == 0) s_wave[wave] = __popcll(b);
  if (tid == 0) s_count = 0;
  __syncthreads();
  int off = 0, m = 0;
  for (int w = 0; w < (int)(kTopKChunk / kWave); ++w) { const int c = s_wave[w]; off += w < wave ? c : 0; m += c; }
  if (cand) {
    const int p = off + __popcll(b & ((1ull << lane) - 1ull));
    s_score[p] = sc; s_key[p] = c_key[i]; s_pos[p] = tid;
    const double* mm = O.metrics(i);
#pragma unroll
    for (int j = 0; j < 4; ++j) s_m[p][j] = mm[j];
  }
  __syncthreads();
  bool dup = false;
  double my = 0.0;
  if (tid < m) {
    my = s_score[tid];
    const unsigned long long mk = s_key[tid];
    for (int j = 0; j < tid; ++j)      // compacted in index order: j < tid is a lower index
      if (s_score[j] == my && s_key[j] == mk && topk::same_bits(s_m[j], s_m[tid])) { dup = true; break; }
    s_dup[tid] = dup ? 1 : 0;
  }
  __syncthreads();
  if (tid < m && !dup) {
    int rank = 0;
    for (int j = 0; j < m && rank < k; ++j)
      rank += (!s_dup[j] && (s_score[j] > my || (s_score[j] == my && j < tid))) ? 1 : 0;
    if (rank < k) {
      TopKEntry& o = blocks[blockIdx.x].e[rank];
      o.score = my; o.index = (long long)(first_index + blockIdx.x * kTopKChunk + (uint32_t)s_pos[tid]);
#pragma unroll
      for (int j = 0; j < 4; ++j) o.metrics[j] = s_m[tid][j];
      o.key = s_key[tid]; o.slot = -1; o.step = 0u;
      atomicAdd(&s_count, 1);
    }
  }
  __syncthreads();
  if (tid == 0) blocks[blockIdx.x].n = s_count;
}

// 3. one workgroup: the list (held entries first, then the blocks' entries) in LDS, reduced to its top-k distinct whenever the next
//    block would not fit, and at the end.  Ranking: score descending, then global index, then place in the list (held before new: an
//    index folded twice keeps the held entry); duplicate: the same identity as an entry that ranks before it in that order.
namespace topk {
constexpr int kCap = 512;
struct MergeLds {
  double score[kCap]; long long index[kCap]; unsigned long long key[kCap]; double m[kCap][4]; int slot[kCap]; uint32_t step[kCap];
  unsigned char dup[kCap];
  TopKEntry out[EG_TOPK_MAX];
  int n, n_out, fresh[EG_TOPK_MAX];
};
__device__ __forceinline__ void put(MergeLds& L, int p, const TopKEntry& e, int slot, uint32_t step) {
  L.score[p] = e.score; L.index[p] = e.index; L.key[p] = e.key; L.slot[p] = slot; L.step[p] = step;
#pragma unroll
  for (int j = 0; j < 4; ++j) L.m[p][j] = e.metrics[j];
}
__device__ __forceinline__ bool before(const MergeLds& L, int j, int i) {      // does list entry j come before entry i (same score)?
  return L.index[j] < L.index[i] || (L.index[j] == L.index[i] && j < i);
}
__device__ void reduce(MergeLds& L, int k) {
  const int tid = threadIdx.x, m = L.n;
  if (tid == 0) L.n_out = 0;
  bool dup = false;
  if (tid < m) {
    for (int j = 0; j < m; ++j)
      if (j != tid && L.score[j] == L.score[tid] && L.key[j] == L.key[tid] && same_bits(L.m[j], L.m[tid]) && before(L, j, tid)) { dup = true; break; }
    L.dup[tid] = dup ? 1 : 0;
  }
  __syncthreads();
  if (tid < m && !dup) {
    int rank = 0;
    for (int j = 0; j < m && rank < k; ++j)
      rank += (!L.dup[j] && (L.score[j] > L.score[tid] || (L.score[j] == L.score[tid] && before(L, j, tid)))) ? 1 : 0;
    if (rank < k) {
      TopKEntry& o = L.out[rank];
      o.score = L.score[tid]; o.index = L.index[tid]; o.key = L.key[tid]; o.slot = L.slot[tid]; o.step = L.step[tid];
#pragma unroll
      for (int j = 0; j < 4; ++j) o.metrics[j] = L.m[tid][j];
      atomicAdd(&L.n_out, 1);
    }
  }
  __syncthreads();
  const int c = L.n_out;
  if (tid < c) put(L, tid, L.out[tid], L.out[tid].slot, L.out[tid].step);
  if (tid == 0) L.n = c;
  __syncthreads();
}
}  // namespace topk

__global__ void __launch_bounds__(1024) k_topk_merge(TopKState* st, const uint8_t* blocks, int n_blocks, unsigned long long block_stride,
                                                     TopKBlock* pack, int k, DevOut O, unsigned long long own_first, uint32_t own_n, uint32_t step) {
  __shared__ topk::MergeLds L;
  const int tid = threadIdx.x;
  if (st) {
    const int held = st->n_held;
    if (tid < held) put(L, tid, st->e[tid], st->e[tid].slot, st->e[tid].step);
    if (tid == 0) L.n = held;
  } else if (tid == 0) L.n = 0;
  __syncthreads();
  for (int b = 0; b < n_blocks; ++b) {
    const TopKBlock* blk = reinterpret_cast<const TopKBlock*>(blocks + (size_t)b * block_stride);
    int nb = blk->n;
    nb = nb < 0 ? 0 : (nb > k ? k : nb);
    if (L.n + nb > topk::kCap) topk::reduce(L, k);      // (L.n: the same for every thread; after a reduction at most k)
    const int base = L.n;
    if (tid < nb) put(L, base + tid, blk->e[tid], -1, step);
    __syncthreads();
    if (tid == 0) L.n = base + nb;
    __syncthreads();
  }
  topk::reduce(L, k);
  const int c = L.n;
  if (!st) {      // a rank's message: its shard's top-k distinct entries
    if (tid < c) {
      TopKEntry& o = pack->e[tid];
      o.score = L.score[tid]; o.index = L.index[tid]; o.key = L.key[tid]; o.slot = -1; o.step = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.metrics[j] = L.m[tid][j];
    }
    if (tid == 0) pack->n = c;
    return;
  }
  if (tid == 0) {      // slots: held entries keep theirs, new ones take the lowest free (the same choice on every rank of a group)
    unsigned long long used = 0ull;
    for (int r = 0; r < c; ++r) if (L.slot[r] >= 0) used |= 1ull << L.slot[r];
    for (int r = 0; r < c; ++r) {
      L.fresh[r] = L.slot[r] < 0 ? 1 : 0;
      if (L.slot[r] < 0) { const int f = __ffsll((long long)~used) - 1; L.slot[r] = f; used |= 1ull << f; }
    }
  }
  __syncthreads();
  uint8_t* slots = reinterpret_cast<uint8_t*>(st) + kTopKRecords;
  for (int r = 0; r < c; ++r) {
    const long long li = L.index[r] - (long long)own_first;
    if (!L.fresh[r] || li < 0 || li >= (long long)own_n) continue;      // held, or run by another rank
    const uint4* src = reinterpret_cast<const uint4*>(O.base + (size_t)li * rec::stride);
    uint4* dst = reinterpret_cast<uint4*>(slots + (size_t)L.slot[r] * rec::stride);
    for (int w = tid; w < (int)(rec::stride / 16); w += 1024) dst[w] = src[w];
    if (tid == 0) { st->tag_index[L.slot[r]] = L.index[r]; st->tag_step[L.slot[r]] = step; }
  }
  if (tid < c) {
    TopKEntry& o = st->e[tid];
    o.score = L.score[tid]; o.index = L.index[tid]; o.key = L.key[tid]; o.slot = L.slot[tid]; o.step = L.step[tid];
#pragma unroll
    for (int j = 0; j < 4; ++j) o.metrics[j] = L.m[tid][j];
  }
  if (tid == 0) st->n_held = c;
}
