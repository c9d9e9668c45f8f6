// eg_pick.h — the pick that ends a round of a plan search (namespace refine), whatever the rule: pick_segment, the body of
// many::k_refine_pick_many (eg_refine_many.h) and of repair::k_repair_pick_many (eg_repair.h), and wave_best, what it reduces with.
// Included by eg_rollout.hip (eg_rollout.o only) behind eg_plan_edits.h and before eg_refine_many.h.
//
// A launch holds the variants of its plans back to back: SEGMENT s is the variants [first_s, first_s + n_s) of one plan, whose base
// block is block slot_s of a buffer of base blocks; variant 0 of a segment is the base itself.  On the null stream behind the launch's
// rollout grids, workgroup s
//   reads    status and metrics of ITS variants straight from the records, a thread a variant, striding by the workgroup's width when
//            there are more variants than threads — the trip count is the same for every thread; no record outside its segment;
//   asks     the rule whether variant j is a CANDIDATE and for its KEY; thread 0 keeps what it read of the base in registers and alone
//            writes the base's key to LDS, in its first trip (initialised to "no candidate" before the loop);
//   counts   the variants that are no candidates and the ones the rule counts besides, a ballot each per trip;
//   reduces  the best key per thread, per wave (wave_best) and across the sixteen waves through ONE LDS exchange that every thread
//            folds for itself;
//   asks     the rule for the winner, given the best key and the base's; -1 when the base is no candidate; clamped into the segment
//            (for a record that lies);
//   writes   entry s once, from thread 0: winner, n_failed, the winner's packed edit and metrics, the list totals of its block, base_ok
//            and n — and what the rule adds; every other byte of the entry type zero;
//   copies   the winner's plan block over base block slot_s when winner > 0 — 552 16-byte vector stores, one per thread — so that the
//            next round's writers find the plan's base where the host uploaded it.
// A rule is a struct with
//   Key, Entry                         its key and entry types; an Entry has the common fields above under these names
//   judge(x, w, j, key) -> bool        is variant j (record w of the launch, read into x) a candidate?  sets its key either way
//   counts(key) -> bool                does a candidate with this key go into the rule's own counter?
//   winner(best, base) -> int          the winner's index, the base being a candidate
//   fill(e, best, base, x0, first, w, counted)      the rest of the entry; e.winner and e.base_ok are set, x0 is the base as read
// and a Key is a plain struct that begins with kWords 32-bit words of payload and ends them with the variant's index j, with
//   none()                             the key of "no candidate": it ranks before nothing, j == kNoIndex
//   before(o) -> bool                  a strict order; a.before(a) is false
// Settled one way for every rule: an EMPTY segment (n == 0 after the clamp, or no base blocks; no host launch describes one — the
// search loop builds none, the hooks refuse them, the launchers return at zero segments) runs no trip, passes the barrier with every
// thread, writes a whole entry — winner -1, all else zero — and copies nothing; no store to global memory happens inside the trip loop;
// the base pointer is clamped once, at the copy.  Every index read from memory or computed from one is clamped.  No scratch memory, no
// atomics; LDS holds the exchange alone.
#pragma once

namespace refine {

constexpr int kThreads = 1024, kWaves = kThreads / kWave;
constexpr int kNoIndex = 0x7FFFFFFF;
static_assert(snap::kPlanStride % 16 == 0 && snap::kPlanStride / 16 <= (size_t)kThreads, "a 16-byte store per thread copies a plan block");

// what the host uploads per segment of a launch
struct Segment { uint32_t first, count, slot, pad; };
static_assert(sizeof(Segment) == 16, "segment table entry");

// what the body reads of a variant's record, and what it comes to under the call's rank mode
struct Variant { double m[4], score; int32_t status; };

// the best key of the wave, in every lane.  The combine is idempotent, so a lane without a DPP source combines with itself.
template <class Key>
__device__ __forceinline__ void wave_best(Key& k) {
  static_assert(sizeof(Key) >= Key::kWords * sizeof(int), "a key is moved as its 32-bit words");
#define EG_DPP_BEST_STEP(ctrl, row_mask, bank_mask)                                                        \
  {                                                                                                         \
    int w[Key::kWords];                                                                                     \
    __builtin_memcpy(w, &k, sizeof w);                                                                      \
    _Pragma("unroll") for (int i = 0; i < Key::kWords; ++i) w[i] = __builtin_amdgcn_update_dpp(w[i], w[i], ctrl, row_mask, bank_mask, false); \
    Key o = k;                                                                                              \
    __builtin_memcpy(&o, w, sizeof w);                                                                      \
    if (o.before(k)) k = o;                                                                                 \
  }
  EG_DPP_BEST_STEP(0x111, 0xf, 0xf)   // row_shr:1
  EG_DPP_BEST_STEP(0x112, 0xf, 0xf)   // row_shr:2
  EG_DPP_BEST_STEP(0x113, 0xf, 0xf)   // row_shr:3
  EG_DPP_BEST_STEP(0x114, 0xf, 0xe)   // row_shr:4 bank_mask:0xe
  EG_DPP_BEST_STEP(0x118, 0xf, 0xc)   // row_shr:8 bank_mask:0xc
  EG_DPP_BEST_STEP(0x142, 0xa, 0xf)   // row_bcast:15 row_mask:0xa
  EG_DPP_BEST_STEP(0x143, 0xc, 0xf)   // row_bcast:31 row_mask:0xc
#undef EG_DPP_BEST_STEP
  int w[Key::kWords];
  __builtin_memcpy(w, &k, sizeof w);
#pragma unroll
  for (int i = 0; i < Key::kWords; ++i) w[i] = __builtin_amdgcn_readlane(w[i], 63);
  __builtin_memcpy(&k, w, sizeof w);
}

// workgroup s: segment s of the launch's n_total variants, picked by `rule`
template <class Rule>
__device__ __forceinline__ void pick_segment(const Rule& rule, const DevOut& O, const Segment* __restrict__ segs, uint32_t n_total, int mode,
                                             const uint2* __restrict__ edits, const uint8_t* __restrict__ pool, uint8_t* __restrict__ bases, uint32_t n_bases,
                                             uint8_t* __restrict__ entries) {
  using Key = typename Rule::Key;
  using Entry = typename Rule::Entry;
  __shared__ Key s_best[kWaves], s_base;
  __shared__ int s_fail[kWaves], s_counted[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const Segment sg = segs[blockIdx.x];
  // the segment inside the launch (uniform in the workgroup); an empty one runs no trip and leaves no candidate
  const uint32_t first = sg.first < n_total ? sg.first : n_total;
  const uint32_t n = n_bases == 0u ? 0u : (sg.count < n_total - first ? sg.count : n_total - first);
  Key best = Key::none();      // (variant indices relative to the segment)
  int fails = 0, counted = 0;
  Variant x0{};                // (thread 0 keeps the base as it read it)
  if (tid == 0) s_base = Key::none();      // (thread 0 alone writes it again, in its first trip)
  for (uint32_t j0 = 0; j0 < n; j0 += (uint32_t)kThreads) {      // (uniform: the ballots below want every lane)
    const uint32_t j = j0 + (uint32_t)tid;
    bool cand = false;
    Key key = Key::none();
    if (j < n) {
      const double* m = O.metrics(first + j);
      Variant x{{m[0], m[1], m[2], m[3]}, 0.0, *O.status(first + j)};
      x.score = rm::rank_score(x.m, mode);
      cand = rule.judge(x, first + j, (int)j, key);
      if (j == 0u) {
        x0 = x;
        if (cand) s_base = key;
      }
    }
    fails += __popcll(__ballot(j < n && !cand));
    counted += __popcll(__ballot(cand && rule.counts(key)));
    if (cand && key.before(best)) best = key;
  }
  wave_best(best);
  if (lane == 0) { s_best[wave] = best; s_fail[wave] = fails; s_counted[wave] = counted; }
  __syncthreads();
  best = Key::none(); fails = 0; counted = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const Key o = s_best[w];
    if (o.before(best)) best = o;
    fails += s_fail[w]; counted += s_counted[w];
  }
  const Key base = s_base;
  const bool base_ok = base.j != kNoIndex;
  int winner = -1;
  if (base_ok) {      // (the clamp is for a record that lies)
    winner = rule.winner(best, base);
    winner = winner < 0 ? 0 : (winner >= (int)n ? (int)n - 1 : winner);
  }
  const uint32_t w = first + (winner < 0 ? 0u : (uint32_t)winner);      // the winner among the launch's variants
  const uint8_t* blk = pool + (size_t)w * snap::kPlanStride;
  if (tid == 0) {
    Entry e{};
    e.winner = winner;
    if (n != 0u) {
      const uint2 ed = edits[w];
      const double* m = O.metrics(w);
      e.n_failed = fails;
      e.edit[0] = ed.x; e.edit[1] = ed.y;
#pragma unroll
      for (int i = 0; i < 4; ++i) e.metrics[i] = m[i];
      e.off26 = reinterpret_cast<const int32_t*>(blk + pblock::kOffOff)[EG_YEARS];
      e.offd26 = reinterpret_cast<const int32_t*>(blk + pblock::kOffDOff)[EG_YEARS];
      e.base_ok = base_ok ? 1 : 0; e.n = (int32_t)n;
      rule.fill(e, best, base, x0, first, w, counted);
    }
    *reinterpret_cast<Entry*>(entries + (size_t)blockIdx.x * kRefineEntryStride) = e;
  }
  if (winner > 0 && tid < (int)(snap::kPlanStride / 16)) {
    uint8_t* dst = bases + (size_t)(sg.slot < n_bases ? sg.slot : n_bases - 1u) * snap::kPlanStride;
    reinterpret_cast<uint4*>(dst)[tid] = reinterpret_cast<const uint4*>(blk)[tid];
  }
}

}  // namespace refine
