// eg_rollout.hip — CDNA4 (gfx950) kernels of the rollout engine.
//
// One wavefront runs one 2025–2050 episode from start to finish; a batch is a grid of episodes, one workgroup each
// (k_rollout<0>: the episode wave alone; k_rollout<1>, small batches: plus a helper wave, see helper_loop).  Control
// flow of an episode is wave-uniform (every lane carries the same scalar state); the lanes fan out over the 64
// candidates of a chunk of the placement search, the per-generator / per-offset gathers at the start of a year, the
// weight rows (nudges, prefix scans of the samplers) and the ChaCha blocks.  Sums and products that end up in an output
// are folded in the reference's list order and every transcendental is a host-built table (eg_tables.cpp), so device
// code is + - * / compare only and reproduces the CPU oracle bit for bit; chains that only feed a decision (the samplers'
// sum-and-walk) are replaced by a parallel form where that provably gives the same decision (weighted_pick).
// Build: -ffp-contract=off (no FMA); compiled twice — the throughput kernels as an object of their own, see EG_TU_THROUGHPUT
// below and csrc/Makefile.
// The map.  One translation unit; a header is a stretch of it, included where it stands, in this order:
//   (here)                LDS layouts, ChaCha stream, chunked placement search, yearly sums, helper_loop, place_search      both objects
//   eg_field.h            the penalty field of a long replay: place_heavy, place_tiles, place_exact_long                    both
//   (here)                nudges, samplers, statistics epilogue, EpisodeMap; k_rollout; k_episodes, k_heavy_register_budget both; eg_rollout_tp.o
//   eg_rollout_episode.h  the episode: the body of k_rollout and of k_episodes (included twice, EG_EPISODE_UNIFORM false / true)    both; eg_rollout_tp.o
//   eg_replay_script.h    a replay episode's script and yearly rows                                                         both
//   eg_replay_solo.h      k_replay_solo, k_replay_lazy                                                                      eg_rollout_tp.o
//   eg_replay_coop.h      k_replay_coop, k_replay_books, k_replay_broadcast: the replay hoist                               eg_rollout.o
//   eg_topk.h             the top-K archive of distinct scenarios                                                           eg_rollout.o
//   eg_pareto.h           the Pareto archive of a run's outcomes                                                            eg_rollout.o
//   eg_plan_block.h       what the kernels that write plan blocks share                                                     eg_rollout.o
//   eg_plan_edits.h       k_plan_edits                                                                                      eg_rollout.o
//   eg_pick.h             the pick that ends a round of a plan search: wave_best, pick_segment                              eg_rollout.o
//   eg_refine_many.h      k_plan_edits_many, k_refine_pick_many                                                             eg_rollout.o
//   eg_plan_moves.h       k_plan_moves                                                                                      eg_rollout.o
//   eg_plan_crosses.h     k_plan_crosses                                                                                    eg_rollout.o
//   eg_plan_rewrites.h    k_plan_rewrites                                                                                   eg_rollout.o
//   eg_plan_constraints.h k_plan_constraints (and pcons::stage_rows, store_judgment: shared with k_build_constraints)       eg_rollout.o
//   eg_repair.h           k_repair_pick_many                                                                                eg_rollout.o
//   eg_build_constraints.h k_build_constraints                                                                              eg_rollout.o
//   eg_breed.h            k_breed_gather, k_breed_turnover                                                                  eg_rollout.o
//   eg_explore.h          k_explore_turnover                                                                                eg_rollout.o
//   eg_update_kernels.h   k_place .. k_apply_update: the kernels that are not rollouts                                      eg_rollout.o
//   (here)                every launch_*, with k_fold_stats, k_fill_lds, k_occupy, k_rewind                                 as the #ifdef says
// Two measured facts shape the code: (1) in the small-batch kernel a lone wave issues one instruction per turn of its
// SIMD, whatever the instruction — the hot loops are written for instruction count, scalar and wait instructions
// included (chunk_product_latency); (2) gfx950 allocates LDS in 1280-byte granules — the throughput kernel's Smem is
// held at seven of them (room for eighteen episodes per CU; sixteen run: four waves per SIMD at 128 VGPRs), the small-batch kernel
// spends LDS freely (SmemLatency).
//
// Reference (paths relative to /root/reference/aiSimulator/src/):
//   episode        core/simulation.rs:22-317, core/iteration.rs:57-74
//   deficit loop   core/simulation.rs:319-522
//   sampling       ai/learning/weights/sampling.rs:76-443
//   nudges         ai/learning/weights/learning.rs:21-88, deficit.rs:82-135
//   apply_action   core/actions.rs:40-204
//   placement      gpu/metal_location_search.rs:110-176
//   metrics        analysis/metrics_calculation.rs:7-175, ai/metrics/scoring.rs:46-85
//   RNG            rand 0.8.5 StdRng = ChaCha12 behind rand_core BlockRng (Cargo.lock:763-785)
#include <hip/hip_runtime.h>
#include <cstddef>
#include <hip/hip_ext.h>

#include "eg_internal.h"

#define EG_DETPOW_QUAL __device__ __forceinline__
#include "eg_detpow.h"
#define EG_RM __device__ __forceinline__
#include "eg_reduced_math.h"

namespace eg {
namespace {

constexpr int kWave = 64;
constexpr int kD2Max = 144, kD2Stride = 146;   // factor table by squared cell distance: 0..144 (12 km = the largest radius), padded
constexpr int kDrHiPlane = 384;         // Smem::dr, kPlanes: words from an entry's low word to its high word (a multiple of 64: ds_read2st64_b32's stride)
static_assert(kDrHiPlane >= kDrCompact && kDrHiPlane % 64 == 0 && kDrHiPlane / 64 < 256, "the high plane lies behind the low one, a two-address read apart");
constexpr int kCmdYear = 1 << 30;       // helper command: fold next year's starting sums (else: a placement search)
constexpr int kHelperWaves = 1;         // small-batch kernel: waves per episode beyond the episode wave (see helper_loop)
// The episode wave polls an LDS flag for the helper's results (s_sleep 1 = 64 cycles per poll).  The helper's longest job —
// a chunk against 512 generators, or a year's sums over full lists — is a few 10^4 cycles; after 2^20 polls (~30 ms) the
// protocol must have slipped: the episode ends with EG_EP_INTERNAL instead of hanging the GPU.
constexpr int kSpinCap = 1 << 20;
constexpr int kSearchLost = -2;         // place_search: the helper never answered
constexpr double kMinWeight = 0.0001;   // ai/learning/constants.rs:14
constexpr double kMaxWeight = 0.999;    // constants.rs:15
constexpr double kMaxCost = 50000000000.0;   // config/constants.rs:115
constexpr int kBattery = 12, kPeaker = 8;
constexpr int kNothing = 60, kFirstOffset = 45, kFirstOther = 57;

// deficit-table slot -> generator type (core.rs:130-149) and the inverse
__constant__ int c_deficit_type[14] = {8, 7, 12, 11, 9, 0, 1, 4, 10, 5, 2, 3, 13, 14};
__constant__ int c_deficit_slot[15] = {5, 6, 10, 11, 7, 9, -1, 1, 0, 4, 8, 3, 2, 12, 13};
// the same map as an immediate (4 bits per generator type, 15 = none) for loops that cannot afford a constant-memory
// round trip per element: slot of an action index, -1 if the deficit table has no entry for it
__device__ __forceinline__ int deficit_slot_of(int action) {
  constexpr unsigned long long kNibbles = 0xDC238401F97BA65ull;      // type 0 in the low nibble: 5, 6, 10, 11, 7, 9, 15, 1, 0, 4, 8, 3, 2, 12, 13
  if (action == 60) return 14;                                        // DoNothing
  if (action >= 45 || action % 3 != 0) return -1;
  const int s = (int)((kNibbles >> (4 * (action / 3))) & 15ull);
  return s == 15 ? -1 : s;
}

struct __align__(16) Smem {
  uint32_t dr[2 * kDrCompact];            // d/R by squared cell distance, class k at entries off_k .. off_k + cap_k (tab::dr_meta): only up to its own
                                      // radius — 1.0 at cap_k, where every larger distance is capped (2.9 instead of 7 KB: with 128 VGPRs that is
                                      // what lets a fourth wave share the SIMD).  In one of two layouts, a kernel's choice (kPlanes):
                                      //  * two planes of 32-bit words (the lean grid, the short-replay variant, k_place — bound by vector issue):
                                      //    entry i's low word at word i, its high word at kDrHiPlane + i, so that an entry's byte address is
                                      //    base + 4 i — what the dot product of a doubled coordinate difference with itself yields (factor_at) —
                                      //    and one two-address read, the second kDrHiPlane words on, returns the double.  The high plane's last
                                      //    32 words lie in `park`, which these kernels do not use: the block is the size it was;
                                      //  * kDrCompact doubles (the long-replay kernels, a lone wave bound by latency: reading a factor as two
                                      //    words measured slower there than the 64-bit read, profiles/r18_ab_notes.log)
  double park[18];                    // long-replay variant: the year's aggregates while the field code runs (see k_rollout).  kPlanes (never the long-replay
                                      // variant): the high plane's last kDrHiPlane - kDrCompact words — it starts kDrHiPlane words into dr and ends in here
  int gstage[2][kWave + 8];           // per wave: (gi, gj) — kPlanes: doubled — as two int16 of the 64 generators being folded (read back four at a time);
                                      // the tail stays at the off-grid padding value: the pipeline reads up to three groups ahead
  double scaled[64];                  // stalled sampler: weights^p in sorted order
  double type_out[16];                // per generator type: output of an operational new plant
  double type_co2[16];                //                     CO2
  int type_info[16];                  //                     variant | radius class << 4 | reach << 8 | output class << 12
  double yend[6];                     // last year's end-of-year sums: capital (generators, offsets), CO2, output classes
  double ystate[4];                   // net CO2 / opinion / balance / cost at the start of the year (success bonus of the repair loop)
  double acc[8];                      // once-a-year accumulators kept out of registers: total cost / credit / sales, last row
  double pol[snap::kPolRow];          // this year's policy row block (layout: eg_internal.h, namespace snap)
  uint32_t rng[64];                   // ChaCha12 output buffer: four blocks
  uint32_t rng_key[8];                // ChaCha12 key of the episode stream
  unsigned long long rng_counter;     // next block counter
  uint16_t gcell[kLdsGens];           // cell | type << 12      (the first kLdsGens generators / offsets of the episode: all of them,
  uint16_t opack[kLdsGens];           // type | year << 4 | mult << 9     except in the long-replay variant, whose lists go on in
  uint8_t gbm[kLdsGens];              // build-year index | mult << 5     the episode's record in HBM — ListTail)
  uint8_t ydef[192];                  // [0,128) this year's deficit actions (success bonus, simulation.rs:505-519);
                                      // [128,192) sort permutation of the stalled sampler
  // helper waves (small-batch kernel only): search command (double-buffered by sequence parity), results, flags
  int cmd[2][2];                      // {year | variant << 8 | radius class << 12 (or -1: exit), generators in the list}
  uint32_t hflag[2];                  // sequence number of the search whose result is in hres[h]
  uint32_t yflag; int ysum_opcnt;     // year-start sums folded by the helper wave (sequence number, count)
  double ysum[8];                     //   gcost, optot, offs, ocost, co2, tg, ig, sg
  struct { double score, m03; int cell, pad; } hres[2];
#ifdef EG_STAMPS
  unsigned long long hdbg[2][4];
#endif
};
// gfx950 hands out LDS in granules of 1280 bytes (160 KB / 128): seven granules per episode leave room for the sixteen workgroups per
// CU that four waves per SIMD (128 VGPRs) allow.  (Ten granules and three waves until the factor table was compacted: 1.305 -> 1.194 ms
// at 16 384 episodes.)
static_assert(offsetof(Smem, park) == sizeof(uint32_t) * 2 * kDrCompact && sizeof(double) * 18 >= sizeof(uint32_t) * (kDrHiPlane - kDrCompact), "the high plane's end lies in park");
#ifndef EG_STAMPS
static_assert(sizeof(Smem) <= 7 * 1280, "sixteen episodes per CU");
#endif

// One instance per workgroup (= per episode).  File scope so that non-inlined helpers address it as LDS.
__shared__ Smem sm;
// Extra LDS of the small-batch kernel only (it is not referenced by the throughput kernel, so it costs that one nothing).
struct __align__(16) SmemLatency {
  int gpk[kLdsGens + 16];                           // (4 gi, 4 gj) as two int16 per generator of the episode; padding beyond the list
  double dr16[kRadiusClasses * kD2Stride * 2];      // the factor table at a stride of 16 bytes (see chunk_product_latency)
};
__shared__ SmemLatency sl;
constexpr int kGenPad4 = (int)0xE000E000;           // a generator far off the grid, in the x4 coordinates
#define SM_W (sm.pol)                      // main weights [61]
#define SM_DW (sm.pol + snap::kPolDw)      // deficit weights [15]
#define SM_CW (sm.pol + snap::kPolCw)      // action-count weights [21]

// A workgroup is ONE wavefront, and a wave's LDS operations execute in program order, so data written to LDS by one
// lane is visible to every lane's later reads without waiting; what is needed is only that the compiler keeps the
// program order of the LDS accesses.  Unlike wave_sync() this does not drain vmcnt, so global loads requested ahead
// of time and the episode's output stores stay in flight across it.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct Rng {      // register part of the stream state; key / counter / buffer live in LDS
  int index;
  unsigned int words;
};
struct Totals {   // (the sums of the rows themselves are taken inside weighted_pick)
  bool scaled_valid;   // the stalled sampler's sorted / powered table in LDS matches the weight row
};

struct Agg {   // aggregates of the map at the current point of the year (map_handler.rs:819-965)
  double co2, tg, ig, sg, optot, gcost, ocost, gcost_prev, ocost_prev, offs, usage;
  int opcnt;
};
struct State { double net, opinion, balance, cost; };   // ActionResult, simulation_metrics.rs:13-18

// A condition that is the same in every lane, made known to the compiler as such (a scalar branch instead of an
// exec-masked region with its save / restore instructions).
#define EG_UNI(c) (__builtin_amdgcn_ballot_w64(c) != 0ull)
// ... and a value that is: under kUniform (eg_rollout_episode.h, k_episodes) the first lane's, in a scalar register; otherwise as it comes.  Only where every
// lane holds the same value and the wave's lanes are all active or all masked alike.
template <bool kUniform> __device__ __forceinline__ int uni(int v) { if constexpr (kUniform) return __builtin_amdgcn_readfirstlane(v); else return v; }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double dabs(double a) { return a < 0.0 ? -a : a; }
// v_max_f64 / v_min_f64 as such: from `a > b ? a : b` the compiler makes a compare and two selects (it may not assume that there are no
// NaNs and that the sign of a zero does not matter).  Only where neither can occur: weights and scores (positive, finite), and
// max(|x|, 1.0) (at least 1.0 whatever the sign of a zero x).
__device__ __forceinline__ double vmax64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double vmin64(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double vmax64_u(double a, double uniform_b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(uniform_b)); return r; }
__device__ __forceinline__ double vmin64_u(double a, double uniform_b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(uniform_b)); return r; }
__device__ __forceinline__ double max_abs_one(double a) { double r; asm("v_max_f64 %0, |%1|, 1.0" : "=v"(r) : "v"(a)); return r; }      // max(|a|, 1.0)
__device__ __forceinline__ uint32_t rotl32(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

#define EG_QR(a, b, c, d)                                                         \
  a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12);           \
  a += b; d ^= a; d = rotl32(d, 8);  c += d; b ^= c; b = rotl32(b, 7);

// Four consecutive ChaCha12 blocks (rand_chacha fills 64 words per refill).  Not inlined: the episode code draws from ~10
// places.  Sixteen lanes work on it: lane 4 b + c holds column c of block b — a word of each of the state's four rows — so a column
// round is one quarter round per lane, and a diagonal round is the same quarter round after rotating rows 1, 2, 3 by one, two,
// three lanes inside the quad (DPP quad_perm) and back: 12 + 6 instructions per lane and half-round pair... 180 for the twelve
// rounds, where one lane per block (four lanes, sixteen words each) took 1 200 — a refill every 32 draws, 2.5 per episode.
__device__ __forceinline__ uint32_t quad_rot(uint32_t v, int ctrl_is_1230_2301_3012) {
  // lane i of a quad takes the value of lane (i + k) % 4: quad_perm [1,2,3,0] = 0x39, [2,3,0,1] = 0x4E, [3,0,1,2] = 0x93
  if (ctrl_is_1230_2301_3012 == 1) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x39, 0xf, 0xf, false);
  if (ctrl_is_1230_2301_3012 == 2) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false);
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x93, 0xf, 0xf, false);
}
__device__ __noinline__ void rng_refill(int lane) {
  wave_sync();
  if (lane < 16) {
    const int blk = lane >> 2, col = lane & 3;
    const unsigned long long counter = sm.rng_counter + (unsigned long long)blk;
    const uint32_t a0 = col == 0 ? 0x61707865u : (col == 1 ? 0x3320646eu : (col == 2 ? 0x79622d32u : 0x6b206574u));
    const uint32_t b0 = sm.rng_key[col], c0 = sm.rng_key[4 + col];
    const uint32_t d0 = col == 0 ? (uint32_t)counter : (col == 1 ? (uint32_t)(counter >> 32) : 0u);
    uint32_t a = a0, bq = b0, c = c0, d = d0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      EG_QR(a, bq, c, d)                                                    // columns
      bq = quad_rot(bq, 1); c = quad_rot(c, 2); d = quad_rot(d, 3);        // row k moves k lanes: the diagonals line up as columns
      EG_QR(a, bq, c, d)                                                    // diagonals
      bq = quad_rot(bq, 3); c = quad_rot(c, 2); d = quad_rot(d, 1);        // ... and back
    }
    uint32_t* out = sm.rng + 16 * blk + col;
    out[0] = a + a0; out[4] = bq + b0; out[8] = c + c0; out[12] = d + d0;
  }
  wave_sync();
  if (lane == 0) sm.rng_counter += 4ull;
  wave_sync();
}

__device__ void rng_seed(Rng& r, unsigned long long state, int lane) {   // rand_core 0.6.4 seed_from_u64
  const unsigned long long MUL = 6364136223846793005ull, INC = 11634580027462260723ull;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    state = state * MUL + INC;
    uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
    uint32_t rot = (uint32_t)(state >> 59);
    if (lane == 0) sm.rng_key[i] = (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
  }
  if (lane == 0) sm.rng_counter = 0ull;
  wave_sync();
  r.index = 64; r.words = 0;
}
__device__ __forceinline__ unsigned long long rng_u64(Rng& r, int lane) {   // BlockRng::next_u64
  r.words += 1;
  unsigned long long lo;
  if (r.index >= 63) {                      // one word left (63) or none (>= 64): refill once
    const bool straddle = r.index == 63;
    const uint32_t tail = sm.rng[63];
    rng_refill(lane);
    if (straddle) { r.index = 1; return ((unsigned long long)sm.rng[0] << 32) | tail; }
    r.index = 0;
  }
  lo = sm.rng[r.index];
  const unsigned long long hi = sm.rng[r.index + 1];
  r.index += 2;
  return (hi << 32) | lo;
}
__device__ __forceinline__ uint32_t rng_u32(Rng& r, int lane) {   // BlockRng::next_u32
  r.words += 1;
  if (r.index >= 64) { rng_refill(lane); r.index = 0; }
  const uint32_t v = sm.rng[r.index];
  r.index += 1;
  return v;
}
__device__ __forceinline__ double rng_f64(Rng& r, int lane) {   // Standard: 53 bits, [0,1)
  return (double)(rng_u64(r, lane) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ unsigned long long rng_range64(Rng& r, int lane, unsigned long long range) {
  const unsigned long long zone = (range << __clzll((long long)range)) - 1ull;   // uniform.rs sample_single_inclusive
  for (int guard = 0; guard < 4096; ++guard) {
    const unsigned long long v = rng_u64(r, lane);
    const unsigned long long hi = __umul64hi(v, range), lo = v * range;
    if (lo <= zone) return hi;
  }
  return 0;
}
__device__ uint32_t rng_range32(Rng& r, int lane, uint32_t range) {
  const uint32_t zone = (range << __clz((int)range)) - 1u;
  for (int guard = 0; guard < 4096; ++guard) {
    const uint32_t v = rng_u32(r, lane);
    const unsigned long long m = (unsigned long long)v * range;
    if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
  }
  return 0;
}

__device__ __forceinline__ State state_of(const Agg& a) {   // simulation.rs:122-135
  State s;
  s.net = a.co2 - a.offs;
  s.opinion = a.opcnt > 0 ? a.optot / (double)a.opcnt : 1.0;
  s.balance = ((a.tg + a.ig) + a.sg) - a.usage;
  s.cost = a.gcost + a.ocost;
  return s;
}
__device__ double evaluate_impact(const State& cur, const State& nxt) {   // scoring.rs:46-85 (mode None)
  if (cur.net > 0.0) return (cur.net - nxt.net) / max_abs_one(cur.net);
  double cost_change = nxt.cost - cur.cost;
  double cost_improvement = -cost_change / max_abs_one(cur.cost);
  double opinion_improvement = (nxt.opinion - cur.opinion) / max_abs_one(cur.opinion);
  double cost_weight = cur.cost > kMaxCost * 8.0 ? 0.8 : 0.5;
  double opinion_weight = 1.0 - cost_weight;
  return cost_improvement * cost_weight + opinion_improvement * opinion_weight;
}

// small per-type / per-class tables -> LDS (one dependent LDS read instead of chains of L2 round trips)
// The host table is indexed by (|di|, |dj|) <= 12; the distance, hence the factor, only depends on di^2 + dj^2 (grid
// coordinates are whole kilometres, so dx^2 + dy^2 is exact), and the kernels index by that: one dot product instead of
// two absolute values, two clamps and a linearisation.  Sums that are not a sum of two squares are never read.
// The two planes of Smem::dr (kPlanes) from the blob, word by word: an even word of tab::dr_compact is an entry's low word, an odd one its high
// word, and a lane keeps to one plane (the high plane ends in Smem::park).  Not inlined, and the blob by ADDRESS (eg_field.h's rule): inlined, whichever way it was written — doubles
// split into words, or words — k_rollout<0,0> came out a vector register wider than the 121 it has (profiles/r18_ab_notes.log r18g); once an episode.
static_assert((2 * kDrCompact) % kWave == 0, "whole blocks of 64 words");
__device__ __noinline__ void load_factor_planes(unsigned long long src_addr, int lane) {
  typedef const uint32_t __attribute__((address_space(1)))* G32;
  const G32 src = (G32)src_addr;
  uint32_t w[2 * kDrCompact / kWave];
#pragma unroll
  for (int k = 0; k < 2 * kDrCompact / kWave; ++k) w[k] = src[lane + k * kWave];
  uint32_t* dst = reinterpret_cast<uint32_t*>(&sm) + offsetof(Smem, dr) / 4 + (lane & 1) * kDrHiPlane + (lane >> 1);      // (the high plane ends in Smem::park)
#pragma unroll
  for (int k = 0; k < 2 * kDrCompact / kWave; ++k) dst[k * (kWave / 2)] = w[k];
}
template <bool kPlanes>
__device__ __forceinline__ void load_factor_table(const DevTables& T, int lane) {
  // tails of the staging rows of chunk_product: generators far off the grid (their factor is 1.0), never overwritten
  if (lane < 8) { sm.gstage[0][kWave + lane] = (int)0xC000C000; sm.gstage[1][kWave + lane] = (int)0xC000C000; }
  // (the host lays the compact table out as LDS holds it — tab::dr_compact: one independent load per lane and block of 64, one
  //  memory round trip at the start of an episode where re-indexing the [6][13][13] table here was sixteen dependent ones)
  if constexpr (kPlanes) { load_factor_planes((unsigned long long)T.dr_compact(), lane); return; }
  double v[(kDrCompact + kWave - 1) / kWave];
#pragma unroll
  for (int k = 0; k < (kDrCompact + kWave - 1) / kWave; ++k) v[k] = lane + k * kWave < kDrCompact ? T.dr_compact()[lane + k * kWave] : 1.0;
#pragma unroll
  for (int k = 0; k < (kDrCompact + kWave - 1) / kWave; ++k) if (lane + k * kWave < kDrCompact) reinterpret_cast<double*>(sm.dr)[lane + k * kWave] = v[k];
}
// byte offset of a radius class's factors inside the LDS block — kPlanes: of their low words, 4 bytes an entry — | its cap << 16: what
// chunk_product / factor_by_q take as `table` in the throughput kernels (from the type's info word: bits 16-23 cap, 24-31 first entry / 2)
template <bool kPlanes = false>
__device__ __forceinline__ int throughput_table(int info) {
  return ((int)offsetof(Smem, dr) + (int)(((unsigned)info >> 24) << (kPlanes ? 3 : 4))) | (((info >> 16) & 255) << 16);
}
// small-batch kernel: the generator list starts as padding everywhere; the factor table goes in at a stride of 16 bytes
__device__ __forceinline__ void load_latency_tables(const DevTables& T, int lane) {
  for (int i = lane; i < kLdsGens + 16; i += kWave) sl.gpk[i] = kGenPad4;
  for (int i = lane; i < kRadiusClasses * kD2Stride; i += kWave) sl.dr16[2 * i] = 1.0;
  for (int i = lane; i < kRadiusClasses * 169; i += kWave) {
    const int rc = i / 169, k = i - rc * 169, di = k / 13, dj = k - di * 13, q = di * di + dj * dj;
    if (q <= kD2Max) sl.dr16[2 * (rc * kD2Stride + q)] = T.dr()[i];
  }
}
template <bool kPlanes = false>
__device__ __forceinline__ void load_static_tables(const DevTables& T, int lane, bool with_factors) {
  if (with_factors) load_factor_table<kPlanes>(T, lane);
  if (lane < kTypes) {
    const int rc = T.rclass()[lane];
    sm.type_info[lane] = T.variant()[lane] | (rc << 4) | (T.reach()[rc] << 8) | (T.cls()[lane] << 12) | (T.dr_meta()[8 + rc] << 16) |
                         (int)((unsigned)(T.dr_meta()[rc] >> 1) << 24);
    sm.type_out[lane] = T.out_mw()[lane];
    sm.type_co2[lane] = T.co2_t()[lane];
  }
}

// ---- placement: arg-max over the 51x51 distinct candidates (Q10) -------------------------------------------
// Reference (metal_location_search.rs:110-176): score(c) = ((te[c] * prod_{g in list order, d<R} d/R) * coast(c)) * 0.9,
// keep the first strictly greater score in (i, j) order, i.e. the maximum with ties to the lowest cell index.
// Here the candidates of (year, radius class, marine) come pre-sorted by their unpenalised score (host, eg_device_tables.cpp).
// Every penalty factor is in [0, 1] and IEEE multiplication is monotone, so score(c) <= base(c): the scan takes 64
// candidates at a time (one per lane, each lane folding the generator list in order for its own cell) and stops as
// soon as the next chunk's largest base score is below the best score found — the same winner, bit for bit, as the
// exhaustive search, usually after one or two chunks.
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// max over the 64 lanes of a NON-NEGATIVE double, returned in every lane.  For non-negative IEEE doubles the order of the
// values is the order of their bit patterns, so the maximum is found on the high dwords first and then on the low dwords
// of the lanes that hold that high dword: two 32-bit DPP reductions (row shifts / row broadcasts; a lane without a DPP
// source reads 0, the identity of an unsigned max) instead of one on 64-bit pairs.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#define EG_DPP_MAX_STEP(ctrl, row_mask, bank_mask)                                                      \
  {                                                                                                     \
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, row_mask, bank_mask, false); \
    v = o > v ? o : v;                                                                                  \
  }
  EG_DPP_MAX_STEP(0x111, 0xf, 0xf)   // row_shr:1
  EG_DPP_MAX_STEP(0x112, 0xf, 0xf)   // row_shr:2
  EG_DPP_MAX_STEP(0x113, 0xf, 0xf)   // row_shr:3
  EG_DPP_MAX_STEP(0x114, 0xf, 0xe)   // row_shr:4 bank_mask:0xe
  EG_DPP_MAX_STEP(0x118, 0xf, 0xc)   // row_shr:8 bank_mask:0xc
  EG_DPP_MAX_STEP(0x142, 0xa, 0xf)   // row_bcast:15 row_mask:0xa
  EG_DPP_MAX_STEP(0x143, 0xc, 0xf)   // row_bcast:31 row_mask:0xc
#undef EG_DPP_MAX_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ double wave_max_f64(double v) {
  const unsigned hi = (unsigned)__double2hiint(v);
  const unsigned mh = wave_max_u32(hi);
  const unsigned ml = wave_max_u32(hi == mh ? (unsigned)__double2loint(v) : 0u);
  return __hiloint2double((int)mh, (int)ml);
}

// Inclusive prefix sum over the 64 lanes (DPP: four row shifts, two row broadcasts; a lane without a source adds 0.0).
// (The shifts say bound_ctrl: a lane whose source lies outside the row reads 0 — no register has to be zeroed first; the
//  broadcasts only write the rows of their row mask, the others keep the 0 they were given.)
__device__ __forceinline__ double wave_prefix_sum_f64(double x) {
#define EG_DPP_ADD_STEP(ctrl, row_mask, bank_mask, bound)                                                           \
  {                                                                                                                 \
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), ctrl, row_mask, bank_mask, bound);             \
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), ctrl, row_mask, bank_mask, bound);             \
    x = x + __hiloint2double(hi, lo);                                                                               \
  }
  EG_DPP_ADD_STEP(0x111, 0xf, 0xf, true)    // row_shr:1
  EG_DPP_ADD_STEP(0x112, 0xf, 0xf, true)    // row_shr:2
  EG_DPP_ADD_STEP(0x114, 0xf, 0xf, true)    // row_shr:4
  EG_DPP_ADD_STEP(0x118, 0xf, 0xf, true)    // row_shr:8
  EG_DPP_ADD_STEP(0x142, 0xa, 0xf, false)   // row_bcast:15 -> rows 1, 3
  EG_DPP_ADD_STEP(0x143, 0xc, 0xf, false)   // row_bcast:31 -> rows 2, 3
#undef EG_DPP_ADD_STEP
  return x;
}

// The weighted pick of the samplers (sampling.rs:182-233, :352-370, :406-416): total = sum of the table in table order,
// v = u * total, then v -= table[a] in table order; the pick is the number of entries after which v was still positive
// (weights are not negative, so v never grows).  Every addition and subtraction rounds, so sum and walk are sequential
// chains — but the OUTCOME only depends on the signs of the v_a, and v_a differs from u * T - P_a, with the prefix sums
// P_a and their last value T evaluated in any other order, by less than 2^-45 * total (61 roundings of values below
// `total` in the sequential sum, 61 in the walk, a 6-level tree on the other side, one multiplication and one
// subtraction each).  So: prefix sums in parallel, and if every u * T - P_a is further than 2^-40 * T from zero the signs
// — hence the pick — are those of the sequential sum-and-walk.  Otherwise (a draw within 1e-12 of a boundary) the
// sequential chains decide.  tests/test_weighted_pick.py checks the rule on the CPU.
// Not inlined (four call sites; inlined, the rarely-run sequential part costs the episode loop its registers).  The table
// is given by its byte offset inside the workgroup's LDS block so that it is read with LDS instructions.
__device__ __noinline__ int weighted_pick(int table_offset, int n, double u, int lane) {
#if defined(EG_PROBE_SKIP) && EG_PROBE_SKIP == 5
  if (true) return (int)(u * (double)n);
#endif
  const double* table = reinterpret_cast<const double*>(reinterpret_cast<const char*>(&sm) + table_offset);
  const double w = lane < n ? table[lane] : 0.0;
  const double P = wave_prefix_sum_f64(w);
  const double T = readlane_f64(P, kWave - 1);             // lanes >= n added 0.0
  const double d = u * T - P;
  const unsigned long long valid = (1ull << n) - 1ull;      // n < 64
  if ((__ballot(dabs(d) <= T * 0x1p-40) & valid) == 0ull) return __popcll(__ballot(d > 0.0) & valid);
  double total = 0.0;
  for (int a = 0; a < n; ++a) total += table[a];
  int pick = 0; double v = u * total;
  for (int a = 0; a < n; ++a) { v -= table[a]; pick += v > 0.0 ? 1 : 0; }
  return pick;
}

typedef short short2v __attribute__((ext_vector_type(2)));
// the double whose low word is at byte `at` of the LDS block and whose high word is kDrHiPlane words on (Smem::dr).  Two plain loads:
// the compiler joins them into one two-address read (ds_read2st64_b32) and keeps its own wait counts.  (Planes back to back, 352 words
// apart, make it two ds_read_b32: measured, the lean grid then gains a third of what it gains with one: profiles/r18_ab_notes.log r18g.)
__device__ __forceinline__ double factor_word_pair(int at) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(&sm) + at);
  return __hiloint2double((int)p[kDrHiPlane], (int)p[0]);
}
// factor of one generator for this lane's candidate: 2 (ci - gi, cj - gj) as two int16 — both sides come with their coordinates
// doubled —, four times their squared length by one dot product whose accumulator is the byte offset of the class's low words
// (`table_offset`, uniform): the byte address of the factor, capped at the class's own radius squared (`cap_at` = table_offset +
// 4 cap: the table holds 1.0 there)
template <bool kPlanes = false>
__device__ __forceinline__ double factor_at(short2v cpk2, int gen_packed2, int table_offset, int cap_at) {
  short2v g; __builtin_memcpy(&g, &gen_packed2, 4);
  const short2v d = cpk2 - g;
  if constexpr (!kPlanes) {      // the table of doubles: plain coordinates, `cap_at` the class's radius squared; an instruction more for the address
    int q, dbits; __builtin_memcpy(&dbits, &d, 4);
    asm("v_dot2_i32_i16 %0, %1, %1, 0" : "=v"(q) : "v"(dbits));
    q = q < cap_at ? q : cap_at;
    return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(&sm) + (table_offset + q * 8));
  }
  // (the three-operand form with a scalar accumulator: from the builtin the compiler makes the two-operand accumulating
  //  v_dot2c and a v_mov to set its destination first — one instruction more per factor)
  int at, dbits; __builtin_memcpy(&dbits, &d, 4);
  asm("v_dot2_i32_i16 %0, %1, %1, %2" : "=v"(at) : "v"(dbits), "s"(table_offset));
  at = at < cap_at ? at : cap_at;
  return factor_word_pair(at);
}

// A search multiplies te by the factor of every generator, in list order.  Searches of the same (year, variant) revisit
// the same candidates while the list only grows at its end, so the running product of a chunk is kept between searches
// and a later search of that (year, variant) continues it with the generators added since — the same multiplications in
// the same order, hence the same bits.  (Years with many additions — the slow episodes — mostly repeat one variant.)
struct PrefixCache { double product; int key; int count; };      // key: year << 8 | variant, -1 = empty; count: generators folded in

// s_init times the factors of generators [k0, ngen_s) for this lane's candidate cell.  `stage`: 0 on the episode wave, 1 on
// the helper wave (each wave has its own staging row in LDS).
// A lone wave issues one instruction per turn of its SIMD whatever the instruction is, so the loop is written for the
// fewest instructions per generator: the packed coordinates of 64 generators are staged in LDS once and come back four
// at a time as ONE broadcast 128-bit read (instead of a readlane and a lane-index add each); per generator that leaves a
// packed subtract, the dot product, the cap, the address, the table read and the multiply.
// Throughput kernel (one wave per episode, sixteen episodes per CU).  `stage`: the wave's staging row in LDS.
// The packed coordinates of 64 generators are staged in LDS once and come back four at a time as ONE broadcast 128-bit
// read (instead of a readlane and a lane-index add each); per generator that leaves a packed subtract, the dot product,
// the cap, the table read and the multiply — the dot product is the factor's address already (factor_at, Smem::dr).
// `row0_kept` (lean / short-replay kernels): staging row 0 is kept up to date by the episode — a generator's packed coordinates are
// appended to it when the generator is placed (k_rollout), its other entries stay padding — so the first 64 generators need no
// staging at all: a chunk re-staged the same list, cell -> (i, j) division included, ~15 vector instructions, 95 times an episode.
// Blocks beyond the first 64 are staged in row 1 (the helper wave's, unused in those kernels).
// `xy4`: the candidate's packed coordinates times four (PsRec::pad, as the small-batch kernel uses them): a packed shift gives
// (2 ci, 2 cj) where dividing the cell by the grid's width took eight instructions per chunk.  The staging rows hold (2 gi, 2 gj).
template <bool kPlanes = false>
__device__ __forceinline__ double chunk_product(int table, int lane, int k0, int ngen_s, double s_init, int xy4, int stage, bool row0_kept = false) {
  double s = s_init;
  const short2v cpk = __builtin_bit_cast(short2v, xy4) >> (short)(kPlanes ? 1 : 2);      // (4 ci, 4 cj) -> (2 ci, 2 cj) / (ci, cj): both halves are small and not negative
  // throughput_table(): the class's factors inside the LDS block, and where they end (uniform; behind a call that is not inlined it arrives in a vector register)
  const int dr_off = table & 0xFFFF, cap = kPlanes ? dr_off + 4 * (table >> 16) : table >> 16;
  const int k0_s = __builtin_amdgcn_readfirstlane(k0);           // uniform (it comes out of a per-wave cache): scalar loop control
  for (int gb = k0_s; gb < ngen_s; gb += kWave) {                 // generators in list order
    const bool kept = row0_kept && gb == 0;
    int* row = sm.gstage[row0_kept && gb > 0 ? 1 : stage];
    const int4* row4 = reinterpret_cast<const int4*>(row);
    if (!kept) {
      // Lanes beyond the list hold a generator far off the grid: its squared distance caps at 144, where the table is 1.0.
      const int mine = gb + lane < ngen_s ? (int)(sm.gcell[gb + lane] & 0xFFF) : -1;
      const int mi = mine / kGrid;
      const int mp = mine < 0 ? (int)0xC000C000 : ((mi | ((mine - mi * kGrid) << 16)) << (kPlanes ? 1 : 0));   // (gi, gj) as two int16; kPlanes: doubled
      row[lane] = mp;
    }
    asm volatile("" ::: "memory");      // LDS executes a wave's accesses in program order: only the compiler must keep it
    const int cnt = ngen_s - gb < kWave ? ngen_s - gb : kWave;
    const int groups = (cnt + 3) >> 2;
    // Branch-free: the factor table holds 1.0 wherever d >= R (including the cap), and x * 1.0 == x exactly, so
    // out-of-range generators and the padding up to a multiple of four multiply by 1.0 instead of branching.
    // Software-pipelined: while four factors are multiplied in list order (only the multiplies form a chain) the next
    // four are on their way from the table; two register sets take turns.
#define EG_FACTORS_LOOSE(g4, f0, f1, f2, f3) { f0 = factor_at<kPlanes>(cpk, g4.x, dr_off, cap); f1 = factor_at<kPlanes>(cpk, g4.y, dr_off, cap); \
                                               f2 = factor_at<kPlanes>(cpk, g4.z, dr_off, cap); f3 = factor_at<kPlanes>(cpk, g4.w, dr_off, cap); }
    double a0, a1, a2, a3, b0, b1, b2, b3;
    int4 gc = row4[0], gn = row4[1];
    EG_FACTORS_LOOSE(gc, a0, a1, a2, a3)
    for (int k = 1;;) {
      if (k >= groups) { s = s * a0; s = s * a1; s = s * a2; s = s * a3; break; }
      gc = gn; gn = row4[k + 1];
      EG_FACTORS_LOOSE(gc, b0, b1, b2, b3)
      __builtin_amdgcn_sched_barrier(0);
      s = s * a0; s = s * a1; s = s * a2; s = s * a3;
      ++k;
      if (k >= groups) { s = s * b0; s = s * b1; s = s * b2; s = s * b3; break; }
      gc = gn; gn = row4[k + 1];
      EG_FACTORS_LOOSE(gc, a0, a1, a2, a3)
      __builtin_amdgcn_sched_barrier(0);
      s = s * b0; s = s * b1; s = s * b2; s = s * b3;
      ++k;
    }
#undef EG_FACTORS_LOOSE
    asm volatile("" ::: "memory");
  }
  return s;
}

// Small-batch kernel (an episode wave and a helper wave per episode, at most four episodes per CU).  A lone wave issues
// one instruction per turn of its SIMD whatever the instruction is, so this version is written for the fewest
// instructions per generator, and spends LDS (plentiful at four workgroups per CU) to get there:
//  * the packed coordinates of the episode's generators live in LDS (sl.gpk, appended when a generator is placed, both
//    waves read it): no staging, no cell -> (i, j) division per search, four generators per broadcast 128-bit read;
//  * coordinates are kept times four and the factor table has a stride of 16 bytes, so the dot product of the packed
//    difference with itself, accumulated onto the table's address, IS the address of the factor: per generator a packed
//    subtract, the dot product, the cap, the table read and the multiply;
//  * one straight-line loop body of two groups, so the wait counts stay exact; padding multiplies by 1.0.
// k0: generators [0, k0) are already in s_init (kept product); the first group is masked accordingly.
// kMaskTail (helper wave): entries behind the list are not trusted to be padding — the episode wave may append the next
// generator while this chunk is still being evaluated — so the last group is taken out of the pipeline and masked.
template <bool kMaskTail>
__device__ __forceinline__ double chunk_product_latency(int class_off, int k0, int ngen_s, double s_init, int xy4) {
  short2v cpk; __builtin_memcpy(&cpk, &xy4, 4);
  double s = s_init;
  const int k0_s = __builtin_amdgcn_readfirstlane(k0);
  const int g0 = k0_s >> 2, skip = k0_s & 3;
  const int groups = ((ngen_s + 3) >> 2) - g0;
  if (groups <= 0) return s;
  const int4* row4 = reinterpret_cast<const int4*>(sl.gpk) + g0;
  const char* t0 = reinterpret_cast<const char*>(sl.dr16);
  const int cap = class_off + 16 * kD2Max;
  // (the three-operand form with the class's offset, uniform, as a scalar accumulator: from the accumulating builtin the compiler makes the
  //  two-operand v_dot2c and a v_mov to set its destination first — config 1: 0.2546 -> 0.2505 ms a batch, profiles/r18_ab_notes.log)
  const int class_off_s = __builtin_amdgcn_readfirstlane(class_off);
#define EG_LAT_DOT(q_, e_) { int eb_; __builtin_memcpy(&eb_, &e_, 4); asm("v_dot2_i32_i16 %0, %1, %1, %2" : "=v"(q_) : "v"(eb_), "s"(class_off_s)); }
#define EG_FACTORS(g4, f0, f1, f2, f3) { \
    short2v e0, e1, e2, e3; int q0, q1, q2, q3; \
    { short2v t; __builtin_memcpy(&t, &g4.x, 4); e0 = cpk - t; __builtin_memcpy(&t, &g4.y, 4); e1 = cpk - t; \
      __builtin_memcpy(&t, &g4.z, 4); e2 = cpk - t; __builtin_memcpy(&t, &g4.w, 4); e3 = cpk - t; } \
    __builtin_amdgcn_sched_barrier(0); \
    EG_LAT_DOT(q0, e0) EG_LAT_DOT(q1, e1) EG_LAT_DOT(q2, e2) EG_LAT_DOT(q3, e3) \
    __builtin_amdgcn_sched_barrier(0); \
    q0 = q0 < cap ? q0 : cap; q1 = q1 < cap ? q1 : cap; q2 = q2 < cap ? q2 : cap; q3 = q3 < cap ? q3 : cap; \
    __builtin_amdgcn_sched_barrier(0); \
    f0 = *reinterpret_cast<const double*>(t0 + q0); f1 = *reinterpret_cast<const double*>(t0 + q1); \
    f2 = *reinterpret_cast<const double*>(t0 + q2); f3 = *reinterpret_cast<const double*>(t0 + q3); }
  double a0, a1, a2, a3, b0, b1, b2, b3;
  if constexpr (kMaskTail) {
    const int last = groups - 1, tail = ngen_s & 3;
    if (last > 0) {      // groups [0, last) through the pipeline (its look-ahead reads are never multiplied)
      int4 ga = row4[0], gb4 = row4[1];
      if (skip > 0) ga.x = kGenPad4;
      if (skip > 1) ga.y = kGenPad4;
      if (skip > 2) ga.z = kGenPad4;
      EG_FACTORS(ga, a0, a1, a2, a3)
      const int pairs = last >> 1;
      for (int p = 0; p < pairs; ++p) {
        ga = row4[2 * p + 2];
        EG_FACTORS(gb4, b0, b1, b2, b3)
        __builtin_amdgcn_sched_barrier(0);
        s = s * a0; s = s * a1; s = s * a2; s = s * a3;
        gb4 = row4[2 * p + 3];
        EG_FACTORS(ga, a0, a1, a2, a3)
        __builtin_amdgcn_sched_barrier(0);
        s = s * b0; s = s * b1; s = s * b2; s = s * b3;
      }
      if (last & 1) { s = s * a0; s = s * a1; s = s * a2; s = s * a3; }
    }
    int4 gl = row4[last];
    if (last == 0) { if (skip > 0) gl.x = kGenPad4; if (skip > 1) gl.y = kGenPad4; if (skip > 2) gl.z = kGenPad4; }
    if (tail != 0) { if (tail < 2) gl.y = kGenPad4; if (tail < 3) gl.z = kGenPad4; gl.w = kGenPad4; }
    EG_FACTORS(gl, a0, a1, a2, a3)
    s = s * a0; s = s * a1; s = s * a2; s = s * a3;
    return s;
  }
  int4 ga = row4[0], gb4 = row4[1];
  if (skip > 0) ga.x = kGenPad4;
  if (skip > 1) ga.y = kGenPad4;
  if (skip > 2) ga.z = kGenPad4;
  EG_FACTORS(ga, a0, a1, a2, a3)
  const int pairs = groups >> 1;
  for (int p = 0; p < pairs; ++p) {          // a holds group 2p
    ga = row4[2 * p + 2];
    EG_FACTORS(gb4, b0, b1, b2, b3)
    __builtin_amdgcn_sched_barrier(0);        // the four table reads stay in flight ahead of the multiply chain
    s = s * a0; s = s * a1; s = s * a2; s = s * a3;
    gb4 = row4[2 * p + 3];
    EG_FACTORS(ga, a0, a1, a2, a3)             // (on the last trip of an even count: a group of padding, never multiplied)
    __builtin_amdgcn_sched_barrier(0);
    s = s * b0; s = s * b1; s = s * b2; s = s * b3;
  }
  if (groups & 1) { s = s * a0; s = s * a1; s = s * a2; s = s * a3; }
#undef EG_FACTORS
#undef EG_LAT_DOT
  return s;
}
// Final score of this lane's candidate (rank r of the sorted list) against the episode's generator list.
// kLatency: small-batch kernel (`table` = byte offset of the radius class inside sl.dr16, xy4 = the candidate's packed
// coordinates); otherwise the throughput kernel (`table` = throughput_table() of the type, `cell`).
template <bool kLatency, bool kPlanes = false>
__device__ __forceinline__ double chunk_score(int table, double size_factor, int lane, int ngen_s, int r, double te,
                                              double cf, int cell, int xy4, bool row0_kept = false) {
  double p;
  if constexpr (kLatency) p = chunk_product_latency<false>(table, 0, ngen_s, te, xy4);
  else p = chunk_product<kPlanes>(table, lane, 0, ngen_s, te, xy4, 0, row0_kept);
  const double s = (p * cf) * size_factor;
  return r < kCells ? s : 0.0;
}
// ... continuing the product kept from the last search of the same (year, variant) when there is one
template <bool kLatency>
__device__ __forceinline__ double chunk_score(int table, double size_factor, int lane, int ngen_s, int r, double te,
                                              double cf, int cell, int xy4, PrefixCache& cache, int key, int stage) {
  double s = te; int k0 = 0;
  if (cache.key == key && cache.count <= ngen_s) { s = cache.product; k0 = cache.count; }
  if constexpr (kLatency) s = stage ? chunk_product_latency<true>(table, k0, ngen_s, s, xy4) : chunk_product_latency<false>(table, k0, ngen_s, s, xy4);
  else s = chunk_product(table, lane, k0, ngen_s, s, xy4, stage);
  cache.product = s; cache.key = key; cache.count = ngen_s;
  s = (s * cf) * size_factor;
  return r < kCells ? s : 0.0;
}

struct ChunkBest { double score, m03; int cell; };
// maximum of a chunk's scores, ties to the lowest cell, with the winner's 0.03 * mean settlement opinion
template <bool kLatency>
__device__ __forceinline__ ChunkBest chunk_reduce(double s, int cell, double m03) {
  ChunkBest b;
  // Scores are not negative, so their order is the order of their bit patterns.  Almost always a single lane holds the
  // largest high word: that lane is the winner and nothing else has to be reduced.  (Small-batch kernel: fewer instructions on
  // the critical path.  Throughput kernels: fewer vector instructions — they are bound by vector issue; 16 384 sampled episodes
  // 1.002 -> 0.982 ms, profiles/r04_ab_notes.log r04za; the branch-free form had measured equal before the kernel was that tight.)
  const unsigned hi = (unsigned)__double2hiint(s);
  const unsigned mh = wave_max_u32(hi);
  const unsigned long long top = __ballot(hi == mh);
  if (__popcll(top) == 1) {
    const int w = __ffsll((long long)top) - 1;
    b.score = readlane_f64(s, w); b.cell = __builtin_amdgcn_readlane(cell, w); b.m03 = readlane_f64(m03, w);
    return b;
  }
  const unsigned ml = wave_max_u32(hi == mh ? (unsigned)__double2loint(s) : 0u);
  b.score = __hiloint2double((int)mh, (int)ml);
  int win_c = s == b.score ? cell : kCells;
  const unsigned long long holders = __ballot(s == b.score);
  if (__popcll(holders) == 1) win_c = __builtin_amdgcn_readlane(cell, __ffsll((long long)holders) - 1);
  else {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) { const int other = __shfl_xor(win_c, sh); win_c = other < win_c ? other : win_c; }
  }
  b.cell = win_c;
  const unsigned long long owner = __ballot(s == b.score && cell == win_c);   // the lane that holds the winner
  b.m03 = readlane_f64(m03, __ffsll((long long)owner) - 1);
  return b;
}

// Workgroup barrier that orders LDS only: the episode's output stores and table loads stay in flight across it.
__device__ __forceinline__ void wg_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- lists beyond the on-chip window (long-replay variant only) ------------------------------------------------------
// The reference's lists are Vecs; a replay episode applies and records every action twice, so in a training loop
// the replayed lists double whenever a replay episode becomes the best strategy: 468 generators after seven updates, 965
// actions in the best list soon after at larger batches.  The first kLdsGens generators / offsets of an episode live in LDS
// (gcell / gbm / opack); a long-replay episode that grows past that goes on in its own output record — it appends every
// generator and offset there anyway (gen_cell / gen_pack / off_pack, EG_MAX_GENS entries) — and reads those entries back in
// blocks of 64 wherever a list is walked: the year-start folds, the exact product of a candidate, a field that joins, the
// exact scan.  Blocks start at multiples of 64 and kLdsGens is one, so a block is either all window or all tail.
// The entries were stored by this wave itself: they are read past the CU's L1 (agent scope), like the penalty field.
struct ListTail { unsigned long long gen_cell, gen_pack, off_pack; };      // addresses: they cross non-inlined calls as integers
typedef unsigned short __attribute__((address_space(1)))* GlobalU16;
__device__ __forceinline__ int tail_u16(unsigned long long addr, int i) {
  return (int)__hip_atomic_load((GlobalU16)addr + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// cell of generator g (a lane each), from the window or from the record; `far`: what a lane beyond the list gets
__device__ __forceinline__ int list_cell(unsigned long long tail_cells, int gb, int lane, int ngen_s, int far) {
  if (gb + lane >= ngen_s) return far;
  return gb < kLdsGens ? (int)(sm.gcell[gb + lane] & 0xFFF) : tail_u16(tail_cells, gb + lane);
}

// ---- aggregates at the start of a year: existing plant first (host tables), then every generator in list order.
//      The lanes gather the per-generator terms in parallel (year_gather: requests only); the sums are then folded lane
//      by lane with readlane, i.e. in list order (year_fold).  Output / CO2 terms of a plant never change (delays off),
//      so the class sums carry over from the end of last year whenever the existing-plant prefix did (`carry`), bit for
//      bit; otherwise they are folded here as well. ----
// acc + x[lane J of the row], in every lane of that row.  gfx90a and later have a DPP form of the VOP2 double-precision
// multiply-accumulate (row_newbcast only; v_add_f64 is VOP3 and has none): acc = x[J] * 1.0 + acc is that addition — the product is
// exact and the sum is rounded once — so a sum in list order over 16 lanes is 16 instructions, instead of 16 x (two v_readlane + one
// add) through scalar registers.
// Inline assembly is opaque to the hazard recogniser: a DPP read needs wait states after a VALU write of the register it reads (2) or
// of EXEC (5).  The s_nop and the sixteen accumulations are therefore ONE asm statement with x as an input: whatever produces x, and
// whatever the compiler schedules in front of the statement, is followed by the five wait states before the first DPP read — two
// statements (a bare s_nop, then the DPP instructions) left the scheduler free to put the producer of x between them.
#define EG_FMAC_DPP(acc_, x_, j_) "v_fmac_f64_dpp " acc_ ", " x_ ", %[one] row_newbcast:" #j_ " row_mask:0xf bank_mask:0xf\n\t"
// acc (the same value in every lane) + x[16 row + 0] + ... + x[16 row + 15], added in that order; valid in the lanes of each row for
// that row's sixteen values
__device__ __forceinline__ double fold_row16(double acc, double x) {
  const double one = 1.0;
  asm("s_nop 4\n\t"
      EG_FMAC_DPP("%[a]", "%[x]", 0) EG_FMAC_DPP("%[a]", "%[x]", 1) EG_FMAC_DPP("%[a]", "%[x]", 2) EG_FMAC_DPP("%[a]", "%[x]", 3)
      EG_FMAC_DPP("%[a]", "%[x]", 4) EG_FMAC_DPP("%[a]", "%[x]", 5) EG_FMAC_DPP("%[a]", "%[x]", 6) EG_FMAC_DPP("%[a]", "%[x]", 7)
      EG_FMAC_DPP("%[a]", "%[x]", 8) EG_FMAC_DPP("%[a]", "%[x]", 9) EG_FMAC_DPP("%[a]", "%[x]", 10) EG_FMAC_DPP("%[a]", "%[x]", 11)
      EG_FMAC_DPP("%[a]", "%[x]", 12) EG_FMAC_DPP("%[a]", "%[x]", 13) EG_FMAC_DPP("%[a]", "%[x]", 14) EG_FMAC_DPP("%[a]", "%[x]", 15)
      : [a] "+v"(acc) : [x] "v"(x), [one] "v"(one));
  return acc;
}
// two such sums side by side (the two chains are independent: interleaved, neither waits for the other's accumulation)
__device__ __forceinline__ void fold2_row16(double& a, double xa, double& b, double xb) {
  const double one = 1.0;
#define EG_FMAC2(j_) EG_FMAC_DPP("%[a]", "%[xa]", j_) EG_FMAC_DPP("%[b]", "%[xb]", j_)
  asm("s_nop 4\n\t"
      EG_FMAC2(0) EG_FMAC2(1) EG_FMAC2(2) EG_FMAC2(3) EG_FMAC2(4) EG_FMAC2(5) EG_FMAC2(6) EG_FMAC2(7)
      EG_FMAC2(8) EG_FMAC2(9) EG_FMAC2(10) EG_FMAC2(11) EG_FMAC2(12) EG_FMAC2(13) EG_FMAC2(14) EG_FMAC2(15)
      : [a] "+v"(a), [b] "+v"(b) : [xa] "v"(xa), [xb] "v"(xb), [one] "v"(one));
#undef EG_FMAC2
}

struct YearTerms { double2 g_cc; double g_m03, g_t12, o_v, o_c; int g_t; };
struct YearSums { double gcost, optot, offs, ocost, co2, tg, ig, sg; int opcnt; };

__device__ __forceinline__ void year_gather_gens(const DevTables& T, int lane, int yi, int base, int ngen_s, YearTerms& t) {
  const double* ccy = T.cc() + (unsigned)yi * kTypes * kYears * kMults * 2;
  const int g = base + lane;
  const bool valid = g < ngen_s;
  const int gc = valid ? sm.gcell[g] : 0, bm = valid ? sm.gbm[g] : 0;
  const int cell = gc & 0xFFF, b = bm & 31, m = bm >> 5;
  t.g_t = gc >> 12;
  t.g_cc = *reinterpret_cast<const double2*>(ccy + ((unsigned)(t.g_t * kYears + b) * kMults + m) * 2);
  t.g_m03 = T.m03()[cell]; t.g_t12 = T.t12()[(unsigned)yi * kTypes + t.g_t];
}
__device__ __forceinline__ void year_gather_offsets(const DevTables& T, int lane, int yi, int base, int noff_s, YearTerms& t) {
  const int k = base + lane;
  const int p = k < noff_s ? sm.opack[k] : 0;
  const int ot = p & 15, b = (p >> 4) & 31, m = p >> 9;
  t.o_v = T.offv()[((unsigned)yi * kOffsetTypes + ot) * kYears + b]; t.o_c = T.offc()[((unsigned)yi * kOffsetTypes + ot) * kMults + m];
}
// the same requests for a block of the list's tail (long-replay variant): the entries come from the episode's record
__device__ __forceinline__ void year_gather_gens_tail(const DevTables& T, int lane, int yi, int base, int ngen_s, YearTerms& t, const ListTail& tail) {
  const double* ccy = T.cc() + (unsigned)yi * kTypes * kYears * kMults * 2;
  const int g = base + lane;
  const bool valid = g < ngen_s;
  const int cell = valid ? tail_u16(tail.gen_cell, g) : 0, pk = valid ? tail_u16(tail.gen_pack, g) : 0;      // type | build year << 4 | mult << 9
  const int b = (pk >> 4) & 31, m = pk >> 9;
  t.g_t = pk & 15;
  t.g_cc = *reinterpret_cast<const double2*>(ccy + ((unsigned)(t.g_t * kYears + b) * kMults + m) * 2);
  t.g_m03 = T.m03()[cell]; t.g_t12 = T.t12()[(unsigned)yi * kTypes + t.g_t];
}
__device__ __forceinline__ void year_gather_offsets_tail(const DevTables& T, int lane, int yi, int base, int noff_s, YearTerms& t, const ListTail& tail) {
  const int k = base + lane;
  const int p = k < noff_s ? tail_u16(tail.off_pack, k) : 0;
  const int ot = p & 15, b = (p >> 4) & 31, m = p >> 9;
  t.o_v = T.offv()[((unsigned)yi * kOffsetTypes + ot) * kYears + b]; t.o_c = T.offc()[((unsigned)yi * kOffsetTypes + ot) * kMults + m];
}
// the first 64 entries of each list are requested here; year_fold gathers the rest (rare) itself
__device__ __forceinline__ YearTerms year_gather(const DevTables& T, int lane, int yi, int ngen_s, int noff_s) {
  YearTerms t; t.g_cc.x = 0.0; t.g_cc.y = 0.0; t.g_m03 = 0.0; t.g_t12 = 0.0; t.o_v = 0.0; t.o_c = 0.0; t.g_t = 0;
  if (ngen_s > 0) year_gather_gens(T, lane, yi, 0, ngen_s, t);
  if (noff_s > 0) year_gather_offsets(T, lane, yi, 0, noff_s, t);
  return t;
}
// `s` comes in holding the starting values (0 / the existing-plant prefix) and leaves holding the year-start sums
// kLong (long-replay variant): blocks beyond the on-chip window come from the episode's record (`tail`)
template <bool kLong>
__device__ __forceinline__ void year_fold(const DevTables& T, int lane, int yi, int ngen_s, int noff_s, bool carry, YearTerms t,
                                          YearSums& s, const ListTail& tail) {
  for (int base = 0; base < ngen_s; base += kWave) {
    if (!kLong && base > 0) year_gather_gens(T, lane, yi, base, ngen_s, t);      // beyond the first 64 generators (rare)
    const double2 cc = t.g_cc;
    const int ty = t.g_t;
    const double op = (t.g_m03 + t.g_t12) + cc.y;
    // long-replay variant (hundreds of generators, registers to spare): the next block's terms are requested before this block is
    // folded — a memory round trip per block and year otherwise, on the serial path of the batch's longest episodes
    if (kLong && base + kWave < ngen_s) {
      if (base + kWave >= kLdsGens) year_gather_gens_tail(T, lane, yi, base + kWave, ngen_s, t, tail);
      else year_gather_gens(T, lane, yi, base + kWave, ngen_s, t);
    }
    double out = 0.0, co2 = 0.0; int cls = 0;
    if (!carry) { out = sm.type_out[ty]; co2 = sm.type_co2[ty]; cls = (sm.type_info[ty] >> 12) & 3; }
    const int cnt = ngen_s - base < kWave ? ngen_s - base : kWave;
    if (carry) {            // the common year: two independent chains
      int j = 0;
      {      // sixteen generators at a time through the DPP adder (a row padded with +0.0: sums of positive terms, x + 0.0 == x)
        const double cz = lane < cnt ? cc.x : 0.0, oz = lane < cnt ? op : 0.0;
        for (; cnt - j >= 7; j += 16) {      // (below seven generators the scalar path is fewer instructions)
          double ag = s.gcost, ao = s.optot;
          fold2_row16(ag, cz, ao, oz);
          s.gcost = readlane_f64(ag, j); s.optot = readlane_f64(ao, j);      // lane j = the first lane of the row just folded
        }
      }
      for (; j + 4 <= cnt; j += 4) {
        const double c0 = readlane_f64(cc.x, j), c1 = readlane_f64(cc.x, j + 1), c2 = readlane_f64(cc.x, j + 2), c3 = readlane_f64(cc.x, j + 3);
        const double o0 = readlane_f64(op, j), o1 = readlane_f64(op, j + 1), o2 = readlane_f64(op, j + 2), o3 = readlane_f64(op, j + 3);
        s.gcost += c0; s.optot += o0; s.gcost += c1; s.optot += o1; s.gcost += c2; s.optot += o2; s.gcost += c3; s.optot += o3;
      }
      for (; j < cnt; ++j) { s.gcost += readlane_f64(cc.x, j); s.optot += readlane_f64(op, j); }
    } else {
      for (int j = 0; j < cnt; ++j) {
        s.gcost += readlane_f64(cc.x, j);
        s.optot += readlane_f64(op, j);
        const double oj = readlane_f64(out, j);
        const int cj = __builtin_amdgcn_readlane(cls, j);
        s.co2 += readlane_f64(co2, j);
        if (cj == 1) s.ig += oj; else if (cj == 2) s.sg += oj; else s.tg += oj;
      }
    }
    s.opcnt += cnt;
  }
  for (int base = 0; base < noff_s; base += kWave) {
    if (base > 0) {
      if (kLong && base >= kLdsGens) year_gather_offsets_tail(T, lane, yi, base, noff_s, t, tail);
      else year_gather_offsets(T, lane, yi, base, noff_s, t);
    }
    const double ov = t.o_v, oc = t.o_c;
    const int cnt = noff_s - base < kWave ? noff_s - base : kWave;
    for (int j = 0; j < cnt; ++j) { s.offs += readlane_f64(ov, j); s.ocost += readlane_f64(oc, j); }
  }
}
// The same fold over generators [g_from, g_to) and offsets [o_from, o_to) only (every block gathered here): a year's sums
// can be started before the year's lists are final — they only grow at their ends — and finished afterwards, with the
// additions in the same order (helper wave, small-batch kernel).
__device__ __forceinline__ void year_fold_range(const DevTables& T, int lane, int yi, int g_from, int g_to, int o_from, int o_to,
                                                bool carry, YearSums& s) {
  YearTerms t; t.g_cc.x = 0.0; t.g_cc.y = 0.0; t.g_m03 = 0.0; t.g_t12 = 0.0; t.o_v = 0.0; t.o_c = 0.0; t.g_t = 0;
  if (g_from < g_to) year_gather_gens(T, lane, yi, g_from, g_to, t);      // both requests first, one latency
  if (o_from < o_to) year_gather_offsets(T, lane, yi, o_from, o_to, t);
  for (int base = g_from; base < g_to; base += kWave) {
    if (base > g_from) year_gather_gens(T, lane, yi, base, g_to, t);
    const double2 cc = t.g_cc;
    const int ty = t.g_t;
    const double op = (t.g_m03 + t.g_t12) + cc.y;
    double out = 0.0, co2 = 0.0; int cls = 0;
    if (!carry) { out = sm.type_out[ty]; co2 = sm.type_co2[ty]; cls = (sm.type_info[ty] >> 12) & 3; }
    const int cnt = g_to - base < kWave ? g_to - base : kWave;
    for (int j = 0; j < cnt; ++j) {
      s.gcost += readlane_f64(cc.x, j);
      s.optot += readlane_f64(op, j);
      if (!carry) {
        const double oj = readlane_f64(out, j);
        const int cj = __builtin_amdgcn_readlane(cls, j);
        s.co2 += readlane_f64(co2, j);
        if (cj == 1) s.ig += oj; else if (cj == 2) s.sg += oj; else s.tg += oj;
      }
    }
    s.opcnt += cnt;
  }
  for (int base = o_from; base < o_to; base += kWave) {
    if (base > o_from) year_gather_offsets(T, lane, yi, base, o_to, t);
    const double ov = t.o_v, oc = t.o_c;
    const int cnt = o_to - base < kWave ? o_to - base : kWave;
    for (int j = 0; j < cnt; ++j) { s.offs += readlane_f64(ov, j); s.ocost += readlane_f64(oc, j); }
  }
}
// starting values of the sums for year yi: zero, or the existing-plant prefix of that year (class sums only when they
// do not carry over)
// The helper wave asks for NEXT year's values, which are not in LDS yet: it reads the tables; the episode wave reads the
// copies that came with this year's policy block.
__device__ __forceinline__ YearSums year_sums_init(const DevTables& T, int yi) {
  YearSums s;
  s.gcost = 0.0; s.ocost = 0.0; s.offs = 0.0; s.optot = T.pre_optot()[yi]; s.opcnt = T.pre_opcnt()[yi];
  s.co2 = T.pre_co2()[yi]; s.tg = T.pre_tg()[yi]; s.ig = T.pre_ig()[yi]; s.sg = T.pre_sg()[yi];
  return s;
}
__device__ __forceinline__ YearSums year_sums_init_current() {
  YearSums s;
  const double* ys = sm.pol + snap::kPolYear;
  s.gcost = 0.0; s.ocost = 0.0; s.offs = 0.0; s.optot = ys[4]; s.opcnt = (int)ys[9];
  s.co2 = ys[0]; s.tg = ys[1]; s.ig = ys[2]; s.sg = ys[3];
  return s;
}

// Helper waves (kHelpers > 0, small batches only).  At B <= 4 x CUs every SIMD holds a single episode wave that is
// latency-bound, and a launch lasts as long as its slowest episode, whose time is dominated by placement searches that
// need several chunks.  A helper wave per episode evaluates chunk 1 of every search while the episode wave
// evaluates chunk 0; the episode wave merges the two maxima in chunk order with the same tie rule, so the winner is the
// one the sequential scan finds (a chunk the sequential scan would not have reached only holds candidates whose
// unpenalised score is already below the best, so evaluating it changes nothing).
// One helper, not more: two-wave workgroups leave the CUs a third empty, and the dispatcher needs that slack — with
// exactly-full CUs (three-wave workgroups, 4 per CU) a few workgroups of every launch were queued behind a full CU,
// started late and stretched the launch by a third (scripts/bench_tail.py shows the workgroups-per-CU histogram).
// Letting the helper run further rounds (chunks 3, 5, ...) was measured too and bought nothing.
//   protocol: episode wave writes cmd[seq & 1] and meets the helpers at a barrier; helper h evaluates chunk h and
//   publishes {result, flag = seq}; the episode wave reads a helper's result only if that chunk's bound still reaches
//   the best score, after spinning on its flag.  The next barrier cannot complete before every helper is back.
// The helper reads the episode's generator list (sl.gpk) while the episode wave may already be appending the next
// generator: it masks what lies behind the count it was given (chunk_product_latency<true>).  At the end of a year it
// also keeps the year's starting sums ahead of the episode wave (kCmdYear: the sums of the year after next are started
// over the lists as they are, the next year's — started a year ago — only receive what was added since).
__device__ __forceinline__ void helper_loop(const DevTables& T, int lane, int h) {
  const double size_factor = T.size_factor;
  PrefixCache cache = {0.0, -1, 0};
  YearSums pre; int pre_year = -1, pre_g = 0, pre_o = 0;      // sums of year pre_year over generators [0, pre_g) / offsets [0, pre_o)
  pre.gcost = pre.optot = pre.offs = pre.ocost = pre.co2 = pre.tg = pre.ig = pre.sg = 0.0; pre.opcnt = 0;
  for (uint32_t sq = 1;; ++sq) {
    wg_barrier_lds();
    const int c0 = __builtin_amdgcn_readfirstlane(sm.cmd[sq & 1][0]);
    const int ngen_s = __builtin_amdgcn_readfirstlane(sm.cmd[sq & 1][1]);
    if (c0 < 0) return;
    if (c0 & kCmdYear) {      // next year's starting sums (year_fold), while the episode wave closes the current year
      const int yi = c0 & 31, ngen = ngen_s & 0xFFFF, noff = (ngen_s >> 16) & 0xFFFF;
      const bool carry = ((c0 >> 8) & 1) != 0;
      // The sums of this year were started a year ago over the lists as they were then (see below): only what has been
      // added since is folded now, so the episode wave finds them ready.
      YearSums ys; int g_from = 0, o_from = 0;
      if (pre_year == yi) { ys = pre; g_from = pre_g; o_from = pre_o; }
      else ys = year_sums_init(T, yi);
      year_fold_range(T, lane, yi, g_from, ngen, o_from, noff, carry, ys);
      if (lane == 0) {
        sm.ysum[0] = ys.gcost; sm.ysum[1] = ys.optot; sm.ysum[2] = ys.offs; sm.ysum[3] = ys.ocost;
        sm.ysum[4] = ys.co2; sm.ysum[5] = ys.tg; sm.ysum[6] = ys.ig; sm.ysum[7] = ys.sg; sm.ysum_opcnt = ys.opcnt;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if defined(EG_TEST_DROP_FLAG) && EG_TEST_DROP_FLAG == 2      // negative build: the sums of 2030 are never announced
      if (yi == 5) continue;
#endif
      if (lane == 0) *(volatile uint32_t*)&sm.yflag = sq;
      // ... and the year after that is started over the lists as they are now (they only grow at their ends)
      if (yi + 1 < kYears) {
        pre = year_sums_init(T, yi + 1);
        year_fold_range(T, lane, yi + 1, 0, ngen, 0, noff, ((c0 >> 9) & 1) != 0, pre);
        pre_year = yi + 1; pre_g = ngen; pre_o = noff;
      }
      continue;
    }
    const int yi = c0 & 31, v = (c0 >> 8) & 15, rc = (c0 >> 12) & 15;
    const int r = h * kWave + lane;
#ifdef EG_STAMPS
    const unsigned long long th0 = __builtin_readcyclecounter();
#endif
    const PsRec c = T.ps()[(size_t)(yi * kMaxVariants + v) * kPsStride + r];
#ifdef EG_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long th1 = __builtin_readcyclecounter();
#endif
    const double s = chunk_score<true>(rc * (kD2Stride * 16), size_factor, lane, ngen_s, r, c.te, c.cf, (int)c.cell, (int)c.pad, cache, (yi << 8) | v, 1);
#ifdef EG_STAMPS
    const unsigned long long th2 = __builtin_readcyclecounter();
#endif
    const ChunkBest b = chunk_reduce<true>(s, (int)c.cell, c.m03);
#ifdef EG_STAMPS
    if (lane == 0) { sm.hdbg[h - 1][0] = th1 - th0; sm.hdbg[h - 1][1] = th2 - th1; sm.hdbg[h - 1][2] = __builtin_readcyclecounter() - th2; }
#endif
    if (lane == 0) { sm.hres[h - 1].score = b.score; sm.hres[h - 1].m03 = b.m03; sm.hres[h - 1].cell = b.cell; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if defined(EG_TEST_DROP_FLAG) && EG_TEST_DROP_FLAG == 1      // negative build: search results of 2027 are never announced
    if (yi == 2) continue;
#endif
    if (lane == 0) *(volatile uint32_t*)&sm.hflag[h - 1] = sq;
  }
}

// `between` is called once the candidate records are requested (and, in the small-batch kernel, the helper has its
// command): whatever the caller has to do before it needs the result goes there and runs under the records' latency.
template <int kHelpers, bool kRow0Kept = false, bool kPlanes = false, class Between>
__device__ __forceinline__ int place_search(const DevTables& T, int lane, int yi, int type, int ngen, double* best_score,
                                            double* best_m03, PrefixCache& cache0, Between&& between, int& nchunks,
                                            uint32_t* seq = nullptr, unsigned long long* stamps = nullptr) {
  const int info = __builtin_amdgcn_readfirstlane(sm.type_info[type]);      // uniform: list address arithmetic on the scalar unit
  const int v = info & 15, rc = (info >> 4) & 15;
  const PsRec* __restrict__ list = T.ps() + (size_t)(yi * kMaxVariants + v) * kPsStride;
  // factor table of the radius class: byte offset inside sl.dr16 (small-batch kernel) / inside the LDS block (sm.dr)
  const int table = kHelpers > 0 ? rc * (kD2Stride * 16) : throughput_table<kPlanes>(info);
  const double size_factor = T.size_factor;
#ifdef EG_PROBE_NO_GEN_LOOP      // diagnostic build only (profiles/r04_ab_notes.log r04u): the searches fold no generator — what the generator loops cost
  const int ngen_s = 0;
#else
  const int ngen_s = __builtin_amdgcn_readfirstlane(ngen);
#endif
  constexpr int kChunks = (kCells + kWave - 1) / kWave;
  double best = 0.0, m03w = 0.0; int best_c = kCells;
  int first = 0;
  bool more = true, lost = false;
  // chunk 0 is loaded here, chunk k+1 while chunk k is being evaluated
  PsRec c = list[lane];
  nchunks += 1 + (kHelpers > 0 ? kHelpers + 1 : 0);      // chunk 0; small-batch kernel: the helpers' chunks and the look-ahead one
  if constexpr (kHelpers > 0) {
    // lanes 0..kHelpers: unpenalised score of the first candidate of chunks 1..kHelpers+1 = the bound of that chunk
    const int bl = (lane <= kHelpers ? lane + 1 : 1) * kWave;
    const PsRec cb = list[bl];
    const double bound = (cb.te * cb.cf) * size_factor;
    *seq += 1;
    const uint32_t sq = *seq;
    if (lane == 0) { sm.cmd[sq & 1][0] = yi | (v << 8) | (rc << 12); sm.cmd[sq & 1][1] = ngen_s; }
    wg_barrier_lds();
    between();
#ifdef EG_STAMPS
    if (stamps) stamps[8] += 1;
    const unsigned long long tg0 = __builtin_readcyclecounter();
#endif
    const double s0 = chunk_score<true>(table, size_factor, lane, ngen_s, lane, c.te, c.cf, (int)c.cell, (int)c.pad, cache0, (yi << 8) | v, 0);
#ifdef EG_STAMPS
    const unsigned long long tg1 = __builtin_readcyclecounter();
    if (stamps) stamps[9] += tg1 - tg0;
#endif
    const ChunkBest b0 = chunk_reduce<true>(s0, (int)c.cell, c.m03);
    if (b0.score > 0.0) { best = b0.score; best_c = b0.cell; m03w = b0.m03; }
    // the records of the first chunk the episode wave would evaluate itself are requested before it waits for the
    // helper: when chunk 1 is needed, that chunk usually is as well
    c = list[(kHelpers + 1) * kWave + lane];
    for (int h = 1; h <= kHelpers && more; ++h) {
      if (!(readlane_f64(bound, h - 1) >= best)) { more = false; break; }
#ifdef EG_STAMPS
      const unsigned long long tw0 = __builtin_readcyclecounter();
#endif
      // (on a timeout the search carries on with whatever the result slot holds — values are only compared — and reports
      //  the fault at its end: an early return here cost the episode loop 18 spilled VGPRs)
      for (int spins = 0; __builtin_amdgcn_readfirstlane((int)*(volatile uint32_t*)&sm.hflag[h - 1]) != (int)sq; ++spins) {
        __builtin_amdgcn_s_sleep(1);
        if (spins >= kSpinCap) { lost = true; break; }
      }
      asm volatile("" ::: "memory");
#ifdef EG_STAMPS
      if (stamps) { stamps[6] += __builtin_readcyclecounter() - tw0; stamps[27] += sm.hdbg[h - 1][0]; stamps[28] += sm.hdbg[h - 1][1]; stamps[29] += sm.hdbg[h - 1][2]; stamps[30] += 1; }
#endif
      const double hs = sm.hres[h - 1].score; const int hc = sm.hres[h - 1].cell;
      if (hs > best || (hs == best && hs > 0.0 && hc < best_c)) { best = hs; best_c = hc; m03w = sm.hres[h - 1].m03; }
#ifdef EG_STAMPS
      if (stamps) stamps[8] += 1;
#endif
    }
    if (more && !(readlane_f64(bound, kHelpers) >= best)) more = false;
    first = kHelpers + 1;
#ifdef EG_STAMPS
    if (stamps) stamps[10] += __builtin_readcyclecounter() - tg1;
#endif
  }
  if constexpr (kHelpers == 0) between();
  for (int chunk = first; more && chunk < kChunks; ++chunk) {
    const int r = chunk * kWave + lane;
    const double base = (c.te * c.cf) * size_factor;      // padded with te = 0 beyond the 2601 candidates
    // (throughput kernel: said to be uniform, this is a scalar branch; measured +4.5 % there, -2 % in the small-batch kernel)
    const bool below = !(readlane_f64(base, 0) >= best);
    if (chunk > 0 && (kHelpers > 0 ? below : EG_UNI(below))) break;      // sorted descending: lane 0 holds the chunk's bound
    const double te_cur = c.te, cf_cur = c.cf, m03_cur = c.m03; const int cell_cur = (int)c.cell, xy_cur = (int)c.pad;
    if (chunk + 1 < kChunks) { c = list[r + kWave]; nchunks += 1; }
#ifdef EG_STAMPS
    if (stamps) stamps[8] += 1;
    const unsigned long long tg0 = __builtin_readcyclecounter();
#endif
    // the single-wave kernel keeps the products of chunks 0 and 1, the episode wave of the helper kernel that of chunk 0
    // (the kept products are used by the small-batch kernel only: in the throughput kernel the extra live registers cost
    //  more than the shorter loops give back)
    const double s = chunk_score<(kHelpers > 0), kPlanes>(table, size_factor, lane, ngen_s, r, te_cur, cf_cur, cell_cur, xy_cur, kRow0Kept);
#ifdef EG_STAMPS
    const unsigned long long tg1 = __builtin_readcyclecounter();
    if (stamps) stamps[9] += tg1 - tg0;
#endif
    if (__any(s > best || (s == best && s > 0.0 && cell_cur < best_c))) {
      const ChunkBest b = chunk_reduce<(kHelpers > 0)>(s, cell_cur, m03_cur);
      if (b.score > best || (b.score == best && b.cell < best_c)) { best = b.score; best_c = b.cell; m03w = b.m03; }
    }
#ifdef EG_STAMPS
    if (stamps) stamps[10] += __builtin_readcyclecounter() - tg1;
#endif
  }
  if (best_score) *best_score = best;
  if (best_m03) *best_m03 = m03w;
  if (lost) return kSearchLost;
  return best > 0.0 ? best_c : -1;
}

#include "eg_field.h"

// ---- weight nudges -----------------------------------------------------------------------------------------
// update_deficit_weights(action, d_improvement) followed by update_weights(action, w_improvement), as the repair loop calls
// them after every applied action (simulation.rs:453-486).  Every table entry receives at most one factor from each
// call (its own adjustment, or the "boost the others" factor, or the do-nothing boost), so both calls become one
// lane-parallel pass — lane l owns w[l] and dw[l] — with the same multiplications and clamps per entry.
__device__ __forceinline__ void nudge_after_repair(const DevSnapshot& S, int lane, int action, double d_improvement, double w_improvement) {
  const int slot = deficit_slot_of(action);
  const double lr = S.learning_rate;
  const double adj_d = d_improvement > 0.0 ? 1.0 + (lr * d_improvement * 1.5) : 1.0 / (1.0 + (lr * dabs(d_improvement) * 1.5));
  const double combined = S.immediate_weight * w_improvement + (1.0 - S.immediate_weight) * S.rel_improvement;
  const double adj_w = combined > 0.0 ? 1.0 + (lr * combined) : 1.0 / (1.0 + (lr * dabs(combined)));
  const double boost = S.boost_others;
  wave_sync();
  if (lane < EG_N_ACTIONS) {
    double v = SM_W[lane];
    if (lane == action) v = vmin64_u(vmax64_u(v * adj_w, kMinWeight), kMaxWeight);      // (weights: positive, finite)
    else if (combined < 0.0 && lane < kFirstOffset) v = vmin64_u(v * boost, kMaxWeight);
    if (combined < 0.0 && S.noop_boost && lane == kNothing) v = vmin64_u(v * S.boost_noop, kMaxWeight);
    SM_W[lane] = v;
  }
  if (slot >= 0 && lane < EG_N_DEFICIT) {
    double v = SM_DW[lane];
    if (lane == slot) v = vmin64_u(vmax64_u(v * adj_d, kMinWeight), kMaxWeight);
    else if (d_improvement < 0.0 && lane < 14) v = vmin64_u(v * boost, kMaxWeight);
    SM_DW[lane] = v;
  }
  wave_sync();
}

// ---- sampling (canonical table order; see include/eirgrid_hip.h) -------------------------------------------
__device__ int smart_fallback(Rng& r, int lane, int year) {   // sampling.rs:445-490
  const uint32_t offw = year < 2035 ? 5u : (year < 2045 ? 15u : 25u);
  const uint32_t w3 = year < 2035 ? 10u : 20u, w6 = year < 2035 ? 15u : (year < 2045 ? 10u : 5u);
  const uint32_t total = 15u + 10u + 15u + w3 + offw + offw + w6;
  uint32_t choice = rng_range32(r, lane, total);
  if (choice < 15u) return 0;              choice -= 15u;     // OnshoreWind
  if (choice < 10u) return 3;              choice -= 10u;     // OffshoreWind
  if (choice < 15u) return 12;             choice -= 15u;     // UtilitySolar
  if (choice < w3) return 3 * kBattery;    choice -= w3;
  if (choice < offw) return kFirstOffset;  choice -= offw;    // Forest
  if (choice < offw) return kFirstOffset + 6; choice -= offw; // ActiveCapture
  if (choice < w6) return 21;                                  // GasCombinedCycle
  return 3 * kBattery;
}
__device__ int smart_deficit_fallback(Rng& r, int lane) {   // sampling.rs:492-528: weights 30, 30, 20, 10, 0, 3
  uint32_t choice = rng_range32(r, lane, 93u);
  if (choice < 30u) return 3 * kPeaker;   choice -= 30u;
  if (choice < 30u) return 3 * kBattery;  choice -= 30u;
  if (choice < 20u) return 21;            choice -= 20u;
  if (choice < 10u) return 0;             choice -= 10u;
  if (choice < 3u) return 12;
  return 3 * kBattery;
}
template <bool kUniform>
__device__ int sample_action_weighted(const DevSnapshot& S, Rng& r, Totals& tot, int lane) {   // sampling.rs:147-237
  const bool explore = rng_f64(r, lane) < S.eps_main;
  if (explore) return (int)rng_range64(r, lane, (unsigned long long)EG_N_ACTIONS);
  if (S.stall > 500u) {   // sampling.rs:190-220: stable sort by weight descending, weights raised to power_scaling
    if (!tot.scaled_valid) {   // the row was nudged this year: rebuild the table (otherwise it is the host-built one)
      const double power = S.scaled_power;
      wave_sync();
      if (lane < EG_N_ACTIONS) {   // rank of this entry in the stable descending order; x^p by the shared eg_detpow
        const double mine = SM_W[lane];
        int rank = 0;
#pragma unroll 4
        for (int b = 0; b < EG_N_ACTIONS; ++b) { const double o = SM_W[b]; rank += (o > mine || (o == mine && b < lane)) ? 1 : 0; }
        sm.scaled[rank] = eg_detpow(mine, power);
        sm.ydef[128 + rank] = (uint8_t)lane;
      }
      wave_sync();
      tot.scaled_valid = true;
    }
    const int idx = uni<kUniform>(weighted_pick((int)offsetof(Smem, scaled), EG_N_ACTIONS, rng_f64(r, lane), lane));
    return sm.ydef[128 + (idx < EG_N_ACTIONS ? idx : 0)];
  }
  // Every weight is >= MIN_WEIGHT > 0, so the running value only decreases: the entry at which it first reaches <= 0 is
  // the number of entries after which it was still positive.
  const int pick = uni<kUniform>(weighted_pick((int)offsetof(Smem, pol), EG_N_ACTIONS, rng_f64(r, lane), lane));
  return pick < EG_N_ACTIONS ? pick : 3 * kPeaker;
}
template <bool kUniform>
__device__ int sample_deficit_weighted(const DevSnapshot& S, Rng& r, Totals& tot, int lane) {   // sampling.rs:315-377
  const bool explore = rng_f64(r, lane) < S.exploration_rate;
  if (explore) return 3 * c_deficit_type[(int)rng_range64(r, lane, 14ull)];
  const int pick = uni<kUniform>(weighted_pick((int)(offsetof(Smem, pol) + 8 * snap::kPolDw), 14, rng_f64(r, lane), lane));
  return pick < 14 ? 3 * c_deficit_type[pick] : 3 * kPeaker;
}

struct Episode {   // wave-uniform bookkeeping of one episode
  int ngen, noff;
  int run_pos, def_pos, act_pos;      // flat log cursors
  int n_run_y, n_def_y, n_act_y;      // this year's counts
  int status;
  unsigned long long bytes;           // algorithmic bytes of SURVEY §8(d): whole numbers, kept as an integer (scalar registers)
  int chunks;                         // 64-candidate chunks of sorted candidate records (32 B each) the searches requested
  int heavy;                          // field slot of a heavy episode (place_heavy); -1: not asked for yet, -2: none to be had
  int heavy_classes;                  // bit rc: the field of radius class rc is built and kept up to date
  int heavy_quads;                    // list entries per lane / 4 of the field update (heavy_pack_list)
};

// ---- batch ("reduced") update statistics --------------------------------------------------------------------
// The reference applies apply_contrast_learning / apply_deficit_contrast_learning one episode at a time under a lock
// (multi_simulation.rs:494-508).  For a batch that shares one snapshot the same multiplicative nudges are
// accumulated in log space, as integers (Q32 fixed point), so the result does not depend on the order in which
// episodes, workgroups or ranks contribute: one sum all-reduce of this buffer is the whole exchange.
//   stats[0] episodes ok   [1] episodes failed   [2] episodes that qualify for contrast (learning.rs:160)
//   stats[3] best score of the batch as a sortable integer (bits of the score + 1; one-GPU best pick, see k_apply_update)
//   stats[8 + (y*61+a)]              Σ Q32 ln(penalty_factor)  over occurrences of a in year y that are absent from best
//   stats[8 + 26*61 + (y*61+a)]      Σ Q32 ln(mild_penalty)    over right-action-wrong-slot occurrences (learning.rs:241-251)
//   stats[8 + 2*26*61 + (y*15+s)]    number of deficit actions of slot s in year y absent from best_deficit_actions[y]
constexpr int kStatsMain = EG_YEARS * EG_N_ACTIONS;
constexpr double kQ32 = 4294967296.0;

// The policy's scalars as the kernels use them: always read from the snapshot buffer (snap::state), where the host
// upload or the last on-device update left them.
__device__ __forceinline__ void load_stats_params(const DevSnapshot& S, StatsParams& P) {
  const DevState& st = *S.state();
  P.best_score = st.p_best_score; P.has_best = st.has_lists; P.threshold = st.p_threshold; P.forced = st.p_forced;
  P.adaptive_lr = st.p_adaptive_lr; P.stagnation = st.p_stagnation;
}
// (They are the same in every lane but arrive through vector loads: said to be uniform, they live in scalar registers — as
//  per-lane values the four doubles alone were eight vector registers of the 128 the throughput kernels have, spilled to
//  scratch and reloaded around every nudge.)
__device__ __forceinline__ double uniform_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ void load_state(DevSnapshot& S) {
  const DevState& st = *S.state();
  S.learning_rate = uniform_f64(st.learning_rate); S.exploration_rate = uniform_f64(st.exploration_rate);
  S.stall = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.stall); S.has_best = __builtin_amdgcn_readfirstlane(st.has_best);
  S.has_cw = __builtin_amdgcn_readfirstlane(st.has_cw); S.noop_boost = __builtin_amdgcn_readfirstlane(st.noop_boost);
  S.rel_improvement = uniform_f64(st.rel_improvement); S.immediate_weight = uniform_f64(st.immediate_weight);
  S.has_best_actions = S.has_best_deficit = __builtin_amdgcn_readfirstlane(st.has_lists);
  S.heur_min = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.heur_min); S.heur_max = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.heur_max);
  S.boost_others = uniform_f64(st.boost_others); S.boost_noop = uniform_f64(st.boost_noop);
  S.eps_main = uniform_f64(st.eps_main); S.scaled_power = uniform_f64(st.scaled_power);
  S.lists = S.base + snap::best_mask;      // the resident list (a plan batch's replay kernels then point it at the episode's plan block)
}
// A plan batch (eg_evaluate_plans): episode e replays plan block e.  `e` is wave-uniform, so the list reads stay scalar loads.
__device__ __forceinline__ void plan_lists(DevSnapshot& S, uint32_t e) {
  if (S.plan_pool != nullptr) S.lists = S.plan_pool + (size_t)e * snap::kPlanStride;
}

// One wave adds the contributions of episode e (its outputs must be visible in memory).
// `mult`: the episode stands for that many identical ones (the hoisted replay, eg_replay_coop.h): every sum receives mult times its
// contribution — integers, so that IS adding it mult times.
// `rep` >= 0: `stats` is the replicated form — kStatsReplicas copies, ENTRY-major (copy r of entry i at i * kStatsReplicas + r, so that
// k_fold_stats reads the copies of an entry as one 512-byte line) — and this episode adds to copy `rep`.
__device__ void episode_update_stats(const DevOut& O, const DevSnapshot& S, const StatsParams& P, uint32_t e, int lane, long long* stats,
                                     unsigned long long mult = 1ull, int rep = -1) {
  unsigned long long* const st0 = reinterpret_cast<unsigned long long*>(stats);
  const int stride = rep >= 0 ? kStatsReplicas : 1, ro = rep >= 0 ? rep : 0;
#define st(i_) st0[(size_t)(i_) * stride + ro]
  if (*O.status(e) != EG_EP_OK) {
    if (lane == 0) { atomicAdd(&st(1), mult); *O.score(e) = -1.0; O.score_list[e] = -1.0; }
    return;
  }
  const double score = rm::score(O.metrics(e));
  // slot 3: the batch's best score as an integer that sorts like the score (scores are not negative; + 1 so that 0 means
  // "no successful episode"): with one GPU k_apply_update finds the best episode from it without a kernel of its own
  if (lane == 0) { atomicAdd(&st(0), mult); *O.score(e) = score; O.score_list[e] = score; atomicMax(&st(3), (unsigned long long)__double_as_longlong(score) + 1ull); }
  if (!P.has_best) return;
  const double det = P.best_score > 0.0 ? (P.best_score - score) / P.best_score : 0.0;
  const bool qualifies = det > P.threshold || P.forced;                                               // learning.rs:160
  unsigned long long q_pen = 0, q_mild = 0;
  if (qualifies) {
    if (lane == 0) atomicAdd(&st(2), mult);
    if (det < 0.0) {      // forced contrast on an episode that beats the best: powf(negative, 0.3) is NaN in the reference and
                          // (w * NaN).max(MIN_WEIGHT) == MIN_WEIGHT — in log space any exponent below -9.2 (eg_reduced_math.h)
      q_pen = q_mild = (unsigned long long)(long long)(rm::kLnNanPenalty * kQ32);
    } else {              // det == 0: pow gives 0, both factors are 1 and only the boost remains
      const double combined = pow(det, 0.3) * P.stagnation;                                            // learning.rs:168-171
      // (the two logarithms side by side — lane 1 the mild one's argument, every other lane the penalty's: one evaluation of `log`,
      //  ~190 vector instructions, instead of two; the same operations on the same operands in the lanes that are read)
      const double arg_pen = P.adaptive_lr * 1.5 * combined;       // learning.rs:177
      const double arg_mild = P.adaptive_lr * combined * 0.5;      // learning.rs:247
      const long long q = llrint(log(1.0 / (1.0 + (lane == 1 ? arg_mild : arg_pen))) * kQ32);
      q_pen = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(q >> 32), 0) << 32) | (unsigned)__builtin_amdgcn_readlane((int)q, 0);
      q_mild = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(q >> 32), 1) << 32) | (unsigned)__builtin_amdgcn_readlane((int)q, 1);
    }
  }
  // The items are the entries of every year's `current = run ++ deficit` list (learning.rs:196-211), position j of year y against
  // position j of `best ++ best_deficit` of that year.  Flattened over the years — a lane an item — so that the episode's lists are
  // read in two memory round trips (the items and the best lists' offsets / masks of their years, then the best-list entries they
  // are compared with) instead of two per year: this runs at the end of every episode of a training batch, behind nothing to hide it.
  const uint8_t* run = O.run_log(e);
  const uint8_t* def = O.def_log(e);
  int nr = 0, nd = 0;      // lane y: the year's counts
  if (lane < EG_YEARS) { nr = O.n_run(e)[lane]; nd = O.n_def(e)[lane]; }
  // exclusive prefix sums over the years (lane y: where year y starts in run_log, in def_log); items of year y start at rp + dp
  int rp = nr, dp = nd;
#pragma unroll
  for (int sh = 1; sh < 32; sh <<= 1) {
    const int ur = __shfl_up(rp, sh), ud = __shfl_up(dp, sh);
    if (lane >= sh) { rp += ur; dp += ud; }
  }
  const int total = __builtin_amdgcn_readlane(rp, EG_YEARS - 1) + __builtin_amdgcn_readlane(dp, EG_YEARS - 1);
  rp -= nr; dp -= nd;
  const int ip = rp + dp;
  q_pen *= mult; q_mild *= mult;      // (two's-complement products: the sum of mult equal terms)
  for (int base = 0; base < total; base += kWave) {
    const int i = base + lane;
    int y = 0;      // the year of item i: the last year that starts at or before it (empty years share their start with the next one)
#pragma unroll
    for (int yy = 1; yy < EG_YEARS; ++yy) y = i >= __builtin_amdgcn_readlane(ip, yy) ? yy : y;
    // (every lane takes part in the shuffles: a lane masked off would not lend its year's values to the others)
    const int j = i - __shfl(ip, y), nr_y = __shfl(nr, y), rp_y = __shfl(rp, y), dp_y = __shfl(dp, y);
    const bool valid = i < total;
    int a = 0;
    unsigned long long mask = 0, dmask = 0; int b0 = 0, nb = 0, d0 = 0, nbd = 0;
    if (valid) {
      a = j < nr_y ? run[rp_y + j] : def[dp_y + (j - nr_y)];
      mask = S.best_mask()[y]; dmask = S.bestd_mask()[y];
      b0 = S.best_off()[y]; nb = S.best_off()[y + 1] - b0; d0 = S.bestd_off()[y]; nbd = S.bestd_off()[y + 1] - d0;
    }
    if (valid && qualifies) {
      if (!((mask >> a) & 1ull)) atomicAdd(&st(8 + y * EG_N_ACTIONS + a), q_pen);
      else if (j < nb + nbd) {
        const int b = j < nb ? S.best_actions()[b0 + j] : S.bestd_actions()[d0 + (j - nb)];
        if (a != b) atomicAdd(&st(8 + kStatsMain + y * EG_N_ACTIONS + a), q_mild);
      }
    }
    if (valid && j >= nr_y && !((dmask >> a) & 1ull)) {        // learning.rs:346-352
      const int slot = (a < kFirstOffset && a % 3 == 0) ? c_deficit_slot[a / 3] : (a == kNothing ? 14 : -1);
      if (slot >= 0) atomicAdd(&st(8 + 2 * kStatsMain + y * EG_N_DEFICIT + slot), mult);
    }
  }
#undef st
}

#ifdef EG_STAMPS
// every cycle of the episode is attributed: a mark charges the time since the previous mark to `slot`
#define EG_MARK(slot) do { const unsigned long long now_ = __builtin_readcyclecounter(); stamps[slot] += now_ - last_; last_ = now_; } while (0)
#define EG_MARKG(slot) EG_MARK(slot)
#define EG_T0() EG_MARK(6)
#define EG_T1(slot) EG_MARK(slot)
#define EG_TB(slot) EG_MARK(6)
#define EG_TE(slot) EG_MARK(slot)
#else
#define EG_T0() do {} while (0)
#define EG_T1(slot) do {} while (0)
#define EG_TB(slot) do {} while (0)
#define EG_MARKG(slot) do {} while (0)
#define EG_TE(slot) do {} while (0)
#endif

// Which episode of the batch a workgroup runs.  A batch is launched as up to three grids that run side by side on two
// streams: the episodes that replay the best strategy — the ones that grow long generator lists, SURVEY Q15 — on the
// replay variants of the kernel (kReplayLong: approximate-field placement from kHeavyGens generators on; kReplayShort: the
// exact scan, for short lists; see k_rollout), all others on the lean
// variant, whose code and registers are those of a kernel without the heavy path (measured: with the heavy calls compiled
// into the one kernel, sampled episodes ran 8 % / 13 % slower at 1 024 / 16 384 episodes).
struct EpisodeMap {
  const uint32_t* index;      // mode 1: episode = index[workgroup]
  uint32_t mode;              // 0: the workgroup index; 2: off + period * workgroup (the replays of a period); 3: the others
  uint32_t count, off, period;
  // replay hoist (eg_replay_coop.h): when *hoist carries this launch's sequence number, k_replay_coop has computed the batch's replay
  // episodes once and k_replay_broadcast hands every one of them the record: the replay variants have nothing to do (0: no hoist)
  const unsigned long long* hoist;
  unsigned long long hoist_seq;
  uint32_t stats_rep;         // 1: `stats` is kStatsReplicas copies of the statistics array (entry-major); this workgroup adds to copy (index % kStatsReplicas)
  // a plan-edit batch with same_index (eg_evaluate_plan_edits): 1 = every episode of this plan batch draws from the stream of global
  // episode first_index.  Read by the replay variants in a plan batch only.  (In the four bytes of padding in front of `solo`: the
  // argument block of every k_rollout keeps its layout.)
  uint32_t same_index;
  // per-episode replay kernel (eg_replay_solo.h): word b carries solo_seq when k_replay_solo has completed workgroup b's episode — the
  // long-replay variant, launched behind it, then has nothing to do for that episode (0 / null: no such kernel in this launch) —, and
  // solo_seq << 21 | 1 << 20 | slot when it gave the episode up holding field slot `slot`: the long-replay variant runs it in that slot
  unsigned long long* solo;
  unsigned long long solo_seq;
};
__device__ __forceinline__ uint32_t map_episode(const EpisodeMap& m, uint32_t b) {
  if (m.mode == 0u) return b;
  if (m.mode == 1u) return m.index[b];
  if (m.mode == 2u) return m.off + m.period * b;
  if (b < m.off) return b;
  const uint32_t q = b - m.off, p1 = m.period - 1u;
  return m.off + (q / p1) * m.period + 1u + q % p1;
}

// (the heavy-capable variant: four waves per SIMD in the throughput kernel — 128 VGPRs, the field code held to 72 by
//  k_heavy_register_budget, the year's aggregates parked in LDS around its calls —, two in the small-batch kernel — 256 VGPRs)
// kKind: kLean = sampled episodes only (no replay code at all); kReplayShort / kReplayLong = the episodes that replay the best
// strategy, on the lean kernel's budget while the replayed list is short and on the heavy-capable variant once it is long.
// Both are launched over the replay episodes of a batch and the one whose turn it is not returns at once: how long the list
// is only the device knows (an on-device update may have replaced it since the host last looked), and the host plans
// launches many batches ahead of the device.
constexpr int kLean = 0, kReplayShort = 1, kReplayLong = 2;
// This file is compiled twice (csrc/Makefile).  eg_rollout.o holds the small-batch kernels (an episode wave and a helper wave) and
// everything that is not a rollout; eg_rollout_tp.o (-DEG_TU_THROUGHPUT) holds the three throughput kernels k_rollout<0, kind>,
// compiled WITHOUT machine-code loop-invariant code motion.  Out of the year and action loops that pass hoists literal constants and
// table addresses into registers — which are then live for the whole episode and across the calls of the field code: the long-replay
// variant takes 157 vector registers with it and 126 without, i.e. four waves per SIMD instead of two (with its aggregates parked in
// LDS around those calls and the field code held to 72 registers, k_heavy_register_budget), so that two long replays leave a SIMD room
// for two lean waves; the lean variant takes 120 instead of 128 + a spill.  Measured (profiles/r03_ab_notes.log): the sustained batch
// 3.07 -> 2.62 ms; 16 384 sampled episodes alone +1.3 %, the seeded batch +1.1 %; the small-batch kernel would lose 3.6 % and keeps
// the pass: hence two objects, and not a flag for the file.
#ifdef EG_TU_THROUGHPUT
#define EG_HEAVY_WAVES 4
#else
#define EG_HEAVY_WAVES 2
#endif
// actions in the best list up to which replay episodes stay on the exact scan (measured at 16 384 x 10 %: a batch with an
// 82-action list — 90 generators per replay episode — takes 2.02 ms this side of the limit and 2.37 ms on the other, one
// with a 109-action list — 117 generators — 2.39 against 2.25)
// (kShortReplayMax = 96, eg_internal.h)
template <int kHelpers, int kKind>
__global__ void __launch_bounds__(kWave * (1 + kHelpers), kKind == kReplayLong ? (kHelpers > 0 ? 2 : EG_HEAVY_WAVES) : (kHelpers > 0 ? 3 : 4)) k_rollout(DevTables T, DevSnapshot S_in, DevOut O, unsigned long long seed,
                                                                    unsigned long long first_index, uint32_t n_episodes,
                                                                    const uint8_t* __restrict__ replay_mask, uint32_t replay_period,
                                                                    long long* stats, EpisodeMap emap) {
#define EG_EPISODE_UNIFORM false
#include "eg_rollout_episode.h"      // the episode: one text under two kernels
#undef EG_EPISODE_UNIFORM
}

#ifdef EG_TU_THROUGHPUT
// The lean and the short-replay kind with the episode's control state uniform (eg_rollout_episode.h, kUniform): what a throughput batch
// launches for them (launch_rollout_throughput; EIRGRID_UNIFORM=0: k_rollout<0, kind>).  Launch bounds, LDS and arguments are k_rollout's.
template <int kKind>
__global__ void __launch_bounds__(kWave, 4) k_episodes(DevTables T, DevSnapshot S_in, DevOut O, unsigned long long seed,
                                                       unsigned long long first_index, uint32_t n_episodes,
                                                       const uint8_t* __restrict__ replay_mask, uint32_t replay_period,
                                                       long long* stats, EpisodeMap emap) {
  static_assert(kKind == kLean || kKind == kReplayShort, "the long-replay kind stays k_rollout<0, kReplayLong>");
  constexpr int kHelpers = 0;
#define EG_EPISODE_UNIFORM true
#include "eg_rollout_episode.h"
#undef EG_EPISODE_UNIFORM
}

// Never launched.  A device function's register budget is the tightest launch bound among the kernels that can reach it, and the
// attributes that would say so directly are for kernels only: this kernel's bound of seven waves per SIMD gives the long-replay
// variant's field code 72 registers, which — with the episode's aggregates parked in LDS around those calls — is what lets that
// variant run four waves per SIMD (128 registers) beside the lean grid.
__global__ void __launch_bounds__(kWave, 7) k_heavy_register_budget(unsigned long long a, unsigned long long b, unsigned long long c, double d, int i, int* out) {
  const int lane = threadIdx.x;
  int r = place_heavy<false>(a, b, c, a + b, b + c, d, lane, i, i, i);
  r += place_exact_long<false>(a, c, d, lane, i, i, i);
  heavy_build_class<false>(a, c, lane, i, i, i, i);
  out[lane] = r;
}
#endif

#include "eg_replay_script.h"      // a replay episode's script and yearly rows (both objects)
#ifdef EG_TU_THROUGHPUT
#include "eg_replay_solo.h"        // k_replay_solo: a long replay episode on its own wave, script / placements / rows one after the other
#endif

#ifndef EG_TU_THROUGHPUT      // (everything from here to the launchers lives in eg_rollout.o only)
#include "eg_replay_coop.h"      // k_replay_coop, k_replay_broadcast: the replay episodes of a batch, computed once
#include "eg_topk.h"             // k_topk_keys, k_topk_select, k_topk_merge: the top-K archive of distinct scenarios
#include "eg_pareto.h"           // k_pareto_filter .. k_pareto_finalize: the Pareto archive of a run's outcomes
#include "eg_plan_block.h"       // pblock: the plan-block layout and what the four kernels that write plan blocks share
#include "eg_plan_edits.h"       // k_plan_edits: the plan blocks of a plan-edit batch from one base block and an edit per variant
#include "eg_pick.h"             // refine::wave_best, pick_segment: the pick that ends a round, whatever the rule
#include "eg_refine_many.h"      // k_plan_edits_many, k_refine_pick_many: a refinement round, a segment of the launch's variants per plan
#include "eg_plan_moves.h"       // k_plan_moves: the plan blocks of the variants that move an entry to another year
#include "eg_plan_crosses.h"     // k_plan_crosses: the plan blocks of the variants that splice one parent's years into another
#include "eg_plan_rewrites.h"    // k_plan_rewrites: the plan blocks of the variants that apply an action map to a window of years
#include "eg_plan_constraints.h" // k_plan_constraints: the context's plan constraints judged over a plan batch's records
#include "eg_repair.h"           // k_repair_pick_many: the pick of a repair round, by the violation k_plan_constraints measured
#include "eg_build_constraints.h" // k_build_constraints: row and build constraints judged in one pass, where a build constraint is set
#include "eg_ensemble.h"          // k_ensemble_keep, k_ensemble_commit: a plan batch judged over R draw streams, a lane a stream
#include "eg_breed.h"            // k_breed_gather, k_breed_turnover: a generation's survivors become the next one's parents on the device
#include "eg_explore.h"          // k_explore_turnover: the members that entered an exploration's archive become the next frontier

#include "eg_update_kernels.h"
#endif      // EG_TU_THROUGHPUT
}  // namespace

// the throughput kernels (one wave per episode), from their own object (see the top of the kernel section)
int launch_rollout_throughput(int kind, bool classic, const DevTables& t, const DevSnapshot& s, const DevOut& o, uint64_t seed, uint64_t first_index, uint32_t n,
                              const uint8_t* d_replay_mask, uint32_t replay_period, long long* d_stats, uint32_t count, uint32_t mode,
                              const uint32_t* index, uint32_t off, uint32_t period, const unsigned long long* hoist, unsigned long long hoist_seq,
                              uint32_t stats_rep, uint32_t same_index, unsigned long long* solo, unsigned long long solo_seq, void* stream, void* ev0, void* ev1);
#ifdef EG_TU_THROUGHPUT
int launch_rollout_throughput(int kind, bool classic, const DevTables& t, const DevSnapshot& s, const DevOut& o, uint64_t seed, uint64_t first_index, uint32_t n,
                              const uint8_t* d_replay_mask, uint32_t replay_period, long long* d_stats, uint32_t count, uint32_t mode,
                              const uint32_t* index, uint32_t off, uint32_t period, const unsigned long long* hoist, unsigned long long hoist_seq,
                              uint32_t stats_rep, uint32_t same_index, unsigned long long* solo, unsigned long long solo_seq, void* stream, void* ev0, void* ev1) {
  EpisodeMap map{};
  map.count = count; map.mode = mode; map.index = index; map.off = off; map.period = period; map.hoist = hoist; map.hoist_seq = hoist_seq; map.stats_rep = stats_rep; map.same_index = same_index;
  map.solo = solo; map.solo_seq = solo_seq;
  // the timing events ride on the dispatch packet itself (no separate barrier packets around the kernel)
#define EG_LAUNCH_TP(kKind) hipExtLaunchKernelGGL((k_rollout<0, kKind>), dim3(map.count), dim3(kWave), 0, (hipStream_t)stream, (hipEvent_t)ev0, (hipEvent_t)ev1, 0, \
                                                  t, s, o, (unsigned long long)seed, (unsigned long long)first_index, n, d_replay_mask, replay_period, d_stats, map)
  if (kind == kReplayLong) {
    // every long replay episode on its own wave, script / placements / rows one after the other (eg_replay_solo.h); the classic variant
    // behind it runs what that kernel left undone (a script that needs a seeded draw or hits a capacity) and carries the stop event
    if (solo_seq != 0ull && t.solo_tiles != 0u && t.solo_lazy != 0u)
      hipLaunchKernelGGL(k_replay_lazy, dim3(map.count), dim3(kWave), 0, (hipStream_t)stream, t, s, o, (unsigned long long)first_index, n, d_replay_mask, replay_period,
                         d_stats, map);
    else if (solo_seq != 0ull)
      hipLaunchKernelGGL(k_replay_solo, dim3(map.count), dim3(kWave), 0, (hipStream_t)stream, t, s, o, (unsigned long long)first_index, n, d_replay_mask, replay_period,
                         d_stats, map);
    EG_LAUNCH_TP(kReplayLong);
  }
  // the lean and the short-replay kind: k_episodes, the same episode with its control state uniform (classic: EIRGRID_UNIFORM=0, the k_rollout they were)
#define EG_LAUNCH_UNI(kKind) hipExtLaunchKernelGGL((k_episodes<kKind>), dim3(map.count), dim3(kWave), 0, (hipStream_t)stream, (hipEvent_t)ev0, (hipEvent_t)ev1, 0, \
                                                   t, s, o, (unsigned long long)seed, (unsigned long long)first_index, n, d_replay_mask, replay_period, d_stats, map)
  else if (kind == kReplayShort) { if (classic) EG_LAUNCH_TP(kReplayShort); else EG_LAUNCH_UNI(kReplayShort); }
  else { if (classic) EG_LAUNCH_TP(kLean); else EG_LAUNCH_UNI(kLean); }
#undef EG_LAUNCH_UNI
#undef EG_LAUNCH_TP
  return (int)hipGetLastError();
}
// test hook (eg_debug_tiles_refresh): one wave; `tile_b` -1: the lone last tile of a round.  The caller has checked the tiles, the class
// and the cells; the field is a class's kFieldStride doubles.
int launch_debug_tiles_refresh(const DevTables& t, double* d_field, const uint16_t* d_cells, int n_cells, int radius_class, int tile_a, int tile_b, int* d_out, void* stream) {
  static_assert(kFieldStride == EG_DEBUG_FIELD_DOUBLES && kTileCounters == EG_DEBUG_TILE_COUNTERS && kTiles == EG_DEBUG_TILES && kTileW == EG_DEBUG_TILE_WIDTH,
                "the class field is what the hook documents");
  hipLaunchKernelGGL(k_debug_tiles_refresh, dim3(1), dim3(kWave), 0, (hipStream_t)stream, t, (unsigned long long)d_field, (unsigned long long)d_cells, n_cells, radius_class,
                     tile_a, tile_b < 0 ? kNoTile : tile_b, d_out);
  return (int)hipGetLastError();
}
#else
namespace {
template <int kKind>
void launch_variant(bool helper_waves, bool classic, const DevTables& t, const DevSnapshot& s, const DevOut& o, uint64_t seed, uint64_t first_index, uint32_t n,
                    const uint8_t* d_replay_mask, uint32_t replay_period, long long* d_stats, const EpisodeMap& map, void* stream, void* ev0, void* ev1) {
  if (helper_waves)
    hipExtLaunchKernelGGL((k_rollout<kHelperWaves, kKind>), dim3(map.count), dim3(kWave * (1 + kHelperWaves)), 0, (hipStream_t)stream,
                          (hipEvent_t)ev0, (hipEvent_t)ev1, 0, t, s, o, (unsigned long long)seed, (unsigned long long)first_index, n,
                          d_replay_mask, replay_period, d_stats, map);
  else
    (void)launch_rollout_throughput(kKind, classic, t, s, o, seed, first_index, n, d_replay_mask, replay_period, d_stats, map.count, map.mode, map.index, map.off, map.period,
                                    map.hoist, map.hoist_seq, map.stats_rep, map.same_index, map.solo, map.solo_seq, stream, ev0, ev1);
}
}  // namespace

int launch_rollout(const DevTables& t, const DevSnapshot& s, const DevOut& o, uint64_t seed, uint64_t first_index,
                   uint32_t n, const uint8_t* d_replay_mask, uint32_t replay_period, long long* d_stats_packet, const RolloutPlan& p) {
  if (n == 0) return 0;
  // the statistics go to the replicated array when the plan brings one (k_fold_stats, launched by the caller behind the grids, folds it
  // into the packet)
  const bool rep = d_stats_packet != nullptr && p.d_stats_rep != nullptr;
  long long* d_stats = rep ? p.d_stats_rep : d_stats_packet;
  if (p.plans) {      // each replay variant over exactly its plans (the kernels then skip their grid-uniform list-length test)
    EpisodeMap ms{}, ml{};
    ms.count = p.n_short; ms.mode = 1u; ms.index = p.d_index;
    ml.count = p.n_heavy - p.n_short; ml.mode = 1u; ml.index = p.d_index_long;
    ms.same_index = ml.same_index = p.same_index ? 1u : 0u;      // (k_rollout: every episode draws from the stream of first_index)
    if (!p.helper_waves && p.solo_seq != 0ull) { ml.solo = p.d_solo; ml.solo_seq = p.solo_seq; }
    if (ms.count > 0) launch_variant<kReplayShort>(p.helper_waves, p.classic_kernels, t, s, o, seed, first_index, n, d_replay_mask, replay_period, d_stats, ms, p.stream_heavy, p.ev[0],
                                                   ml.count > 0 ? nullptr : p.ev[1]);
    else (void)hipEventRecord((hipEvent_t)p.ev[0], (hipStream_t)p.stream_heavy);      // (k_replay_solo runs first: the start is a marker)
    if (ml.count > 0) launch_variant<kReplayLong>(p.helper_waves, p.classic_kernels, t, s, o, seed, first_index, n, d_replay_mask, replay_period, d_stats, ml, p.stream_heavy, nullptr, p.ev[1]);
    return (int)hipGetLastError();
  }
  if (p.n_heavy > 0) {      // first, so that the long episodes start first: both replay variants, one of which returns at once
    EpisodeMap m{};
    m.count = p.n_heavy; m.stats_rep = rep ? 1u : 0u;
    if (p.n_lean == 0) m.mode = 0u;
    else if (p.mode == 1u) { m.mode = 1u; m.index = p.d_index; }
    else { m.mode = 2u; m.off = p.off; m.period = p.period; }
    if (!p.helper_waves && p.solo_seq != 0ull) { m.solo = p.d_solo; m.solo_seq = p.solo_seq; }
    const bool hoist = p.hoist_seq != 0ull;
    if (hoist) {
      // Replay hoist: ONE workgroup computes the batch's replay script and its placements (k_replay_coop, EG_COOP_WAVES waves with the whole
      // register file and LDS of a CU — it must be dispatched BEFORE the lean grid fills every CU: the lean grid's stream waits for an
      // event recorded right in front of it), k_replay_books the yearly rows; the per-episode variants follow and return at once when
      // that has succeeded, k_replay_broadcast hands out the record.
      m.hoist = reinterpret_cast<const unsigned long long*>(p.d_hoist); m.hoist_seq = p.hoist_seq;      // (HoistInfo::served_seq comes first)
      if (p.go_event && p.n_lean > 0) {
        (void)hipEventRecord((hipEvent_t)p.go_event, (hipStream_t)p.stream_heavy);
        (void)hipStreamWaitEvent((hipStream_t)p.stream_lean, (hipEvent_t)p.go_event, 0);
      }
      const DevOut scratch{p.coop_out, reinterpret_cast<double*>(p.coop_out + rec::stride)};
      hipExtLaunchKernelGGL(k_replay_coop, dim3(1), dim3(coop::kThreads), 0, (hipStream_t)p.stream_heavy, (hipEvent_t)p.ev[0], nullptr, 0,
                            t, s, scratch, p.hoist_seq, p.d_hoist, p.coop_force);
      hipLaunchKernelGGL(k_replay_books, dim3(EG_YEARS), dim3(kWave), 0, (hipStream_t)p.stream_heavy, t, s, scratch, p.hoist_seq, p.d_hoist, d_stats, p.n_heavy, rep ? 1 : 0);
    }
    // (the short one first: when it is the one that returns at once it finds the chip empty and is gone in microseconds; a
    //  256-register wave of the long one, when IT has nothing to do, must wait until a SIMD full of lean waves has drained two
    //  of them, and whatever is queued behind it on the stream waits with it — measured: 0.6 ms)
    launch_variant<kReplayShort>(p.helper_waves, p.classic_kernels, t, s, o, seed, first_index, n, d_replay_mask, replay_period, d_stats, m, p.stream_heavy, hoist ? nullptr : p.ev[0], nullptr);
    if (!hoist && p.go_event && p.n_lean > 0) {
      (void)hipEventRecord((hipEvent_t)p.go_event, (hipStream_t)p.stream_heavy);
      (void)hipStreamWaitEvent((hipStream_t)p.stream_lean, (hipEvent_t)p.go_event, 0);
    }
    // (the short variant's launch carries the start event, the long one's the stop event; without the long one a marker does)
    if (!p.skip_long) launch_variant<kReplayLong>(p.helper_waves, p.classic_kernels, t, s, o, seed, first_index, n, d_replay_mask, replay_period, d_stats, m, p.stream_heavy, nullptr, hoist ? nullptr : p.ev[1]);
    else if (!hoist) (void)hipEventRecord((hipEvent_t)p.ev[1], (hipStream_t)p.stream_heavy);
    if (hoist) {
      const DevOut scratch{p.coop_out, reinterpret_cast<double*>(p.coop_out + rec::stride)};
      hipExtLaunchKernelGGL(k_replay_broadcast, dim3(m.count), dim3(kWave), 0, (hipStream_t)p.stream_heavy, nullptr, (hipEvent_t)p.ev[1], 0,
                            s, scratch, o, n, d_stats != nullptr ? 1 : 0, m, (const HoistInfo*)p.d_hoist, p.hoist_seq);
    }
  }
  if (p.n_lean > 0) {
    EpisodeMap m{};
    m.count = p.n_lean; m.stats_rep = rep ? 1u : 0u;
    if (p.n_heavy == 0) m.mode = 0u;
    else if (p.mode == 1u) { m.mode = 1u; m.index = p.d_index + p.n_heavy; }
    else { m.mode = 3u; m.off = p.off; m.period = p.period; }
    launch_variant<kLean>(p.helper_waves, p.classic_kernels, t, s, o, seed, first_index, n, d_replay_mask, replay_period, d_stats, m, p.stream_lean, p.ev[2], p.ev[3]);
  }
  return (int)hipGetLastError();
}
// The replicated statistics of a batch into its packet (sums; slot 3 is a maximum), and the copies cleared for the next batch: a wave
// an entry — its 64 copies are one 512-byte line.
__global__ void __launch_bounds__(256) k_fold_stats(long long* rep, long long* stats) {
  static_assert(kStatsReplicas == kWave, "a lane a copy");
  const int lane = threadIdx.x & (kWave - 1);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= EG_STATS_LEN) return;
  unsigned long long v = (unsigned long long)rep[(size_t)i * kStatsReplicas + lane];
  rep[(size_t)i * kStatsReplicas + lane] = 0;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, sh);
    v = i == 3 ? (o > v ? o : v) : v + o;
  }
  if (lane == 0) {
    const unsigned long long old = (unsigned long long)stats[i];
    stats[i] = (long long)(i == 3 ? (v > old ? v : old) : old + v);
  }
}
int launch_fold_stats(long long* d_rep, long long* d_stats, void* stream) {
  hipLaunchKernelGGL(k_fold_stats, dim3((EG_STATS_LEN + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_rep, d_stats);
  return (int)hipGetLastError();
}
int launch_place(const DevTables& t, int gen_type, int year_index, const uint16_t* d_cells, int n_extra,
                 int32_t* d_out_cell, double* d_out_score, void* stream) {
  hipLaunchKernelGGL(k_place, dim3(1), dim3(kWave), 0, (hipStream_t)stream, t, gen_type, year_index, d_cells, n_extra,
                     d_out_cell, d_out_score);
  return (int)hipGetLastError();
}
int launch_place_xy(const DevTables& t, int gen_type, int year_index, const double* d_x, const double* d_y, int n, double radius,
                    double size_term, int32_t* d_out_cell, double* d_out_score, void* stream) {
  hipLaunchKernelGGL(k_place_xy, dim3(1), dim3(kWave), 0, (hipStream_t)stream, t, gen_type, year_index, d_x, d_y, n, radius, size_term,
                     d_out_cell, d_out_score);
  return (int)hipGetLastError();
}
// Test hook: leaves `value` in every LDS word a later workgroup can be handed (tests/test_gpu_parity.py uses it to show
// that no kernel reads LDS it has not written).  One workgroup of 64 KB per slot, enough of them to cover every CU.
__global__ void __launch_bounds__(256) k_fill_lds(uint32_t value, uint32_t* sink) {
  __shared__ uint32_t words[16384];
  for (int i = threadIdx.x; i < 16384; i += 256) words[i] = value;
  __syncthreads();
  if (words[(threadIdx.x * 61u + blockIdx.x) & 16383u] != value) *sink = 1u;      // keeps the stores alive
}
// Diagnostic (eg_debug_occupy; scripts/side_kernel_probe.py): ONE workgroup that holds `kBytes` of LDS and its registers for `cycles` shader
// cycles and does nothing — what does a resident workgroup of that footprint cost the grid that runs beside it?
template <int kBytes, int kRegs, int kBusy = 0>
__global__ void __launch_bounds__(256, 1) k_occupy(unsigned long long cycles, uint32_t* sink) {
  __shared__ uint32_t words[kBytes / 4];
  double r[kRegs];
#pragma unroll
  for (int i = 0; i < kRegs; ++i) r[i] = (double)(threadIdx.x + i);
  words[threadIdx.x] = threadIdx.x;
  const unsigned long long t0 = __builtin_readcyclecounter();
  while (__builtin_readcyclecounter() - t0 < cycles) {
#pragma unroll
    for (int i = 0; i < kRegs; ++i) r[i] = r[i] * 1.0000001 + (double)words[(threadIdx.x + i) & 255];
    if (kBusy == 0) __builtin_amdgcn_s_sleep(8);
    if (kBusy >= 2) { words[(threadIdx.x * 7 + 1) & 255] = (uint32_t)r[0]; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
  }
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < kRegs; ++i) acc += r[i];
  if (acc == 12345.678) *sink = 1u;      // keeps the registers alive
}
int launch_occupy(int variant, unsigned long long cycles, uint32_t* d_sink, void* stream) {
  if (variant == 0) hipLaunchKernelGGL((k_occupy<1024, 4>), dim3(1), dim3(256), 0, (hipStream_t)stream, cycles, d_sink);            // small in every way
  else if (variant == 1) hipLaunchKernelGGL((k_occupy<150 * 1024, 4>), dim3(1), dim3(256), 0, (hipStream_t)stream, cycles, d_sink);  // the whole LDS of a CU
  else if (variant == 2) hipLaunchKernelGGL((k_occupy<1024, 100>), dim3(1), dim3(256), 0, (hipStream_t)stream, cycles, d_sink);       // 200+ registers a lane
  else if (variant == 3) hipLaunchKernelGGL((k_occupy<150 * 1024, 100>), dim3(1), dim3(256), 0, (hipStream_t)stream, cycles, d_sink);  // both
  else if (variant == 4) hipLaunchKernelGGL((k_occupy<150 * 1024, 100, 1>), dim3(1), dim3(256), 0, (hipStream_t)stream, cycles, d_sink);  // both, busy (no sleep)
  else hipLaunchKernelGGL((k_occupy<150 * 1024, 100, 2>), dim3(1), dim3(256), 0, (hipStream_t)stream, cycles, d_sink);                   // both, busy, LDS writes and barriers
  return (int)hipGetLastError();
}
int launch_fill_lds(uint32_t value, uint32_t* d_sink, int n_workgroups, void* stream) {
  hipLaunchKernelGGL(k_fill_lds, dim3(n_workgroups), dim3(256), 0, (hipStream_t)stream, value, d_sink);
  return (int)hipGetLastError();
}
__global__ void __launch_bounds__(1024) k_rewind(uint8_t* snap_base, const uint8_t* held, uint32_t* list_len_out) {
  static_assert(snap::total % 16 == 0 && (snap::state + offsetof(DevState, failed_total)) % 4 == 0, "snapshot layout");
  constexpr uint32_t kFailedWord = (uint32_t)((snap::state + offsetof(DevState, failed_total)) / 4);
  const uint32_t failed = reinterpret_cast<const uint32_t*>(snap_base)[kFailedWord];
  __syncthreads();      // (one workgroup: everybody has read the counter before anybody overwrites it)
  const uint4* src = reinterpret_cast<const uint4*>(held);
  uint4* dst = reinterpret_cast<uint4*>(snap_base);
  for (uint32_t i = threadIdx.x; i < (uint32_t)(snap::total / 16); i += 1024u) dst[i] = src[i];
  __syncthreads();
  if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(snap_base)[kFailedWord] = failed;
  if (threadIdx.x == 64 && list_len_out) {
    const DevState* hs = reinterpret_cast<const DevState*>(held + snap::state);
    const uint32_t len = hs->has_lists ? (uint32_t)reinterpret_cast<const int32_t*>(held + snap::best_off)[EG_YEARS] : 0u;
    __hip_atomic_store(list_len_out, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
int launch_rewind(uint8_t* d_snap, const uint8_t* d_held, uint32_t* list_len_out, void* stream) {
  hipLaunchKernelGGL(k_rewind, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_snap, d_held, list_len_out);
  return (int)hipGetLastError();
}
int launch_stalled_tables(uint8_t* d_snap, void* stream) {
  hipLaunchKernelGGL(k_stalled_tables, dim3(EG_YEARS), dim3(kWave), 0, (hipStream_t)stream, d_snap);
  return (int)hipGetLastError();
}
int launch_apply_update(uint8_t* d_snap, const void* d_packets, int n_packets, size_t packet_stride, long long* d_zero_stats, uint64_t noise_seed,
                        const DevOut& o, uint32_t n_local, uint64_t first_index, bool local_pick, uint32_t* list_len_out, void* stream) {
  hipLaunchKernelGGL(k_apply_update, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_snap, (const uint8_t*)d_packets, n_packets,
                     (unsigned long long)packet_stride, d_zero_stats, (unsigned long long)noise_seed, (const uint8_t*)o.base, (const double*)o.score_list, n_local, (unsigned long long)first_index,
                     local_pick ? 1 : 0, list_len_out);
  return (int)hipGetLastError();
}
int launch_update_stats(const DevSnapshot& s, const DevOut& o, uint32_t n, long long* d_stats, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_update_stats, dim3(n), dim3(kWave), 0, (hipStream_t)stream, o, s, n, d_stats);
  return (int)hipGetLastError();
}
int launch_fold_best(const DevOut& o, uint32_t n, uint64_t first_index, bool cost_only, uint8_t* d_fold, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_fold_best, dim3(1), dim3(1024), 0, (hipStream_t)stream, o, n, (unsigned long long)first_index, cost_only ? 1 : 0, d_fold);
  return (int)hipGetLastError();
}
int launch_fold_pack(const DevOut& o, uint32_t n, uint8_t* d_packet, FoldEntry* block, void* stream) {
  if (n > 0 && block == nullptr) return 0;
  hipLaunchKernelGGL(k_fold_pack, dim3(n > 0 ? (n + 255u) / 256u : 1u), dim3(256), 0, (hipStream_t)stream, o, n, d_packet, block);
  return (int)hipGetLastError();
}
int launch_fold_gathered(const uint8_t* d_gathered, size_t slot_stride, int n_ranks, uint32_t n_global, uint64_t first_index, const DevOut& o,
                         uint32_t own_first, uint32_t own_n, bool cost_only, uint32_t step, uint8_t* d_fold, void* stream) {
  if (n_global == 0) return 0;
  hipLaunchKernelGGL(k_fold_gathered, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_gathered, (unsigned long long)slot_stride, n_ranks, n_global,
                     (unsigned long long)first_index, o, own_first, own_n, cost_only ? 1 : 0, step, d_fold);
  return (int)hipGetLastError();
}
int launch_topk_keys(const DevOut& o, uint32_t n, uint64_t first_index, int mode, bool use_score_list, const uint8_t* d_state,
                     double* d_score, unsigned long long* d_key, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_topk_keys, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, o, n, (unsigned long long)first_index, mode,
                     use_score_list ? 1 : 0, reinterpret_cast<const TopKState*>(d_state), d_score, d_key);
  return (int)hipGetLastError();
}
int launch_topk_select(const DevOut& o, uint32_t n, uint64_t first_index, const double* d_score, const unsigned long long* d_key, int k,
                       TopKBlock* d_blocks, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_topk_select, dim3((n + kTopKChunk - 1u) / kTopKChunk), dim3(1024), 0, (hipStream_t)stream, o, n,
                     (unsigned long long)first_index, d_score, d_key, k, d_blocks);
  return (int)hipGetLastError();
}
int launch_topk_merge(uint8_t* d_state, const uint8_t* d_blocks, int n_blocks, size_t block_stride, TopKBlock* d_pack, int k, const DevOut& o,
                      uint64_t own_first, uint32_t own_n, uint32_t step, void* stream) {
  hipLaunchKernelGGL(k_topk_merge, dim3(1), dim3(1024), 0, (hipStream_t)stream, reinterpret_cast<TopKState*>(d_state), d_blocks, n_blocks,
                     (unsigned long long)block_stride, d_pack, k, o, (unsigned long long)own_first, own_n, step);
  return (int)hipGetLastError();
}
int launch_pareto_fold(uint8_t* d_state, const ParetoWork& w, const DevOut& o, uint32_t n, uint64_t first_index, bool keep_spread, void* stream) {
  if (n == 0 || n > w.cap_n) return n == 0 ? 0 : (int)hipErrorInvalidValue;
  ParetoState* st = reinterpret_cast<ParetoState*>(d_state);
  const dim3 chunks((n + kParetoChunk - 1u) / kParetoChunk), block(pareto::kBlock);
  // (the list's length is the device's: the pairwise grids are sized for the longest one, blocks beyond it return at once)
  const dim3 pairs((n + (uint32_t)EG_PARETO_MAX + pareto::kBlock - 1u) / pareto::kBlock, pareto::kSplit);
  hipLaunchKernelGGL(k_pareto_filter, chunks, block, 0, (hipStream_t)stream, o, n, (unsigned long long)first_index, st, w);
  hipLaunchKernelGGL(k_pareto_compact, chunks, block, 0, (hipStream_t)stream, o, n, (unsigned long long)first_index, st, w);
  hipLaunchKernelGGL(k_pareto_dominate, pairs, block, 0, (hipStream_t)stream, st, w);
  if (keep_spread) hipLaunchKernelGGL(k_pareto_spread, dim3(1), dim3(pareto::kSpreadBlock), 0, (hipStream_t)stream, st, w);
  else hipLaunchKernelGGL(k_pareto_rank, pairs, block, 0, (hipStream_t)stream, st, w);
  hipLaunchKernelGGL(k_pareto_finalize, dim3(pareto::kCopyBlocks), block, 0, (hipStream_t)stream, st, w, o, n);
  return (int)hipGetLastError();
}
static_assert(sizeof(EpisodeMap) == 64 && offsetof(EpisodeMap, solo) == 48, "EpisodeMap: same_index sits in what was padding");
int launch_plan_edits(const uint8_t* d_base, const void* d_edits, uint32_t n, uint8_t* d_pool, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_plan_edits, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_base, reinterpret_cast<const uint2*>(d_edits), n, d_pool);
  return (int)hipGetLastError();
}
int launch_plan_edits_many(const uint8_t* d_bases, uint32_t n_bases, const uint32_t* d_slot, const void* d_edits, uint32_t n, uint8_t* d_pool, void* stream) {
  if (n == 0 || n_bases == 0) return 0;
  hipLaunchKernelGGL(many::k_plan_edits_many, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_bases, n_bases, d_slot, reinterpret_cast<const uint2*>(d_edits), n, d_pool);
  return (int)hipGetLastError();
}
int launch_plan_moves(const uint8_t* d_bases, uint32_t n_bases, const uint32_t* d_slot, const void* d_moves, uint32_t n, uint8_t* d_pool, void* stream) {
  if (n == 0 || n_bases == 0) return 0;
  hipLaunchKernelGGL(k_plan_moves, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_bases, n_bases, d_slot, reinterpret_cast<const uint2*>(d_moves), n, d_pool);
  return (int)hipGetLastError();
}
int launch_plan_crosses(const uint8_t* d_parents, uint32_t n_parents, const void* d_crosses, uint32_t n, uint8_t* d_pool, void* stream) {
  if (n == 0 || n_parents == 0) return 0;
  hipLaunchKernelGGL(k_plan_crosses, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_parents, n_parents, reinterpret_cast<const uint2*>(d_crosses), n, d_pool);
  return (int)hipGetLastError();
}
int launch_plan_rewrites(const uint8_t* d_plans, uint32_t n_plans, const uint8_t* d_maps, uint32_t n_maps, const void* d_rewrites, uint32_t n, uint8_t* d_pool,
                         void* stream) {
  if (n == 0 || n_plans == 0 || n_maps == 0) return 0;
  hipLaunchKernelGGL(k_plan_rewrites, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, d_plans, n_plans, d_maps, n_maps,
                     reinterpret_cast<const uint2*>(d_rewrites), n, d_pool);
  return (int)hipGetLastError();
}
int launch_plan_constraints(const DevOut& o, uint32_t n, const void* d_constraints, uint32_t k, uint32_t* d_violated, double* d_excess, void* stream) {
  if (n == 0 || k == 0 || k > (uint32_t)EG_CONSTRAINTS_MAX) return n == 0 || k == 0 ? 0 : (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_plan_constraints, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, o, n, reinterpret_cast<const pcons::Packed*>(d_constraints), k, d_violated,
                     d_excess);
  return (int)hipGetLastError();
}
int launch_build_constraints(const DevOut& o, uint32_t n, const void* d_constraints, uint32_t k_rows, const void* d_build_constraints, uint32_t k_builds,
                             uint32_t* d_violated, double* d_excess, void* stream) {
  if (n == 0 || k_builds == 0) return 0;
  if (k_rows + k_builds > (uint32_t)EG_CONSTRAINTS_MAX || k_rows > (uint32_t)EG_CONSTRAINTS_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_build_constraints, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, o, n, reinterpret_cast<const pcons::Packed*>(d_constraints), k_rows,
                     reinterpret_cast<const bcons::Packed*>(d_build_constraints), k_builds, d_violated, d_excess);
  return (int)hipGetLastError();
}
int launch_ensemble_keep(const DevOut& o, uint32_t n, void* d_slab, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_ensemble_keep, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, o, n, reinterpret_cast<ens::Kept*>(d_slab));
  return (int)hipGetLastError();
}
int launch_ensemble_commit(const DevOut& o, uint32_t n, const void* d_slabs, uint32_t n_streams, uint32_t tail, int mode, void* d_rows, void* stream) {
  if (n == 0) return 0;
  if (n_streams < 1u || n_streams > (uint32_t)EG_STREAMS_MAX || tail < 1u || tail > n_streams) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ensemble_commit, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, o, n, reinterpret_cast<const ens::Kept*>(d_slabs), n_streams, tail, mode,
                     reinterpret_cast<eg_ensemble_row*>(d_rows));
  return (int)hipGetLastError();
}
int launch_breed_gather(uint8_t* d_breed, const DevOut& o, uint32_t n, uint64_t first, const uint8_t* d_pool, void* stream) {
  if (n == 0 || n > (uint32_t)EG_PARETO_MAX * kWave) return n == 0 ? 0 : (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_breed_gather, dim3(EG_PARETO_MAX), dim3(kWave), 0, (hipStream_t)stream, reinterpret_cast<const ParetoState*>(d_breed), o, n,
                     (unsigned long long)first, d_pool, d_breed + breed_at::blocks, reinterpret_cast<BreedCounters*>(d_breed + breed_at::counters));
  return (int)hipGetLastError();
}
int launch_breed_turnover(uint8_t* d_breed, int next, void* stream) {
  hipLaunchKernelGGL(k_breed_turnover, dim3(EG_PARETO_MAX), dim3(kWave), 0, (hipStream_t)stream, reinterpret_cast<ParetoState*>(d_breed), d_breed + breed_at::blocks,
                     d_breed + breed_at::parents + (next ? breed_at::kParentArray : 0), d_breed + breed_at::readback,
                     reinterpret_cast<BreedCounters*>(d_breed + breed_at::counters));
  return (int)hipGetLastError();
}
int launch_explore_turnover(uint8_t* d_breed, int next, long long m_first, void* stream) {
  hipLaunchKernelGGL(k_explore_turnover, dim3(EG_PARETO_MAX), dim3(kWave), 0, (hipStream_t)stream, reinterpret_cast<const ParetoState*>(d_breed),
                     d_breed + breed_at::blocks, d_breed + breed_at::parents + (next ? breed_at::kParentArray : 0), d_breed + breed_at::readback,
                     reinterpret_cast<BreedCounters*>(d_breed + breed_at::counters), m_first);
  return (int)hipGetLastError();
}
int launch_refine_pick_many(const DevOut& o, const void* d_segs, uint32_t n_segs, uint32_t n_total, int mode, const void* d_edits, const uint8_t* d_pool,
                            uint8_t* d_bases, uint32_t n_bases, uint8_t* d_entries, void* stream) {
  static_assert(sizeof(refine::Segment) == kRefineSegmentBytes, "segment table entry");
  if (n_segs == 0 || n_total == 0) return 0;
  hipLaunchKernelGGL(many::k_refine_pick_many, dim3(n_segs), dim3(refine::kThreads), 0, (hipStream_t)stream, o, reinterpret_cast<const refine::Segment*>(d_segs), n_total, mode,
                     reinterpret_cast<const uint2*>(d_edits), d_pool, d_bases, n_bases, d_entries);
  return (int)hipGetLastError();
}
int launch_repair_pick_many(const DevOut& o, const void* d_segs, uint32_t n_segs, uint32_t n_total, int mode, const void* d_edits, const uint8_t* d_pool,
                            uint8_t* d_bases, uint32_t n_bases, const uint32_t* d_violated, const double* d_excess, uint32_t k, const double* d_weights,
                            uint8_t* d_entries, void* stream) {
  if (n_segs == 0 || n_total == 0) return 0;
  if (k == 0 || k > (uint32_t)EG_CONSTRAINTS_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(repair::k_repair_pick_many, dim3(n_segs), dim3(refine::kThreads), 0, (hipStream_t)stream, o, reinterpret_cast<const refine::Segment*>(d_segs), n_total, mode,
                     reinterpret_cast<const uint2*>(d_edits), d_pool, d_bases, n_bases, d_violated, d_excess, k, d_weights, d_entries);
  return (int)hipGetLastError();
}
int launch_pick_best(const DevOut& o, uint32_t n, uint64_t first_index, UpdateCandidate* d_cand, void* stream) {
  hipLaunchKernelGGL(k_pick_best, dim3(1), dim3(1024), 0, (hipStream_t)stream, o, n, (unsigned long long)first_index, d_cand);
  return (int)hipGetLastError();
}

#endif      // EG_TU_THROUGHPUT

}  // namespace eg
