// eg_host.h — what the host units of the C ABI share (eg_api / eg_fetch / eg_debug / eg_plans / eg_plan_host / eg_constraints / eg_streams / eg_refine / eg_breed / eg_explore /
// eg_place / eg_group .cpp): owned buffers, the error macros, the context and the helpers that cross units, listed by the unit that holds them.  Host only: the kernels include eg_internal.h, never this.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "eg_internal.h"

#define EG_HIP(call) \
  do { const hipError_t e_ = (call); if (e_ != hipSuccess) { eg::set_error(std::string(#call) + ": " + hipGetErrorString(e_)); return EG_ERR_HIP; } } while (0)
// a launcher of eg_rollout.hip (they return the launch's hipError_t as an int): "k_x launch: <what HIP says>"
#define EG_LAUNCH_AS(what, call) \
  do { const int lr_ = (call); if (lr_ != 0) { eg::set_error(std::string(what ": ") + hipGetErrorString((hipError_t)lr_)); return EG_ERR_HIP; } } while (0)
#define EG_LAUNCH(name, call) EG_LAUNCH_AS(name " launch", call)
// a call that returns EG_OK or an error code with the error text set
#define EG_TRY(call) do { const int rc_ = (call); if (rc_ != EG_OK) return rc_; } while (0)

namespace eg {
// An owned allocation of `count` elements of T in device memory (Pinned: in pinned host memory).  Move-only; converts to T*.
template <typename T, bool Pinned = false>
struct DevBuf {
  T* ptr = nullptr; size_t count = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { std::swap(ptr, o.ptr); std::swap(count, o.count); }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(ptr, o.ptr); std::swap(count, o.count); return *this; }
  ~DevBuf() { release(); }
  operator T*() const { return ptr; }
  void release() { if (ptr) (void)(Pinned ? hipHostFree(ptr) : hipFree(ptr)); ptr = nullptr; count = 0; }
  // Room for n elements: a new allocation of exactly n only when n exceeds what is held (what is held is what eg_memory_report tells),
  // the old one freed first — hipFree waits for the launches that may still use it.  *fresh: whether the buffer is a new one (its
  // contents undefined: the callers that rely on zeros clear it).  After a failure nothing is held.  `flags`: of hipHostMalloc.
  hipError_t reserve(size_t n, bool* fresh = nullptr, unsigned flags = 0) {
    if (fresh) *fresh = n > count;
    if (n <= count) return hipSuccess;
    release();
    const hipError_t e = Pinned ? hipHostMalloc((void**)&ptr, sizeof(T) * n, flags) : hipMalloc((void**)&ptr, sizeof(T) * n);
    if (e != hipSuccess) ptr = nullptr; else count = n;
    return e;
  }
  // the same for callers that carry on without the buffer when memory is short: the sticky HIP error is cleared
  bool try_reserve(size_t n, unsigned flags = 0) {
    if (reserve(n, nullptr, flags) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
};
template <typename T> using PinBuf = DevBuf<T, true>;
// the constraints of one kind that a context holds: the n set ones on the device (EG_CONSTRAINTS_MAX slots, zeros behind the n), their host
// copy, and the host copy of what the last judged batch ran under (eg_last_batch_constraints, eg_last_batch_build_constraints)
template <class T> struct ConstraintSet { DevBuf<uint8_t> dev; int n = 0; T set[EG_CONSTRAINTS_MAX] = {}, judged[EG_CONSTRAINTS_MAX] = {}; };
}  // namespace eg

struct eg_host_tables {
  eg::HostTables H;
  std::map<std::string, std::pair<const double*, int64_t>> f64;
  std::map<std::string, std::pair<const int32_t*, int64_t>> i32;
  void index();
};

struct eg_ctx {
  int device = 0;
  eg_host_tables tables;
  eg::DevBuf<uint8_t> d_tables;      // the table blob (dev.base)
  eg::DevTables dev{};
  // snapshot in HBM: the whole snapshot lives in ONE device buffer filled by ONE copy from a pinned staging buffer
  eg::DevBuf<uint8_t> d_snap; eg::PinBuf<uint8_t> h_snap;
  eg::DevBuf<uint8_t> d_snap_held;      // eg_policy_hold / eg_policy_rewind
  // the reference's best_result fold (multi_simulation.rs:613-620): 0 = not tracked, 1 = optimization_mode None, 2 = cost_only
  int fold_mode = 0; eg::DevBuf<uint8_t> d_fold;
  bool group_member = false;      // owned by an eg_group: the group folds its ranks' results (eg_group_best_result_track), never the context itself
  // the top-K archive of distinct scenarios (eg_top_k_track; eg_topk.h): 0 = not tracked, 1 = mode None, 2 = cost_only; d_topk: TopKState
  // and the record slots; per batch, the rank score and key of every episode and one block per chunk (also a group rank's scratch)
  int topk_mode = 0, topk_k = 0; eg::DevBuf<uint8_t> d_topk;
  eg::DevBuf<double> d_tk_score; eg::DevBuf<unsigned long long> d_tk_key; eg::DevBuf<eg::TopKBlock> d_tk_blocks;
  // the Pareto archive of outcomes (eg_pareto_track; eg_pareto.h): pareto_cap 0 = not tracked; d_pareto: ParetoState and the cap record
  // slots, allocated by eg_pareto_track; d_pareto_work: what the kernels of a fold hand each other, sized for pareto_work_n episodes
  // pareto_spread: the archive's capacity rule is "keep spread" (EG_PARETO_KEEP_SPREAD): a fold launches k_pareto_spread, not k_pareto_rank
  int pareto_cap = 0; eg::DevBuf<uint8_t> d_pareto, d_pareto_work; uint32_t pareto_work_n = 0; bool pareto_spread = false;
  // Is the best list long (the replay episodes run the heavy-capable variant and are the batch's long pole)?  `list_exact`: the host
  // KNOWS the list the next launch will find on the device (it uploaded, rewound or pulled it and no on-device update has been
  // enqueued since): the replay variant that has nothing to do is then not launched at all.  Otherwise the device may have replaced
  // the list since the host last looked — both variants are launched and decide for themselves — and the hint only orders the
  // launches; it follows the device through `h_list_len`, a pinned host word that k_apply_update and k_rewind write the list's
  // length to (read without synchronising: as old as the launch queue is deep).
  bool long_list_hint = false, long_list_hint_held = false, list_exact = false, list_exact_held = false;
  eg::PinBuf<uint32_t> h_list_len; uint32_t* d_list_len = nullptr;      // the same pinned word, host and device address
  eg::DevSnapshot snap{};
  bool snap_valid = false;
  // outputs: the records and the score list in one buffer (ensure_outputs); `out` points into it
  eg::DevBuf<uint8_t> d_out; eg::DevOut out{};
  uint32_t last_n = 0;
  uint64_t last_first = 0;      // global index of the first episode of the last batch
  eg::DevBuf<uint8_t> d_mask;
  // timing: a ring of event pairs riding on the rollout dispatches.  A pair is only waited for when the ring comes round to
  // it again (kTimingRing launches later: long finished) or when the caller reads the timing — never inside a training step.
  static constexpr int kTimingRing = 256;
  hipEvent_t ev[kTimingRing][4] = {};       // start / stop of the heavy grid, start / stop of the lean grid (eg_internal.h RolloutPlan)
  uint8_t ev_used[kTimingRing] = {};        // bit 0: the heavy pair was recorded, bit 1: the lean pair
  hipStream_t stream_heavy = nullptr;   // the replay grids of a split batch run beside the lean grid (which stays on the null stream)
  hipEvent_t ev_fork[kTimingRing] = {}, ev_go[kTimingRing] = {}, ev_join[kTimingRing] = {};
  eg::DevBuf<uint32_t> d_index;         // replay / other episode indices of a host-masked batch
  int ring_head = 0, ring_pending = 0;      // next pair to use; pairs recorded and not yet collected (the oldest is head - pending)
  double total_ms = 0.0; int32_t n_launches = 0;
  double grids_ms = 0.0;      // the same launches, every grid's own duration added up (== total_ms when a batch is one grid)
  // eg_place / eg_find_suitable_location: device buffers kept between calls (d_place_xy: the x, then the y, half the buffer each)
  eg::DevBuf<uint16_t> d_place_cells; eg::DevBuf<int32_t> d_place_cell; eg::DevBuf<double> d_place_score, d_place_xy;
  uint32_t push_iteration_count = 0;     // iteration counter written into the device state by the next upload
  uint32_t push_failed = 0;              // ... and the failed-episode counter
  uint32_t pulled_improvements = 0;      // on-device improvement log entries already appended to a host policy
  // eg_train_step / eg_device_step: library-owned update packet (device) and its pinned host copy
  eg::DevBuf<uint8_t> d_packet; eg::PinBuf<uint8_t> h_packet;
  // batches of at most this many episodes run the helper-wave kernel (three waves per episode, all resident at once)
  uint32_t helper_max_episodes = 0;
  // heavy episodes (eg_field.h place_heavy): pool of penalty fields, one slot per episode that outgrows kHeavyGens (d_heavy, d_heavy_claim: what dev.heavy* point to)
  // EIRGRID_HEAVY_POOL_GB (default 64): what the pool may grow to, 126 KB per replay episode of a launch; 131 072 replay episodes
  // (an all-replay batch of configs[3]'s size) want 16 GB.  eg_memory_report tells what is held.
  eg::DevBuf<uint8_t> d_heavy; eg::DevBuf<unsigned> d_heavy_claim;
  uint32_t heavy_slots_max = 0, heavy_slots_wanted = 4096, launch_epoch = 0;
  bool heavy_slots_auto = true;      // (EIRGRID_HEAVY_SLOTS fixes the pool size instead)
  // replay hoist (eg_replay_coop.h; eg_replay_hoist / EIRGRID_REPLAY_HOIST=1): the replay episodes of a batch computed once.
  // d_hoist: a HoistInfo (eg_internal.h); d_coop: the scratch record.
  bool hoist_on = false, hoist_supported = false;
  unsigned long long hoist_seq = 0;
  eg::DevBuf<uint8_t> d_hoist, d_coop;
  uint64_t hoist_batches = 0;      // batches launched with the hoist armed (eg_replay_hoist_stats)
  int coop_force = 0;              // EIRGRID_COOP_FORCE (test hook): the hoisted searches' rarely-run paths
  eg::DevBuf<long long> d_stats_rep;      // kStatsReplicas copies of the statistics array (RolloutPlan::d_stats_rep); EIRGRID_STATS_REPLICAS=0: none
  // set from a launch that adds to the copies until k_fold_stats (which clears them) is enqueued behind it: a batch that failed in
  // between left partial sums there, and the next batch that uses the copies clears them first
  bool stats_rep_dirty = false;
  // per-episode replay kernel (eg_replay_solo.h; EIRGRID_REPLAY_SOLO=0: off): a word per replay episode of a launch, the launches' sequence
  eg::DevBuf<unsigned long long> d_solo; unsigned long long solo_seq = 0;
  bool solo_on = true;
  bool uniform_on = true;      // EIRGRID_UNIFORM=0: throughput batches launch k_rollout<0, kind> for the lean and short-replay kinds, not k_episodes
  // plan batches (eg_evaluate_plans): the evaluated policy's own snapshot (the resident one in d_snap stays untouched), the plan blocks
  // (snap::kPlanStride bytes each) and the index lists of the short and the long plans
  eg::DevBuf<uint8_t> d_eval_snap, d_plans;
  eg::DevBuf<uint32_t> d_plan_index;
  // plan-edit batches (eg_evaluate_plan_edits): the base plan's block followed by the packed edits, 8 bytes each — what k_plan_edits reads
  // (a plan-cross batch, eg_evaluate_plan_crosses: every parent's block, then the packed crosses — what k_plan_crosses reads; a plan-rewrite
  //  batch, eg_evaluate_plan_rewrites: every plan's block, the maps, then the packed rewrites — what k_plan_rewrites reads)
  eg::DevBuf<uint8_t> d_plan_edit_in;
  size_t n_plan_blocks = 0;      // blocks of the last plan or plan-edit batch in d_plans (eg_debug_fetch_plan_block)
  // constraints (eg_plan_constraints_set, eg_build_constraints_set; eg_constraints.cpp), a ConstraintSet per kind: rows, the plan constraints
  // on the yearly rows, 16 bytes each, and builds, the build constraints, 168 bytes each.  The two side buffers are what k_plan_constraints
  // — with a build constraint set k_build_constraints, which judges both kinds — fills behind a plan batch: a mask per record, an excess
  // row of feas_k doubles per record.  feas_k: the constraints the last batch was judged under, 0 when it was not (every batch that sets
  // last_n sets it); feas_builds: how many of them — the last columns of an excess row — are build constraints (constrain_batch sets both)
  eg::ConstraintSet<eg_plan_constraint> rows; eg::ConstraintSet<eg_build_constraint> builds;
  eg::DevBuf<uint32_t> d_violated; eg::DevBuf<double> d_excess; int feas_k = 0, feas_builds = 0;
  // plan streams (eg_plan_streams_set; eg_streams.cpp): what is set (n 0: none), what the last batch ran under (ran.n 0: no streams; every batch
  // that sets last_n sets it), the store of what every pass left — entry (r, j) at (r * last_n + j) * kEnsembleKeptBytes — and the rows
  // k_ensemble_commit wrote, both reserved by the first batch that needs them
  struct Streams { int n = 0, tail = 0, mode = 0; } streams, ran;
  eg::DevBuf<uint8_t> d_ens_kept; eg::DevBuf<eg_ensemble_row> d_ens_rows;
  // what the store holds: the n its slabs are laid out for and, bit r, the slabs kept since the store was last laid out (ensemble_keep)
  uint32_t ens_kept_n = 0; uint64_t ens_kept_mask = 0;
  // plan refinement (eg_refine_plan, eg_refine_plans): the step log k_refine_pick_many writes, an entry per plan of a launch from the
  // start (kRefineLog entries of kRefineEntryStride bytes); the base blocks of the call's plans (uploaded once, kept current by
  // k_refine_pick_many) and what a launch uploads in one copy: the packed edits, the base slot of every variant, the segment table
  // (eg_repair_plans, the same loop under its other rule: k_repair_pick_many writes the log and the bases, its weights ride behind the table)
  // EIRGRID_REFINE_LAUNCH_VARIANTS (default and at most 16 384, at least 1; read at every call): the variants a launch may hold — a plan
  // with more gets a launch to itself (so eg_refine_plan's one plan always does); for tests that want many launches per round at small sizes
  eg::DevBuf<uint8_t> d_refine_log, d_refine_bases, d_refine_in;
  // generations of crosses (eg_breed_plans): the private archive with its block slots, parent arrays and readback (eg_internal.h breed_at),
  // allocated at the first call, and Pareto work of its own sized for a launch of EG_CROSS_MAX_VARIANTS.  eg_explore_plans uses both the
  // same way (the parent arrays as its frontier arrays); either call starts the archive empty
  eg::DevBuf<uint8_t> d_breed, d_breed_work;
  bool breed_spread = false;     // the private archive's capacity rule, as pareto_spread (archive_begin sets it from the call's mode)
  bool debug_breed = false;     // eg_debug_breed_begin has started the private archive (the crafted-generation test hooks)
};

namespace eg {
// the two process-wide switches, read from the environment at first use (eg_api.cpp, next to the context's options)
bool stats_replicas_off();      // EIRGRID_STATS_REPLICAS=0
bool fetch_full();              // EIRGRID_FETCH_FULL=1
// eg_api.cpp
int ensure_outputs(eg_ctx* c, uint32_t n);
int prepare_heavy(eg_ctx* c, uint32_t n_heavy, bool known_short);
int ring_take(eg_ctx* c, RolloutPlan& plan, int& slot);
void ring_commit(eg_ctx* c, int slot, int ev_used);
int arm_solo(eg_ctx* c, RolloutPlan& plan, uint32_t n);
int ensure_packet(eg_ctx* c);      // the library-owned update packet (d_packet, zeroed when new) and its pinned copy
int device_apply(eg_ctx* c, const void* d_packets, int32_t n_packets, size_t packet_stride, void* d_own_packet, uint64_t noise_seed, bool local_pick);
// eg_plans.cpp: a policy in snapshot layout, a plan batch's launches, what is packed per variant, plan sets to blocks and back
int check_policy(const eg_policy_snapshot* s, const eg_opts* o, const char* who);
void stage_policy(eg_ctx* c, const eg_policy_snapshot* s, bool have_lists, uint8_t* h);
DevSnapshot snapshot_of(uint8_t* d_base, const eg_opts* o);
void write_lists(uint8_t* dst, const int32_t* count, const uint8_t* act, const int32_t* dcount, const uint8_t* dact);
int stage_eval_snapshot(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, DevSnapshot* S);
int launch_plans(eg_ctx* c, const DevSnapshot& S, uint64_t seed, uint64_t first_index, uint32_t n, uint32_t n_short, bool same_index);
// ... a move's 8 bytes (eg_plan_moves.h unpack_move), a cross's (eg_plan_crosses.h unpack_cross) and a rewrite's (eg_plan_rewrites.h unpack_rewrite)
void pack_plan_move(const eg_plan_move& m, uint32_t* packed);
void pack_plan_cross(const eg_plan_cross& x, uint32_t* packed);
void pack_plan_rewrite(const eg_plan_rewrite& r, uint32_t* packed);
// ... the prefix offsets of every plan of a set (off[w][p * 27 + y]) and a child's list length from them
void parent_offsets(const eg_plan_set* p, std::vector<int32_t> off[2]);
int64_t child_len(const std::vector<int32_t>& off, const eg_plan_cross& x);
// ... a set's plan blocks, and the reverse: n plan blocks read back from the device (host memory) decoded into a plan set (names "")
void write_plan_blocks(const eg_plan_set* p, uint8_t* dst);
int decode_plan_blocks(const uint8_t* blocks, int32_t n, const char* who, eg_plan_set** set);

// eg_constraints.cpp: k_plan_constraints — with a build constraint set, k_build_constraints in its place — over the n records of
// c->out under the context's constraints (at least one of either kind is set), on the null stream; the side buffers reserved, c->feas_k
// and c->feas_builds set
int constrain_batch(eg_ctx* c, uint32_t n);
// eg_streams.cpp: the two launches of a batch under plan streams, on the null stream behind a pass.  keep: the n records of c->out into slab
// r of a store reserved for `slabs` slabs of n (a store that has to grow loses what it held: the caller reserves for all its slabs with
// the first one it keeps); commit: k_ensemble_commit over slabs 0..R-1, the rows reserved, c->ran set
int ensemble_keep(eg_ctx* c, uint32_t n, int r, int slabs);
int ensemble_commit(eg_ctx* c, uint32_t n, int R, int tail, int mode);

// eg_plan_host.cpp: the pieces a plan search is written from.  `fn` / `who` name the entry point in the messages.
// Behind an entry point's own NULL test: a rank of a group is refused, then `validate` runs, then check_policy, then hipSetDevice
int plan_entry(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, const char* fn, const std::function<int32_t()>& validate);
// The routing of a launch (launch_plans): the variants whose best_actions list is short (<= kShortReplayMax entries) first, then the long
// ones, each in the order they were added.  finish(): the short ones' count; idx is then the index array.
struct Routing {
  std::vector<uint32_t> idx, longs;
  void clear() { idx.clear(); longs.clear(); }
  void add(uint32_t j, int64_t len0) { (len0 > kShortReplayMax ? longs : idx).push_back(j); }
  uint32_t finish() { const uint32_t n_short = uint32_t(idx.size()); idx.insert(idx.end(), longs.begin(), longs.end()); longs.clear(); return n_short; }
};
void pack_plan_edits(const eg_plan_edit* edits, uint32_t n, int64_t base_len, uint32_t* packed, uint32_t* idx, uint32_t* n_short);
// Variants [first, first + n_edits + n_moves) of a launch: edits, then moves, of the plan in base block `base_slot` whose best_actions
// holds len0 entries — their 8 bytes into `packed`, their route into R, their base into `slot`.  Returns whether a move was packed.
bool pack_neighbourhood(uint32_t base_slot, int64_t len0, const eg_plan_edit* edits, uint32_t n_edits, const eg_plan_move* moves, uint32_t n_moves, uint32_t first,
                        uint32_t* packed, uint32_t* slot, Routing& R);
// A launch of n variants: `in` (the packed variants, at at_slot every variant's base slot) into c->d_refine_in and R's finished index up,
// k_plan_edits_many and (any_moves) k_plan_moves over the n_bases blocks at d_bases, then the plan batch with same_index
int launch_variants(eg_ctx* c, const DevSnapshot& S, const uint8_t* d_bases, uint32_t n_bases, const std::vector<uint8_t>& in, size_t at_slot, uint32_t n,
                    Routing& R, bool any_moves, uint64_t seed, uint64_t index);
// The private archive of a breed / explore call (c->d_breed, eg_internal.h breed_at; c->d_breed_work).  begin: allocated at the first call,
// started empty at every call (`between`, the test hooks': runs between the state's upload and the counters'); array: parent / frontier
// array 0 | 1; upload: a set's blocks into it; fold: the n results of c->out with the blocks of c->d_plans, launch_pareto_fold then
// k_breed_gather; read_generation: the readback buffer (waits for the generation); row: row r of it, false unless its tables start at 0,
// ascend and stay within snap::kBestCap and its slot lies in [0, cap) — the index is the caller's to check; fetch_record: the record in
// `slot` into row r of `out` (NULL: nothing); decode: n blocks at d_blocks (slots != NULL: block r is in slots[r]) as a plan set
int archive_begin(eg_ctx* c, int32_t cap, int32_t objectives, int32_t mode, const std::function<int()>& between = nullptr);
inline uint8_t* archive_array(eg_ctx* c, int which) { return c->d_breed + breed_at::parents + size_t(which) * breed_at::kParentArray; }
int archive_upload(eg_ctx* c, const eg_plan_set* set, int array);
int archive_fold(eg_ctx* c, uint32_t n, uint64_t first_index);
int archive_read_generation(eg_ctx* c, std::vector<uint8_t>& rb);
bool archive_row(const std::vector<uint8_t>& rb, int32_t r, int32_t cap, ParetoEntry* entry, int32_t (&tab)[2][28]);
int archive_fetch_record(eg_ctx* c, int32_t slot, const eg_episode_out* out, size_t r);
int decode_device_blocks(const uint8_t* d_blocks, int32_t n, const int32_t* slots, const char* who, eg_plan_set** set);
// The option checks the validators share; `fail` sets "<validator>: <message>" and returns EG_ERR_BAD_ARG
using Fail = std::function<int32_t(const std::string&)>;
int32_t check_mode(const Fail& fail, int32_t mode);
int32_t check_objectives(const Fail& fail, int32_t objectives);
int32_t check_cap(const Fail& fail, int32_t cap);
int32_t check_launch_variants(const Fail& fail, int32_t launch_variants);
int32_t validate_action_lists(const Fail& fail, int32_t n_replace, const uint8_t* replace_with, int32_t n_append, const uint8_t* append_with);
// the weights of a repair (eg_repair_plans, eg_debug_repair_pick_many) for k constraints: k 1..EG_CONSTRAINTS_MAX, each weight finite and > 0 (NULL: 1.0 each)
int32_t check_repair_weights(const Fail& fail, const double* weights, int32_t k);
// what eg_breed_validate and eg_explore_validate open with (their options begin alike): the set's size, the options, mode .. max_generations
template <typename Opts> int32_t validate_front_opts(const Fail& fail, const eg_plan_set* set, const Opts* o) {
  if (set->n_plans > EG_CROSS_MAX_PARENTS) return fail("the set holds " + std::to_string(set->n_plans) + " plans (at most " + std::to_string(EG_CROSS_MAX_PARENTS) + ")");
  if (!o) return fail("NULL options");
  EG_TRY(check_mode(fail, o->mode)); EG_TRY(check_objectives(fail, o->objectives)); EG_TRY(check_cap(fail, o->cap));
  return o->max_generations < 1 ? fail("max_generations = " + std::to_string(o->max_generations) + " (at least 1)") : EG_OK;
}
// eg_fetch.cpp
int fetch_records(const uint8_t* d_base, size_t N, eg_episode_out* o);
eg_episode_out out_row(const eg_episode_out* o, size_t r);      // row r of a caller's episode-major buffers
int fold_reset(DevBuf<uint8_t>& d_fold);
int topk_reset(DevBuf<uint8_t>& d_topk, int k, int mode);
int topk_select(eg_ctx* c, uint32_t n, uint64_t first_index, int mode, bool use_score_list, const uint8_t* d_state, int k);
// the n results of c->out (global indices first_index..) folded behind a batch, on the null stream: into the best_result fold
// (c->fold_mode != 0), into the top-K archive (c->topk_mode != 0: topk_select, then k_topk_merge), into the Pareto archive
int best_result_fold(eg_ctx* c, uint32_t n, uint64_t first_index);
int topk_fold(eg_ctx* c, uint32_t n, uint64_t first_index, bool use_score_list);
int pareto_fold(eg_ctx* c, uint32_t n, uint64_t first_index);
inline uint32_t topk_chunks(uint32_t n) { return (n + kTopKChunk - 1u) / kTopKChunk; }
// The entries of the archive state `st` into the caller's rows: archive_of(i, entry) is the device archive (TopKState, then the record
// slots) that holds entry i's record, made current on its device — or NULL with the error text set.  `who` names the entry point.
int fetch_topk_rows(const char* who, const TopKState& st, const std::function<const uint8_t*(int, const TopKEntry&)>& archive_of,
                    eg_episode_out* o, int32_t* n_held, double* scores, int64_t* global_index);

}  // namespace eg
