// eg_api.cpp — C ABI glue: the context's life cycle, HBM residency of tables / snapshot / outputs, the batch launches, training steps,
// the device-resident policy, timing.  (Results: eg_fetch.cpp; test hooks over crafted batches: eg_debug.cpp; plan batches: eg_plans.cpp; placement queries: eg_place.cpp; N ranks in
// one process: eg_group.cpp; what they share: eg_host.h.)
// There is no CPU execution path behind these entry points: without a HIP device eg_create fails.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "eg_device_tables.h"
#include "eg_host.h"
#include "eg_policy_internal.h"

namespace eg {
namespace {
thread_local std::string g_error;
}
void set_error(const std::string& s) { g_error = s; }
}  // namespace eg

using namespace eg;

void eg_host_tables::index() {
  auto F = [&](const char* n, const std::vector<double>& v) { f64[n] = {v.data(), (int64_t)v.size()}; };
  auto I = [&](const char* n, const std::vector<int32_t>& v) { i32[n] = {v.data(), (int64_t)v.size()}; };
  F("usage", H.usage); F("population", H.population); F("pre_co2", H.pre_co2); F("pre_tg", H.pre_tg); F("pre_ig", H.pre_ig);
  F("pre_sg", H.pre_sg); F("pre_optot", H.pre_optot); F("te", H.te); F("coastf", H.coastf); F("dr", H.dr); F("m03", H.m03);
  F("t12", H.t12); F("cc", H.cc); F("out_mw", H.out_mw); F("co2_t", H.co2_t); F("offv", H.offv); F("offc", H.offc);
  F("inflation", H.inflation); F("carbon_price", H.carbon_price);
  f64["size_factor"] = {&H.size_factor, 1};
  I("pre_opcnt", H.pre_opcnt); I("cls", H.cls); I("rclass", H.rclass); I("marine", H.marine); I("reach", H.reach);
  I("existing_online", H.existing_online);
}

// ---- run-time switches: everything the library reads from the environment ----------------------------------------------
namespace {
// a context's, read once by eg_create
struct Options {
  bool helper_off = false, helper_all = false;      // EIRGRID_HELPER_WAVES=0: no small-batch kernel, =all: for every batch size (diagnostics / parity tests)
  // EIRGRID_HEAVY_SLOTS: a fixed number of field slots for heavy episodes (default: 4096 = 516 MB, enlarged to what a launch needs;
  // 0 = every search is the exact scan)
  bool heavy_slots_auto = true; uint32_t heavy_slots_wanted = 4096;
  uint32_t heavy_slots_max = 0;      // EIRGRID_HEAVY_POOL_GB (default 64): what the pool may grow to, in slots
  bool side_stream_plain = false;      // EIRGRID_SIDE_STREAM=plain (diagnostics): the side stream without a priority of its own
  bool replay_hoist = false;           // EIRGRID_REPLAY_HOIST=1: the hoist armed from the start (where the world supports it)
  int coop_force = 0;                  // EIRGRID_COOP_FORCE (test hook)
  bool solo_on = true;                 // EIRGRID_REPLAY_SOLO=0: no per-episode replay kernel
  uint32_t solo_tiles = 1u;            // EIRGRID_SOLO_TILES=0: k_replay_solo searches by rank, as the classic variant does (A/B on one library)
  // EIRGRID_SOLO_LAZY: the longest replay script (generators) that runs with the lazy field (k_replay_lazy in k_replay_solo's place); 0: none
  // (k_replay_solo: the field current after every placement, as the classic variant keeps it), all: every script.  Default: measured on the benchmark's states — 9 % faster at
  // 228 generators, 4 % slower at 468, 16 % slower at 916 (profiles/r10_ab_notes.log): six blocks of 64 generators.
  bool uniform_on = true;              // EIRGRID_UNIFORM=0: the lean and the short-replay kind on k_rollout<0, kind>, not on k_episodes (tests, A/B on one library)
  uint32_t solo_lazy = 512u;      // (the lists' on-chip window: measured ahead of the eager field at 228 and 468 generators, behind it at 916 — DESIGN §4, round 14)
};
Options read_options() {
  Options o;
  if (const char* hv = std::getenv("EIRGRID_HELPER_WAVES")) { o.helper_off = std::string(hv) == "0"; o.helper_all = std::string(hv) == "all"; }
  if (const char* hs = std::getenv("EIRGRID_HEAVY_SLOTS")) { o.heavy_slots_wanted = (uint32_t)std::strtoul(hs, nullptr, 10); o.heavy_slots_auto = false; }
  o.heavy_slots_max = uint32_t((size_t(64) << 30) / (size_t(kRadiusClasses) * 2624 * sizeof(double)));
  if (const char* hg = std::getenv("EIRGRID_HEAVY_POOL_GB"))
    o.heavy_slots_max = uint32_t(std::min(double((1u << 20) - 1u), std::max(0.0, std::atof(hg)) * double(size_t(1) << 30) / double(size_t(kRadiusClasses) * 2624 * sizeof(double))));
  if (o.heavy_slots_max > (1u << 20) - 1u) o.heavy_slots_max = (1u << 20) - 1u;      // (the claim word counts slots in 20 bits)
  if (o.heavy_slots_wanted > o.heavy_slots_max) o.heavy_slots_wanted = o.heavy_slots_max;
  if (const char* sp = std::getenv("EIRGRID_SIDE_STREAM")) o.side_stream_plain = std::string(sp) == "plain";
  if (const char* rh = std::getenv("EIRGRID_REPLAY_HOIST")) o.replay_hoist = rh[0] == '1';
  if (const char* cf = std::getenv("EIRGRID_COOP_FORCE")) o.coop_force = std::atoi(cf);
  if (const char* so = std::getenv("EIRGRID_REPLAY_SOLO")) o.solo_on = so[0] != '0';
  if (const char* st = std::getenv("EIRGRID_SOLO_TILES")) o.solo_tiles = st[0] != '0' ? 1u : 0u;
  if (const char* sl = std::getenv("EIRGRID_SOLO_LAZY")) o.solo_lazy = std::string(sl) == "all" ? 0xFFFFFFFFu : (uint32_t)std::strtoul(sl, nullptr, 10);
  if (const char* un = std::getenv("EIRGRID_UNIFORM")) o.uniform_on = un[0] != '0';
  return o;
}

// collects the oldest `count` recorded launches (all of them when count < 0).  A batch that ran as several grids counts as
// ONE launch lasting from the earlier start to the later end.
int collect_timing(eg_ctx* c, int count = -1) {
  if (count < 0 || count > c->ring_pending) count = c->ring_pending;
  for (; count > 0; --count) {
    const int i = (c->ring_head - c->ring_pending + 2 * eg_ctx::kTimingRing) % eg_ctx::kTimingRing;
    const bool heavy = c->ev_used[i] & 1, lean = c->ev_used[i] & 2;
    float best = 0.f, sum = 0.f;      // the longest of start a .. stop b; every grid's own start .. stop added up
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        if (!(a ? lean : heavy) || !(b ? lean : heavy)) continue;
        EG_HIP(hipEventSynchronize(c->ev[i][2 * b + 1]));
        float ms = 0.f;
        EG_HIP(hipEventElapsedTime(&ms, c->ev[i][2 * a], c->ev[i][2 * b + 1]));
        if (a == b) sum += ms;
        if (ms > best) best = ms;
      }
    c->total_ms += double(best); c->grids_ms += double(sum); c->n_launches += 1; c->ring_pending -= 1;
  }
  return EG_OK;
}
}  // namespace
// the process's, read at first use
static bool env_starts(const char* name, char ch) { const char* e = std::getenv(name); return e && e[0] == ch; }
bool eg::stats_replicas_off() { static const bool off = env_starts("EIRGRID_STATS_REPLICAS", '0'); return off; }
bool eg::fetch_full() { static const bool full = env_starts("EIRGRID_FETCH_FULL", '1'); return full; }

int eg::ensure_outputs(eg_ctx* c, uint32_t n) {
  const size_t bytes = size_t(n) * rec::stride + size_t(n) * sizeof(double);
  if (bytes <= c->d_out.count) return EG_OK;
  c->out = DevOut{};
  EG_HIP(c->d_out.reserve(bytes));
  c->out.base = c->d_out;
  c->out.score_list = reinterpret_cast<double*>(c->out.base + size_t(n) * rec::stride);
  // zero once so episodes that end early leave defined year counts / rows behind
  EG_HIP(hipMemset(c->out.base, 0, bytes));
  return EG_OK;
}

// The next slot of the timing ring for a launch (the oldest pair is collected first when the ring is full): its events into plan.ev.
int eg::ring_take(eg_ctx* c, RolloutPlan& plan, int& slot) {
  if (c->ring_pending == eg_ctx::kTimingRing) EG_TRY(collect_timing(c, 1));
  slot = c->ring_head;
  for (int k = 0; k < 4; ++k) plan.ev[k] = c->ev[slot][k];
  plan.classic_kernels = !c->uniform_on;      // (every rollout launch takes its events here)
  return EG_OK;
}
// ... and behind the launch: which of its pairs were recorded (bit 0: the heavy grid's, bit 1: the lean grid's)
void eg::ring_commit(eg_ctx* c, int slot, int ev_used) {
  c->ev_used[slot] = uint8_t(ev_used);
  c->ring_head = (c->ring_head + 1) % eg_ctx::kTimingRing; c->ring_pending += 1;
}
// k_replay_solo ahead of the long-replay variant for the n long replays of a launch (eg_replay_solo.h): a word each, a sequence number
int eg::arm_solo(eg_ctx* c, RolloutPlan& plan, uint32_t n) {
  if (!c->solo_on) return EG_OK;
  bool fresh = false;
  EG_HIP(c->d_solo.reserve(n, &fresh));
  if (fresh) EG_HIP(hipMemsetAsync(c->d_solo, 0, sizeof(unsigned long long) * n, nullptr));
  plan.solo_seq = ++c->solo_seq; plan.d_solo = c->d_solo;
  return EG_OK;
}

// before every rollout launch: the field pool holds a slot for every heavy episode of the launch (allocated on first use,
// enlarged when a launch brings more of them: a replay episode without a slot falls back to the exact scan, 20-40x slower,
// and a launch lasts as long as its slowest episode) and the launch has an epoch of its own
int eg::prepare_heavy(eg_ctx* c, uint32_t n_heavy, bool known_short) {
  constexpr size_t kSlotBytes = size_t(kRadiusClasses) * 2624 * sizeof(double), kTileBytes = size_t(kMaxVariants) * 64 * sizeof(double);
  // No pool while the host KNOWS the best list to be short: replay episodes of a short list never ask for a slot.  (Not by the
  // pinned hint: the host enqueues a free-running loop many batches ahead of the device, the hint is as old as the queue is deep,
  // and a long replay episode without a slot takes the exact scan — 33 instead of 5 ms per batch, measured.)
  if (known_short && !c->dev.heavy) n_heavy = 0;
  uint32_t want = c->heavy_slots_wanted;
  if (c->heavy_slots_auto && want > 0) {      // 4 096 slots (516 MB) to begin with, then the next power of two, up to the budget
    while (want < n_heavy && want < c->heavy_slots_max) want = want * 2u < c->heavy_slots_max ? want * 2u : c->heavy_slots_max;
  }
  if (want > 0 && n_heavy > 0 && (!c->dev.heavy || want > c->dev.heavy_slots)) {
    if (c->dev.heavy) {      // earlier launches may still use the old pool
      EG_HIP(hipDeviceSynchronize());
      c->d_heavy.release();
      c->dev.heavy = nullptr; c->dev.heavy_slots = 0; c->dev.heavy_tiles = nullptr;
    }
    if (!c->dev.heavy_claim) {
      if (!c->d_heavy_claim.try_reserve(16)) { c->heavy_slots_wanted = 0; want = 0; }
      else { EG_HIP(hipMemset(c->d_heavy_claim, 0xFF, 64)); c->dev.heavy_claim = c->d_heavy_claim; }      // 0xFF..: an epoch no launch uses
    }
    while (want > 0 && !c->d_heavy.try_reserve((kSlotBytes + kTileBytes) * want)) {      // no memory for that many: fewer; none: heavy episodes take the exact scan
      want = want > 4096u ? want / 2u : 0u;
      c->heavy_slots_auto = false; c->heavy_slots_wanted = want;
    }
    if (want > 0) {
      c->dev.heavy = c->d_heavy; c->dev.heavy_slots = want;
      c->dev.heavy_tiles = reinterpret_cast<double*>(c->d_heavy + kSlotBytes * want);      // (the fields, then their tile bounds)
    }
  }
  c->launch_epoch = (c->launch_epoch + 1u) & 0xFFFu;
  if (c->launch_epoch == 0xFFFu) c->launch_epoch = 0u;      // 0xFFF is the "never" epoch the claim word starts with
  c->dev.heavy_epoch = c->launch_epoch;
  return EG_OK;
}

namespace {
// One batch = up to three grids of k_rollout (eg_internal.h RolloutPlan): the episodes that replay the best strategy on the
// two replay variants (one of which returns at once), the others on the lean one, on two streams side by side.  `host_mask` (n bytes, may be NULL):
// which episodes replay; otherwise `period` (0: none): episode i replays when (first_index + i) % period == 0.
// Uploads the mask and the index lists, takes a slot of the timing ring, gives the launch its field-pool epoch, launches.
int launch_batch(eg_ctx* c, uint64_t seed, uint64_t first_index, uint32_t n, const uint8_t* host_mask, uint32_t period, long long* d_stats) {
  if (n == 0) return EG_OK;
  RolloutPlan plan{};
  plan.helper_waves = n <= c->helper_max_episodes;
  plan.n_lean = n;
  const uint8_t* d_mask = nullptr;
  if (host_mask) {
    EG_HIP(c->d_mask.reserve(n));
    EG_HIP(c->d_index.reserve(n));
    std::vector<uint32_t> idx(n);
    uint32_t nh = 0;
    for (uint32_t i = 0; i < n; ++i) if (host_mask[i]) idx[nh++] = i;
    uint32_t k = nh;
    for (uint32_t i = 0; i < n; ++i) if (!host_mask[i]) idx[k++] = i;
    EG_HIP(hipMemcpy(c->d_mask, host_mask, n, hipMemcpyHostToDevice));
    EG_HIP(hipMemcpy(c->d_index, idx.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    d_mask = c->d_mask;
    plan.n_heavy = nh; plan.n_lean = n - nh; plan.mode = 1u; plan.d_index = c->d_index;
  } else if (period == 1u) {
    plan.n_heavy = n; plan.n_lean = 0;
  } else if (period > 1u) {
    plan.off = uint32_t((uint64_t(period) - first_index % period) % period);
    plan.n_heavy = plan.off < n ? (n - plan.off + period - 1u) / period : 0u;
    plan.n_lean = n - plan.n_heavy; plan.mode = 2u; plan.period = period;
  }
  int slot = 0;
  EG_TRY(ring_take(c, plan, slot));
  // A batch that is one kind of grid stays on the null stream like every other kernel of the library.  With both kinds the lean
  // grid still does; the replay grids go to a (non-blocking) stream of their own that forks off the null stream before them and
  // joins it after the lean grid's launch — two explicit events.  (They were two blocking streams at first: the implicit
  // null-stream synchronisation of those cost 30 us before the grids and 16 us after them, every batch.)
  const bool split = plan.n_heavy > 0 && plan.n_lean > 0;
  plan.stream_heavy = split ? c->stream_heavy : nullptr;
  plan.stream_lean = nullptr;
  // what the host knows about the best list: exactly (then only the replay variant with work is launched), or from the pinned word
  bool list_long = c->long_list_hint;
  if (!c->list_exact && c->h_list_len) list_long = *(volatile uint32_t*)c->h_list_len > uint32_t(kShortReplayMax);
  plan.skip_long = c->list_exact && !list_long;
  EG_TRY(prepare_heavy(c, plan.n_heavy, plan.skip_long));
  if (d_stats != nullptr) {      // the statistics epilogue adds to replicated arrays, folded into the packet behind the grids
    const bool off = stats_replicas_off();
    if (!off && n >= 4096u) {
      bool fresh = false;
      EG_HIP(c->d_stats_rep.reserve(size_t(kStatsReplicas) * EG_STATS_LEN, &fresh));
      if (fresh) EG_HIP(hipMemsetAsync(c->d_stats_rep, 0, sizeof(long long) * size_t(kStatsReplicas) * EG_STATS_LEN, nullptr));
    }
    // (small batches add directly: a few hundred episodes do not queue up in L2, and the fold is a launch of its own — configs[1],
    //  1 024 episodes: 0.257 ms per batch without it, 0.264 with)
    plan.d_stats_rep = (off || n < 4096u) ? nullptr : c->d_stats_rep;
    if (plan.d_stats_rep != nullptr && c->stats_rep_dirty) {      // (on the null stream, ahead of the fork to the replay stream;
      if (c->stream_heavy) EG_HIP(hipStreamSynchronize(c->stream_heavy));      //  replay grids of that batch that were never joined end first)
      EG_HIP(hipMemsetAsync(c->d_stats_rep, 0, sizeof(long long) * size_t(kStatsReplicas) * EG_STATS_LEN, nullptr));
      c->stats_rep_dirty = false;
    }
  }
  // long replay episodes: script / placements / rows, each on its own wave (eg_replay_solo.h) — unless the batch's replays are computed
  // once anyway (what ends that script ends this one as well: the classic variant alone is the fallback then)
  if (plan.n_heavy > 0 && !plan.helper_waves && !plan.skip_long && !c->hoist_on)
    EG_TRY(arm_solo(c, plan, plan.n_heavy));
  if (c->hoist_on && plan.n_heavy > 0) {      // the replay episodes of this batch are computed once (eg_replay_coop.h)
    plan.hoist_seq = ++c->hoist_seq; plan.d_hoist = reinterpret_cast<HoistInfo*>(c->d_hoist.ptr); plan.coop_out = c->d_coop; plan.coop_force = c->coop_force;
    c->hoist_batches += 1;
  }
  if (split) {
    EG_HIP(hipEventRecord(c->ev_fork[slot], nullptr));
    EG_HIP(hipStreamWaitEvent(c->stream_heavy, c->ev_fork[slot], 0));
    // The lean grid waits for an event recorded behind the short-replay variant — which has nothing to do and is gone in
    // microseconds — i.e. until the long variant is being dispatched.  The hold dates from when a long replay was a 256-register
    // wave and the batch's long pole (arriving behind 16 384 lean episodes it waited for two of them to finish on its SIMD: 5.6
    // instead of 4.95 ms per batch at 468 generators per replay).  Today a long replay is a 123-register wave of k_replay_lazy /
    // k_replay_solo in one slot, and at 228 generators per replay the lean grid ends the batch, so the hold (a 23 us grid and a
    // 6 us hop in the trace) sits on the critical path there; at 468 and 916 generators the replays still end it.  Launching the
    // replay kernel first and letting the lean grid go without the hold has not been measured: the order stands as it was.
    // With short replays (or when the host's idea of the list is out of date) nobody waits for anybody.
    // (the hoisted replay is one workgroup that needs a whole CU: it is dispatched ahead of the lean grid in any case)
    if (list_long || plan.hoist_seq != 0ull) plan.go_event = c->ev_go[slot];
  }
  if (plan.d_stats_rep != nullptr) c->stats_rep_dirty = true;      // until the fold is enqueued: every return before it leaves them dirty
  EG_LAUNCH("k_rollout", launch_rollout(c->dev, c->snap, c->out, seed, first_index, n, d_mask, period, d_stats, plan));
  if (split) {
    EG_HIP(hipEventRecord(c->ev_join[slot], c->stream_heavy));
    EG_HIP(hipStreamWaitEvent(nullptr, c->ev_join[slot], 0));
  }
  if (d_stats != nullptr && plan.d_stats_rep != nullptr) {
    EG_LAUNCH("k_fold_stats", launch_fold_stats(plan.d_stats_rep, d_stats, nullptr));
    c->stats_rep_dirty = false;
  }
  if (c->fold_mode != 0) EG_TRY(best_result_fold(c, n, first_index));      // behind the batch on the null stream: its results are in iteration order in the records
  if (c->topk_mode != 0) EG_TRY(topk_fold(c, n, first_index, d_stats != nullptr && c->topk_mode == 1));      // the top-K archive, behind the batch as well (the epilogue's scores are the rank scores in mode 1)
  if (c->pareto_cap != 0) EG_TRY(pareto_fold(c, n, first_index));      // the Pareto archive, behind the top-K fold
  ring_commit(c, slot, (plan.n_heavy > 0 ? 1 : 0) | (plan.n_lean > 0 ? 2 : 0));
  c->last_n = n; c->last_first = first_index; c->feas_k = 0; c->ran = {};
  return EG_OK;
}

// eg_create, on the context's device: the tables uploaded, the events and the side stream, the buffers a context always has
int create_device_state(eg_ctx* c, const std::vector<uint8_t>& blob, bool side_stream_plain) {
  if (c->d_tables.reserve(tab::total) != hipSuccess) { set_error("hipMalloc(tables) failed"); return EG_ERR_HIP; }
  c->dev.base = c->d_tables;
  if (hipMemcpy(c->d_tables, blob.data(), tab::total, hipMemcpyHostToDevice) != hipSuccess) { set_error("hipMemcpy(tables) failed"); return EG_ERR_HIP; }
  for (int i = 0; i < eg_ctx::kTimingRing; ++i)
    for (int k = 0; k < 4; ++k)
      if (hipEventCreate(&c->ev[i][k]) != hipSuccess) { set_error("hipEventCreate failed"); return EG_ERR_HIP; }
  // A priority of its own gives the stream a hardware queue of its own.  (A plain stream created after torch / RCCL have made
  // theirs ended up sharing one with the null stream: the grids of a batch then ran one after the other — measured.)
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  if ((side_stream_plain ? hipStreamCreateWithFlags(&c->stream_heavy, hipStreamNonBlocking)
                         : hipStreamCreateWithPriority(&c->stream_heavy, hipStreamNonBlocking, greatest)) != hipSuccess) { set_error("hipStreamCreate failed"); return EG_ERR_HIP; }
  for (int i = 0; i < eg_ctx::kTimingRing; ++i)
    if (hipEventCreateWithFlags(&c->ev_fork[i], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_go[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming) != hipSuccess) {
      set_error("hipEventCreate failed"); return EG_ERR_HIP;
    }
  if (c->d_snap.reserve(snap::total) != hipSuccess || c->h_snap.reserve(snap::total) != hipSuccess) { set_error("hipMalloc(snapshot) failed"); return EG_ERR_HIP; }
  if (hipMemset(c->d_snap, 0, snap::total) != hipSuccess) { set_error("hipMemset(snapshot) failed"); return EG_ERR_HIP; }
  // (a convenience, not a requirement: without it the hint stays what the host last knew)
  if (c->h_list_len.try_reserve(16, hipHostMallocMapped)) {
    *c->h_list_len = 0u;
    if (hipHostGetDevicePointer((void**)&c->d_list_len, c->h_list_len, 0) != hipSuccess) { (void)hipGetLastError(); c->d_list_len = nullptr; }
  }
  if (c->d_hoist.reserve(kHoistBytes) != hipSuccess || c->d_coop.reserve(rec::stride + 64) != hipSuccess ||
      hipMemset(c->d_hoist, 0, kHoistBytes) != hipSuccess || hipMemset(c->d_coop, 0, rec::stride + 64) != hipSuccess) {
    set_error("hipMalloc(replay hoist) failed"); return EG_ERR_HIP;
  }
  return EG_OK;
}

template <typename Map, typename T>
int find_table(const char* who, const Map& tables, const char* name, const T** ptr, int64_t* len) {      // eg_host_tables_f64 / _i32
  if (!name || !ptr || !len) return EG_ERR_BAD_ARG;
  auto it = tables.find(name);
  if (it == tables.end()) { set_error(std::string(who) + ": unknown table " + name); return EG_ERR_BAD_ARG; }
  *ptr = it->second.first; *len = it->second.second;
  return EG_OK;
}

int device_rollout(eg_ctx* c, uint64_t seed, uint64_t first_index, uint32_t n, uint32_t replay_period, void* d_packet, bool pick) {
  if (!c || !c->snap_valid || !d_packet) { set_error("eg_device_rollout: push a policy first"); return EG_ERR_BAD_ARG; }
  if (n == 0) { c->last_n = 0; c->feas_k = 0; c->ran = {}; return EG_OK; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_outputs(c, n));
  EG_TRY(launch_batch(c, seed, first_index, n, nullptr, replay_period, (long long*)d_packet));
  if (!pick) return EG_OK;
  EG_LAUNCH("k_pick_best", launch_pick_best(c->out, n, first_index, reinterpret_cast<UpdateCandidate*>(static_cast<uint8_t*>(d_packet) + 8 * EG_STATS_LEN), nullptr));
  return EG_OK;
}
}  // namespace

int eg::ensure_packet(eg_ctx* c) {      // eg_train_step / eg_device_step / eg_policy_push
  bool fresh = false;
  EG_HIP(c->d_packet.reserve(EG_PACKET_BYTES, &fresh));
  if (fresh) EG_HIP(hipMemset(c->d_packet, 0, EG_PACKET_BYTES));      // the rollout epilogue ADDS to the statistics
  EG_HIP(c->h_packet.reserve(EG_PACKET_BYTES));
  return EG_OK;
}

int eg::device_apply(eg_ctx* c, const void* d_packets, int32_t n_packets, size_t packet_stride, void* d_own_packet, uint64_t noise_seed, bool local_pick) {
  if (!c || !c->snap_valid || !d_packets || n_packets < 1 || !d_own_packet) { set_error("eg_device_apply: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  c->list_exact = false;      // from here on the device may hold another best list than the host thinks
  EG_LAUNCH("k_apply_update", launch_apply_update(c->d_snap, d_packets, n_packets, packet_stride, (long long*)d_own_packet, noise_seed, c->out, c->last_n, c->last_first,
                               local_pick && n_packets == 1 && c->last_n > 0, c->d_list_len, nullptr));
  // (the stalled sampler's tables of the updated rows are rebuilt inside k_apply_update)
  return EG_OK;
}

extern "C" {

const char* eg_last_error(void) { return g_error.c_str(); }

int32_t eg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

eg_ctx* eg_create(int32_t device_ordinal, const eg_world* world) {
  if (!world || world->n_settlements < 0 || world->n_existing < 0 || world->n_coast < 0) { set_error("eg_create: bad world"); return nullptr; }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("eg_create: no HIP device (this library has no CPU path)"); return nullptr; }
  if (device_ordinal < 0 || device_ordinal >= n) { set_error("eg_create: device ordinal out of range"); return nullptr; }
  if (hipSetDevice(device_ordinal) != hipSuccess) { set_error("eg_create: hipSetDevice failed"); return nullptr; }
  // The small-batch kernel holds 3 waves per episode at 3 waves per SIMD: 4 episodes per CU are resident together.
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) != hipSuccess) cus = 0;
  const Options opt = read_options();
  eg_ctx* c = new eg_ctx();
  c->device = device_ordinal;
  c->helper_max_episodes = opt.helper_off ? 0u : opt.helper_all ? 0xFFFFFFFFu : 4u * (uint32_t)(cus > 0 ? cus : 0);
  c->heavy_slots_wanted = opt.heavy_slots_wanted; c->heavy_slots_auto = opt.heavy_slots_auto; c->heavy_slots_max = opt.heavy_slots_max;
  build_tables(*world, c->tables.H);
  c->tables.index();
  std::vector<uint8_t> blob;
  BlobInfo info;
  int rc = build_device_blob(c->tables.H, blob, info);
  if (rc == EG_OK) {
    c->dev.n_variants = info.n_variants; c->dev.size_factor = c->tables.H.size_factor; c->dev.n_existing = world->n_existing;
    c->dev.solo_tiles = opt.solo_tiles; c->dev.solo_lazy = opt.solo_lazy;
    if (!info.box_list_fits) c->heavy_slots_wanted = 0;
    c->hoist_supported = info.hoist_supported; c->hoist_on = info.hoist_supported && opt.replay_hoist;
    c->coop_force = opt.coop_force; c->solo_on = opt.solo_on; c->uniform_on = opt.uniform_on;
    rc = create_device_state(c, blob, opt.side_stream_plain);
  }
  if (rc != EG_OK) { eg_destroy(c); return nullptr; }
  return c;
}

void eg_destroy(eg_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < eg_ctx::kTimingRing; ++i)
    for (int k = 0; k < 4; ++k) if (c->ev[i][k]) (void)hipEventDestroy(c->ev[i][k]);
  if (c->stream_heavy) (void)hipStreamDestroy(c->stream_heavy);
  for (int i = 0; i < eg_ctx::kTimingRing; ++i) { if (c->ev_fork[i]) (void)hipEventDestroy(c->ev_fork[i]); if (c->ev_go[i]) (void)hipEventDestroy(c->ev_go[i]); if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]); }
  delete c;      // (the buffers free themselves, on the device made current above)
}

eg_host_tables* eg_host_tables_create(const eg_world* world) {
  if (!world || world->n_settlements < 0 || world->n_existing < 0 || world->n_coast < 0) { set_error("eg_host_tables_create: bad world"); return nullptr; }
  eg_host_tables* h = new eg_host_tables();
  build_tables(*world, h->H);
  h->index();
  return h;
}
void eg_host_tables_free(eg_host_tables* h) { delete h; }
int32_t eg_host_tables_f64(const eg_host_tables* h, const char* name, const double** ptr, int64_t* len) {
  return h ? find_table("eg_host_tables_f64", h->f64, name, ptr, len) : EG_ERR_BAD_ARG;
}
int32_t eg_host_tables_i32(const eg_host_tables* h, const char* name, const int32_t** ptr, int64_t* len) {
  return h ? find_table("eg_host_tables_i32", h->i32, name, ptr, len) : EG_ERR_BAD_ARG;
}

int32_t eg_upload_snapshot(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o) {
  if (!c || !s || !s->weights || !s->deficit_weights) { set_error("eg_upload_snapshot: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(check_policy(s, o, "eg_upload_snapshot"));
  EG_HIP(hipSetDevice(c->device));
  const bool have_lists = s->has_best && s->best_count && s->best_actions && s->best_deficit_count && s->best_deficit_actions;
  int32_t len = 0, lend = 0;
  if (have_lists) for (int y = 0; y < EG_YEARS; ++y) { len += s->best_count[y]; lend += s->best_deficit_count[y]; }
  if (size_t(len) > snap::kBestCap || size_t(lend) > snap::kBestCap) { set_error("eg_upload_snapshot: best action lists too long"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipStreamSynchronize(nullptr));   // the pinned staging buffer may still feed the previous copy
  stage_policy(c, s, have_lists, c->h_snap);
  c->long_list_hint = have_lists && len > kShortReplayMax; c->list_exact = true;
  // (the pinned word is a HINT only — read when list_exact is false, to order the launches: an update or rewind kernel enqueued before
  //  this upload may still store an older length over this one; nothing but the launch order ever depends on it)
  if (c->h_list_len) *(volatile uint32_t*)c->h_list_len = have_lists ? uint32_t(len) : 0u;
  EG_HIP(hipMemcpyAsync(c->d_snap, c->h_snap, snap::upload_bytes, hipMemcpyHostToDevice, nullptr));   // stream-ordered before the next launch
  EG_LAUNCH("k_stalled_tables", launch_stalled_tables(c->d_snap, nullptr));      // sampling.rs:190-220 on the un-nudged rows (no-op unless stalled)
  c->snap = snapshot_of(c->d_snap, o);
  c->snap_valid = true;
  return EG_OK;
}

int32_t eg_rollout_launch(eg_ctx* c, uint64_t seed, uint64_t first_index, uint32_t n, const uint8_t* replay_mask) {
  if (!c || !c->snap_valid) { set_error("eg_rollout_launch: upload a snapshot first"); return EG_ERR_BAD_ARG; }
  if (n == 0) { c->last_n = 0; c->feas_k = 0; c->ran = {}; return EG_OK; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_outputs(c, n));
  return launch_batch(c, seed, first_index, n, replay_mask, 0u, nullptr);
}

int32_t eg_rollout_launch_update(eg_ctx* c, uint64_t seed, uint64_t first_index, uint32_t n, const uint8_t* replay_mask, void* d_packet) {
  if (!c || !c->snap_valid || !d_packet) { set_error("eg_rollout_launch_update: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_outputs(c, n ? n : 1));
  EG_HIP(hipMemsetAsync(d_packet, 0, EG_PACKET_BYTES, nullptr));
  c->last_n = n; c->last_first = first_index; c->feas_k = 0; c->ran = {};
  EG_TRY(launch_batch(c, seed, first_index, n, replay_mask, 0u, (long long*)d_packet));
  EG_LAUNCH("k_pick_best", launch_pick_best(c->out, n, first_index, reinterpret_cast<UpdateCandidate*>(static_cast<uint8_t*>(d_packet) + 8 * EG_STATS_LEN), nullptr));
  return EG_OK;
}

int32_t eg_debug_fill_lds(eg_ctx* c, uint32_t value) {
  if (!c) { set_error("eg_debug_fill_lds: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_outputs(c, 1));
  hipDeviceProp_t prop;
  EG_HIP(hipGetDeviceProperties(&prop, c->device));
  // 64 KB per workgroup: at most two share a CU's 160 KB, so 4 per CU in flight-order covers every slot several times
  EG_LAUNCH("k_fill_lds", launch_fill_lds(value, reinterpret_cast<uint32_t*>(c->out.base), prop.multiProcessorCount * 8, nullptr));
  EG_HIP(hipDeviceSynchronize());
  return EG_OK;
}

int32_t eg_debug_occupy(eg_ctx* c, int32_t variant, uint64_t cycles) {
  if (!c) return EG_ERR_BAD_ARG;
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_outputs(c, 1));
  EG_LAUNCH("k_occupy", launch_occupy(variant, cycles, reinterpret_cast<uint32_t*>(c->out.score_list), c->stream_heavy));      // the library's side stream
  return EG_OK;
}

int32_t eg_sync(eg_ctx* c) {
  if (!c) return EG_ERR_BAD_ARG;
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipDeviceSynchronize());
  return collect_timing(c);
}

int32_t eg_train_step(eg_ctx* c, eg_policy* p, const eg_opts* o, uint64_t seed, uint64_t first_index, uint32_t n,
                      const uint8_t* replay_mask, uint64_t noise_seed) {
  if (!c || !p) { set_error("eg_train_step: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_packet(c));
  eg_policy_snapshot snap;
  EG_TRY(eg_policy_snapshot_view(p, &snap));
  EG_TRY(eg_upload_snapshot(c, &snap, o));
  EG_TRY(eg_rollout_launch_update(c, seed, first_index, n, replay_mask, c->d_packet));
  EG_HIP(hipMemcpyAsync(c->h_packet, c->d_packet, EG_PACKET_BYTES, hipMemcpyDeviceToHost, nullptr));
  EG_HIP(hipStreamSynchronize(nullptr));
  return eg_policy_apply_packet(p, reinterpret_cast<const int64_t*>(c->h_packet.ptr), c->h_packet + 8 * EG_STATS_LEN, 1, noise_seed);
}

// ---- device-resident policy: push once, step without host synchronisation, pull when needed -----------------------

int32_t eg_policy_push(eg_ctx* c, const eg_policy* p, const eg_opts* o) {
  if (!c || !p) { set_error("eg_policy_push: bad argument"); return EG_ERR_BAD_ARG; }
  eg_policy_snapshot snap;
  EG_TRY(eg_policy_snapshot_view(p, &snap));
  c->push_iteration_count = p->iteration_count; c->push_failed = p->failed_episodes;
  const int rc = eg_upload_snapshot(c, &snap, o);
  c->push_iteration_count = 0; c->push_failed = 0;
  if (rc != EG_OK) return rc;
  c->pulled_improvements = 0;
  EG_TRY(ensure_packet(c));
  EG_HIP(hipMemsetAsync(c->d_packet, 0, EG_PACKET_BYTES, nullptr));
  {  // the kept record of the best episode (eg_fetch_best_run) survives a push only when it is the pushed policy's best
     // strategy (checkpoint / resume on the same context); a record left by another policy is dropped
    uint32_t word = 0; double m[4] = {0, 0, 0, 0};
    EG_HIP(hipMemcpy(&word, c->d_snap + snap::best_rec_state, sizeof(word), hipMemcpyDeviceToHost));
    if (word == 1u) EG_HIP(hipMemcpy(m, c->d_snap + snap::best_rec + rec::metrics, sizeof(m), hipMemcpyDeviceToHost));
    const bool same = word == 1u && p->has_best && std::memcmp(m, p->best_metrics.data(), sizeof(m)) == 0;
    if (word != 0u && !same) EG_HIP(hipMemsetAsync(c->d_snap + snap::best_rec_state, 0, sizeof(uint32_t), nullptr));
  }
  // main weights at the last improvement travel with the policy
  if (p->has_best_weights) EG_HIP(hipMemcpyAsync(c->d_snap + snap::best_w, p->best_w.data(), sizeof(double) * EG_YEARS * EG_N_ACTIONS, hipMemcpyHostToDevice, nullptr));
  EG_HIP(hipStreamSynchronize(nullptr));      // p->best_w is pageable host memory
  return EG_OK;
}

int32_t eg_device_rollout(eg_ctx* c, uint64_t seed, uint64_t first_index, uint32_t n, uint32_t replay_period, void* d_packet) {
  return device_rollout(c, seed, first_index, n, replay_period, d_packet, true);
}
int32_t eg_device_apply(eg_ctx* c, const void* d_packets, int32_t n_packets, void* d_own_packet, uint64_t noise_seed) {
  return device_apply(c, d_packets, n_packets, EG_PACKET_BYTES, d_own_packet, noise_seed, false);
}
// One GPU: the best episode is found inside k_apply_update (from the best-score key the rollout epilogue leaves in the
// statistics), so a step is three launches: k_rollout, k_apply_update, k_stalled_tables.
int32_t eg_device_step(eg_ctx* c, uint64_t seed, uint64_t first_index, uint32_t n, uint32_t replay_period, uint64_t noise_seed) {
  if (!c) return EG_ERR_BAD_ARG;
  if (n == 0) return EG_OK;
  EG_TRY(ensure_packet(c));
  EG_TRY(device_rollout(c, seed, first_index, n, replay_period, c->d_packet, false));
  return device_apply(c, c->d_packet, 1, EG_PACKET_BYTES, c->d_packet, noise_seed, true);
}

int32_t eg_replay_hoist(eg_ctx* c, int32_t on) {
  if (!c) { set_error("eg_replay_hoist: bad argument"); return EG_ERR_BAD_ARG; }
  if (on && !c->hoist_supported) { set_error("eg_replay_hoist: this world's penalty radii / type variants exceed what the hoisted replay is sized for"); return EG_ERR_UNSUPPORTED; }
  c->hoist_on = on != 0;
  return EG_OK;
}

int32_t eg_replay_hoist_stats(eg_ctx* c, uint64_t* batches_armed, int32_t* last_batch_hoisted) {
  if (!c) return EG_ERR_BAD_ARG;
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipDeviceSynchronize());
  unsigned long long word = 0;
  EG_HIP(hipMemcpy(&word, c->d_hoist, sizeof(word), hipMemcpyDeviceToHost));
  if (batches_armed) *batches_armed = c->hoist_batches;
  static_assert(offsetof(HoistInfo, served_seq) == 0, "the served word comes first");
  if (last_batch_hoisted) *last_batch_hoisted = (c->hoist_seq != 0ull && word == c->hoist_seq) ? 1 : 0;
  return EG_OK;
}

int32_t eg_debug_hoist_stamps(eg_ctx* c, uint64_t stamps[8]) {
  if (!c || !stamps) return EG_ERR_BAD_ARG;
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipDeviceSynchronize());
  EG_HIP(hipMemcpy(stamps, c->d_hoist + offsetof(HoistInfo, stamps), 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return EG_OK;
}

int32_t eg_policy_hold(eg_ctx* c) {
  if (!c || !c->snap_valid) { set_error("eg_policy_hold: push a policy first"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(c->d_snap_held.reserve(snap::total));
  EG_HIP(hipMemcpyAsync(c->d_snap_held, c->d_snap, snap::total, hipMemcpyDeviceToDevice, nullptr));
  // What the host knows about the list it is holding travels with the copy: a hold behind on-device updates that nobody has pulled
  // (list_exact == false) must not come back from a rewind as "known to be short" — the long-replay variant would not be launched
  // and the replay episodes' records would keep the previous batch's bytes.
  c->long_list_hint_held = c->long_list_hint; c->list_exact_held = c->list_exact;
  return EG_OK;
}

int32_t eg_policy_rewind(eg_ctx* c) {
  if (!c || !c->d_snap_held) { set_error("eg_policy_rewind: nothing held"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  // (the count of failed episodes is a diagnostic of the run, not policy: it goes on counting; one small kernel instead of two copies)
  EG_LAUNCH("k_rewind", launch_rewind(c->d_snap, c->d_snap_held, c->d_list_len, nullptr));
  // the next launch finds the held policy's list: the host knows it exactly when it knew it at the hold; otherwise both replay
  // variants are launched and decide on the device (k_rewind publishes the held list's length through the pinned word for the order)
  c->long_list_hint = c->long_list_hint_held; c->list_exact = c->list_exact_held;
  return EG_OK;
}

int32_t eg_policy_pull(eg_ctx* c, eg_policy* p) {
  if (!c || !p || !c->snap_valid) { set_error("eg_policy_pull: push a policy first"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipStreamSynchronize(nullptr));
  std::vector<uint8_t> h(snap::total);
  EG_HIP(hipMemcpy(h.data(), c->d_snap, snap::total, hipMemcpyDeviceToHost));
  const double* pol = reinterpret_cast<const double*>(h.data() + snap::pol);
  DevState st; std::memcpy(&st, h.data() + snap::state, sizeof(st));
  for (int y = 0; y < EG_YEARS; ++y) {
    const double* row = pol + y * snap::kPolRow;
    for (int a = 0; a < EG_N_ACTIONS; ++a) p->w[y][a] = row[a];
    for (int i = 0; i < EG_N_DEFICIT; ++i) p->dw[y][i] = row[snap::kPolDw + i];
  }
  p->stall = st.stall; p->iteration_count = st.iteration_count; p->failed_episodes = st.failed_total;
  c->long_list_hint = st.has_lists && reinterpret_cast<const int32_t*>(h.data() + snap::best_off)[EG_YEARS] > kShortReplayMax;
  c->list_exact = true;      // (the stream was drained above: nothing is in flight that could change it)
  if (st.n_improvements > 0) {      // at least one on-device improvement since the push: the best strategy is the device's
    p->has_best = true; for (int i = 0; i < 4; ++i) p->best_metrics[i] = st.best_metrics[i];
    const int32_t* off = reinterpret_cast<const int32_t*>(h.data() + snap::best_off);
    const int32_t* offd = reinterpret_cast<const int32_t*>(h.data() + snap::bestd_off);
    for (int y = 0; y < EG_YEARS; ++y) {
      p->best_actions[y].assign(h.data() + snap::best_actions + off[y], h.data() + snap::best_actions + off[y + 1]);
      p->best_deficit[y].assign(h.data() + snap::bestd_actions + offd[y], h.data() + snap::bestd_actions + offd[y + 1]);
      p->cur_run[y] = p->best_actions[y]; p->cur_def[y] = p->best_deficit[y];
    }
    p->has_best_actions = true; p->has_best_deficit = true; p->has_best_weights = true;
    std::memcpy(p->best_w.data(), h.data() + snap::best_w, sizeof(double) * EG_YEARS * EG_N_ACTIONS);
  }
  if (st.n_improvements > c->pulled_improvements) {      // history records are appended once per context, whichever policy pulls
    const DevImprovement* log = reinterpret_cast<const DevImprovement*>(h.data() + snap::imp_log);
    uint32_t from = c->pulled_improvements;
    if (st.n_improvements - from > uint32_t(snap::kImpLogCap)) from = st.n_improvements - uint32_t(snap::kImpLogCap);   // ring overwrote older ones
    const uint32_t keep = p->iteration_count;
    for (uint32_t k = from; k < st.n_improvements; ++k) {
      const DevImprovement& e = log[k % snap::kImpLogCap];
      p->iteration_count = e.iteration;
      p->record_improvement(e.score, e.metrics);
    }
    p->iteration_count = keep;
    c->pulled_improvements = st.n_improvements;
  }
  return EG_OK;
}

int32_t eg_rollout_batch(eg_ctx* c, const eg_policy_snapshot* s, const eg_opts* o, uint64_t seed, uint64_t first_index,
                         uint32_t n, const uint8_t* replay_mask, eg_episode_out* out) {
  EG_TRY(eg_upload_snapshot(c, s, o));
  EG_TRY(eg_rollout_launch(c, seed, first_index, n, replay_mask));
  return eg_fetch(c, out);
}

int32_t eg_timing_reset(eg_ctx* c) {
  if (!c) return EG_ERR_BAD_ARG;
  int rc = collect_timing(c);
  c->total_ms = 0.0; c->grids_ms = 0.0; c->n_launches = 0;
  return rc;
}
int32_t eg_timing_read_grids(eg_ctx* c, double* span_ms, double* grids_ms, int32_t* n_launches) {
  if (!c) return EG_ERR_BAD_ARG;
  int rc = collect_timing(c);
  if (span_ms) *span_ms = c->total_ms;
  if (grids_ms) *grids_ms = c->grids_ms;
  if (n_launches) *n_launches = c->n_launches;
  return rc;
}
int32_t eg_timing_read(eg_ctx* c, double* total_ms, int32_t* n_launches) { return eg_timing_read_grids(c, total_ms, nullptr, n_launches); }

int32_t eg_update_stats(eg_ctx* c, int64_t* d_stats) {
  if (!c || !d_stats || !c->snap_valid) { set_error("eg_update_stats: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * EG_STATS_LEN, nullptr));
  EG_LAUNCH("k_update_stats", launch_update_stats(c->snap, c->out, c->last_n, (long long*)d_stats, nullptr));
  return EG_OK;
}


}  // extern "C"
