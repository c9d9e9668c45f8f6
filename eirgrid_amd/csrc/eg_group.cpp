// eg_group.cpp — eg_group: N ranks, one context each, driven from one host thread.
// A step shards the global batch (parallel.shard_range), runs every rank's shard, exchanges one message per rank — its update
// packet, followed by its fold block when the best_result fold is tracked and, at the fixed offset topk_off behind the fold block's
// room, its top-K block when the top-K archive is — into every rank's gathered buffer, and applies the N
// packets on every rank (the statistics are integer sums, the candidate choice is order-free: every rank makes the same update).
// Nothing synchronises the host inside a step; the order comes from events, on the legacy null stream of each rank's device:
//   ev_sent[r]  recorded by rank r behind its rollout and its message (fold block / empty-shard packet);
//   ev_recv[q]  recorded by rank q behind the N copies into its gathered buffer, each of which waited for ev_sent of its sender.
// Read after write: rank q's apply and fold follow the copies into its gathered buffer on q's own stream, and every copy follows
// the sender's ev_sent — an apply never starts before all N messages have arrived.  Write after read: rank r's apply (which zeroes
// its packet's statistics) and everything after it on r's stream — its next rollout and message — wait for ev_recv of every
// other rank, i.e. until every peer has copied r's message; a rank's gathered buffer is only written again by the next step's
// copies, which its own stream orders behind this step's apply and fold.  (Ranks that share a device share its null stream, so
// there the order holds twice over; the events are what keeps it on separate devices.)
#include <algorithm>
#include <cstring>

#include "eg_host.h"

using namespace eg;

struct eg_group {
  int n = 0;
  std::vector<eg_ctx*> ctx;
  std::vector<int> device;
  // rank r's message (update packet, then FoldEntry[cap], then a TopKBlock at topk_off) and its gathered buffer (n slots of `stride`
  // bytes, rank order)
  std::vector<DevBuf<uint8_t>> d_send, d_gather;
  size_t stride = 0, topk_off = 0; uint32_t cap = 0;
  std::vector<hipEvent_t> ev_sent, ev_recv;
  int fold_mode = 0; std::vector<DevBuf<uint8_t>> d_fold;      // GroupFoldState + the record, per rank
  int topk_mode = 0, topk_k = 0; std::vector<DevBuf<uint8_t>> d_topk;      // the top-K archive per rank: replicated state, the records this rank ran
  uint32_t step = 0;         // steps run: the tag of a take-over
  bool pushed = false;
};

namespace {
void shard(uint32_t total, int rank, int n, uint32_t& first, uint32_t& count) {      // parallel.shard_range
  const uint32_t base = total / uint32_t(n), rem = total % uint32_t(n);
  count = base + (uint32_t(rank) < rem ? 1u : 0u);
  first = uint32_t(rank) * base + std::min(uint32_t(rank), rem);
}
int group_sync(eg_group* g) {
  for (int r = 0; r < g->n; ++r) { EG_HIP(hipSetDevice(g->device[r])); EG_HIP(hipDeviceSynchronize()); }
  return EG_OK;
}
// messages of up to `cap` results per rank (grown with a synchronisation: the buffers may be in use by the previous step)
int group_buffers(eg_group* g, uint32_t cap) {
  if (g->d_send[0] && cap <= g->cap) return EG_OK;
  EG_TRY(group_sync(g));
  g->cap = 0;      // (until every rank holds the larger buffers)
  const size_t topk_off = (size_t(EG_PACKET_BYTES) + sizeof(FoldEntry) * cap + 255) & ~size_t(255);
  const size_t stride = (topk_off + sizeof(TopKBlock) + 255) & ~size_t(255);
  for (int r = 0; r < g->n; ++r) {
    EG_HIP(hipSetDevice(g->device[r]));
    EG_HIP(g->d_send[r].reserve(stride));
    EG_HIP(g->d_gather[r].reserve(stride * size_t(g->n)));
    EG_HIP(hipMemset(g->d_send[r], 0, stride));      // the rollout epilogue ADDS to the statistics
    EG_HIP(hipMemset(g->d_gather[r], 0, stride * size_t(g->n)));
  }
  g->cap = cap; g->stride = stride; g->topk_off = topk_off;
  return EG_OK;
}
}  // namespace

extern "C" {

eg_group* eg_group_create(const int32_t* devices, int32_t n_ranks, const eg_world* world) {
  if (!devices || n_ranks < 1 || !world) { set_error("eg_group_create: bad argument"); return nullptr; }
  const int count = eg_device_count();
  for (int r = 0; r < n_ranks; ++r)
    if (devices[r] < 0 || devices[r] >= count) { set_error("eg_group_create: device " + std::to_string(devices[r]) + " does not exist (" + std::to_string(count) + " visible)"); return nullptr; }
  eg_group* g = new eg_group();
  g->n = n_ranks;
  g->device.assign(devices, devices + n_ranks);
  g->ctx.assign(n_ranks, nullptr); g->d_send.resize(n_ranks); g->d_gather.resize(n_ranks); g->d_fold.resize(n_ranks); g->d_topk.resize(n_ranks);
  g->ev_sent.assign(n_ranks, nullptr); g->ev_recv.assign(n_ranks, nullptr);
  bool ok = true;
  for (int r = 0; r < n_ranks && ok; ++r) {
    g->ctx[r] = eg_create(devices[r], world);
    if (!g->ctx[r]) { ok = false; break; }
    g->ctx[r]->group_member = true;
    if (hipEventCreateWithFlags(&g->ev_sent[r], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_recv[r], hipEventDisableTiming) != hipSuccess) { set_error("eg_group_create: hipEventCreate failed"); ok = false; }
  }
  // direct access between distinct devices where the platform offers it (the copies work without it, staged)
  for (int a = 0; a < n_ranks && ok; ++a)
    for (int b = 0; b < n_ranks; ++b) {
      if (g->device[a] == g->device[b]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, g->device[a], g->device[b]) == hipSuccess && can && hipSetDevice(g->device[a]) == hipSuccess)
        (void)hipDeviceEnablePeerAccess(g->device[b], 0);
      (void)hipGetLastError();      // (already enabled: not an error)
    }
  if (!ok) { const std::string e = eg_last_error(); eg_group_destroy(g); set_error(e); return nullptr; }
  return g;
}

void eg_group_destroy(eg_group* g) {
  if (!g) return;
  (void)group_sync(g);
  for (int r = 0; r < g->n; ++r) {      // every rank's buffers go on its own device
    (void)hipSetDevice(g->device[r]);
    g->d_send[r].release(); g->d_gather[r].release(); g->d_fold[r].release(); g->d_topk[r].release();
    if (g->ev_sent[r]) (void)hipEventDestroy(g->ev_sent[r]);
    if (g->ev_recv[r]) (void)hipEventDestroy(g->ev_recv[r]);
    eg_destroy(g->ctx[r]);
  }
  delete g;
}

eg_ctx* eg_group_rank(eg_group* g, int32_t rank) {
  if (!g || rank < 0 || rank >= g->n) { set_error("eg_group_rank: bad argument"); return nullptr; }
  return g->ctx[rank];
}

int32_t eg_group_push(eg_group* g, const eg_policy* p, const eg_opts* o) {
  if (!g || !p) { set_error("eg_group_push: bad argument"); return EG_ERR_BAD_ARG; }
  for (int r = 0; r < g->n; ++r)
    EG_TRY(eg_policy_push(g->ctx[r], p, o));
  g->pushed = true;
  return EG_OK;
}

int32_t eg_group_pull(eg_group* g, int32_t rank, eg_policy* p) {
  if (!g || rank < 0 || rank >= g->n || !p) { set_error("eg_group_pull: bad argument"); return EG_ERR_BAD_ARG; }
  return eg_policy_pull(g->ctx[rank], p);
}

int32_t eg_group_replay_hoist(eg_group* g, int32_t on) {
  if (!g) { set_error("eg_group_replay_hoist: bad argument"); return EG_ERR_BAD_ARG; }
  for (int r = 0; r < g->n; ++r)
    EG_TRY(eg_replay_hoist(g->ctx[r], on));
  return EG_OK;
}

int32_t eg_group_best_result_track(eg_group* g, int32_t mode) {
  if (!g || mode < 0 || mode > 2) { set_error("eg_group_best_result_track: bad argument"); return EG_ERR_BAD_ARG; }
  if (mode != 0)
    for (int r = 0; r < g->n; ++r) {
      EG_HIP(hipSetDevice(g->device[r]));
      EG_TRY(fold_reset(g->d_fold[r]));      // best_result = None; no record tagged (steps count from 1)
    }
  g->fold_mode = mode;
  return EG_OK;
}

int32_t eg_group_top_k_track(eg_group* g, int32_t k, int32_t mode) {
  if (!g || mode < 0 || mode > 2 || (mode != 0 && (k < 1 || k > EG_TOPK_MAX))) { set_error("eg_group_top_k_track: bad argument (1 <= k <= EG_TOPK_MAX, mode 0..2)"); return EG_ERR_BAD_ARG; }
  if (mode != 0) {
    for (int r = 0; r < g->n; ++r) {
      EG_HIP(hipSetDevice(g->device[r]));
      EG_TRY(topk_reset(g->d_topk[r], k, mode));      // (no slot tagged: steps count from 1)
    }
    g->topk_k = k;
  }
  g->topk_mode = mode;
  return EG_OK;
}

int32_t eg_group_step(eg_group* g, uint64_t seed, uint64_t first_index, uint32_t n_global, uint32_t replay_period, uint64_t noise_seed) {
  if (!g || !g->pushed) { set_error("eg_group_step: push a policy first (eg_group_push)"); return EG_ERR_BAD_ARG; }
  if (n_global == 0) return EG_OK;
  const int N = g->n;
  const bool fold = g->fold_mode != 0, topk = g->topk_mode != 0;
  EG_TRY(group_buffers(g, n_global / uint32_t(N) + (n_global % uint32_t(N) ? 1u : 0u)));
  g->step += 1;
  // 1. every rank runs its shard; its message is completed behind the rollout and marked sent
  for (int r = 0; r < N; ++r) {
    uint32_t first = 0, n = 0;
    shard(n_global, r, N, first, n);
    eg_ctx* c = g->ctx[r];
    EG_TRY(eg_device_rollout(c, seed, first_index + first, n, replay_period, g->d_send[r]));
    EG_HIP(hipSetDevice(g->device[r]));
    if (n == 0 || fold)      // an empty shard's packet still holds the previous step's candidate: it says "none" instead
      EG_LAUNCH("k_fold_pack", launch_fold_pack(c->out, n, g->d_send[r], reinterpret_cast<FoldEntry*>(g->d_send[r] + EG_PACKET_BYTES), nullptr));
    if (topk) {      // the shard's own top-k distinct entries (against this rank's replica of the archive); an empty shard: none
      if (n > 0) EG_TRY(topk_select(c, n, first_index + first, g->topk_mode, g->topk_mode == 1, g->d_topk[r], g->topk_k));
      EG_LAUNCH("k_topk_merge", launch_topk_merge(nullptr, reinterpret_cast<const uint8_t*>(c->d_tk_blocks.ptr), n > 0 ? int(topk_chunks(n)) : 0, sizeof(TopKBlock),
                                       reinterpret_cast<TopKBlock*>(g->d_send[r] + g->topk_off), g->topk_k, c->out, 0, 0, 0u, nullptr));
    }
    EG_HIP(hipEventRecord(g->ev_sent[r], nullptr));
  }
  // 2. every rank receives every message into slot r of its gathered buffer (read after write: each copy waits for its sender)
  for (int q = 0; q < N; ++q) {
    EG_HIP(hipSetDevice(g->device[q]));
    for (int r = 0; r < N; ++r) {
      uint32_t first = 0, n = 0;
      shard(n_global, r, N, first, n);
      const size_t bytes = size_t(EG_PACKET_BYTES) + (fold ? sizeof(FoldEntry) * n : 0);
      uint8_t* dst = g->d_gather[q] + size_t(r) * g->stride;
      EG_HIP(hipStreamWaitEvent(nullptr, g->ev_sent[r], 0));
      auto copy = [&](size_t off, size_t count) {      // the same bytes of r's message into slot r
        return g->device[r] == g->device[q] ? hipMemcpyAsync(dst + off, g->d_send[r] + off, count, hipMemcpyDeviceToDevice, nullptr)
                                            : hipMemcpyPeerAsync(dst + off, g->device[q], g->d_send[r] + off, g->device[r], count, nullptr);
      };
      EG_HIP(copy(0, bytes));
      if (topk) EG_HIP(copy(g->topk_off, sizeof(TopKBlock)));
    }
    EG_HIP(hipEventRecord(g->ev_recv[q], nullptr));
  }
  // 3. every rank applies the N packets and folds the N blocks (write after read: not before every peer holds its message)
  for (int r = 0; r < N; ++r) {
    EG_HIP(hipSetDevice(g->device[r]));
    for (int q = 0; q < N; ++q) if (q != r) EG_HIP(hipStreamWaitEvent(nullptr, g->ev_recv[q], 0));
    eg_ctx* c = g->ctx[r];
    EG_TRY(device_apply(c, g->d_gather[r], N, g->stride, g->d_send[r], noise_seed, false));
    uint32_t first = 0, n = 0;
    shard(n_global, r, N, first, n);
    if (fold)
      EG_LAUNCH("k_fold_gathered", launch_fold_gathered(g->d_gather[r], g->stride, N, n_global, first_index, c->out, first, n, g->fold_mode == 2, g->step, g->d_fold[r], nullptr));
    if (topk)      // the N blocks into this rank's replica; the records of new entries its own shard ran are copied and tagged here
      EG_LAUNCH("k_topk_merge", launch_topk_merge(g->d_topk[r], g->d_gather[r] + g->topk_off, N, g->stride, nullptr, g->topk_k, c->out, first_index + first, n, g->step, nullptr));
  }
  return EG_OK;
}

int32_t eg_group_fetch_best_result(eg_group* g, eg_episode_out* o, int32_t* state, int64_t* global_index) {
  if (!g || !o || !state) { set_error("eg_group_fetch_best_result: bad argument"); return EG_ERR_BAD_ARG; }
  if (!g->d_fold[0] || g->fold_mode == 0) { set_error("eg_group_fetch_best_result: eg_group_best_result_track first"); return EG_ERR_BAD_ARG; }
  EG_TRY(group_sync(g));
  std::vector<GroupFoldState> st(g->n);
  for (int r = 0; r < g->n; ++r) {
    EG_HIP(hipSetDevice(g->device[r]));
    EG_HIP(hipMemcpy(&st[r], g->d_fold[r], sizeof(GroupFoldState), hipMemcpyDeviceToHost));
    if (std::memcmp(st[r].metrics, st[0].metrics, sizeof(st[0].metrics)) != 0 || st[r].index != st[0].index || st[r].has != st[0].has ||
        st[r].step != st[0].step) { set_error("eg_group_fetch_best_result: the ranks' fold states differ"); return EG_ERR_INTERNAL; }
  }
  *state = st[0].has ? 1 : 0;
  if (global_index) *global_index = st[0].has ? int64_t(st[0].index) : -1;
  if (!st[0].has) return EG_OK;
  for (int r = 0; r < g->n; ++r)
    if (st[r].tag_index == st[0].index && st[r].tag_step == st[0].step) {
      EG_HIP(hipSetDevice(g->device[r]));
      return fetch_records(g->d_fold[r] + kFoldRecord, 1, o);
    }
  set_error("eg_group_fetch_best_result: no rank holds the record of the held run");
  return EG_ERR_INTERNAL;
}

int32_t eg_group_fetch_top_k(eg_group* g, eg_episode_out* o, int32_t* n_held, double* scores, int64_t* global_index) {
  if (!g || !o || !n_held) { set_error("eg_group_fetch_top_k: bad argument"); return EG_ERR_BAD_ARG; }
  if (!g->d_topk[0]) { set_error("eg_group_fetch_top_k: eg_group_top_k_track first"); return EG_ERR_BAD_ARG; }
  EG_TRY(group_sync(g));
  std::vector<TopKState> st(g->n);
  for (int r = 0; r < g->n; ++r) {
    EG_HIP(hipSetDevice(g->device[r]));
    EG_HIP(hipMemcpy(&st[r], g->d_topk[r], sizeof(TopKState), hipMemcpyDeviceToHost));
    if (st[r].n_held != st[0].n_held || st[r].k != st[0].k ||
        std::memcmp(st[r].e, st[0].e, sizeof(TopKEntry) * size_t(std::max(0, std::min(st[0].n_held, EG_TOPK_MAX)))) != 0) {
      set_error("eg_group_fetch_top_k: the ranks' archives differ"); return EG_ERR_INTERNAL;
    }
  }
  auto archive_of = [&](int i, const TopKEntry& e) -> const uint8_t* {      // the rank that ran the entry's episode keeps its record
    for (int r = 0; r < g->n; ++r)
      if (st[r].tag_index[e.slot] == e.index && st[r].tag_step[e.slot] == e.step) {
        if (hipSetDevice(g->device[r]) != hipSuccess) { set_error("eg_group_fetch_top_k: hipSetDevice failed"); return nullptr; }
        return g->d_topk[r];
      }
    set_error("eg_group_fetch_top_k: no rank holds the record of entry " + std::to_string(i));
    return nullptr;
  };
  return fetch_topk_rows("eg_group_fetch_top_k", st[0], archive_of, o, n_held, scores, global_index);
}

}  // extern "C"

