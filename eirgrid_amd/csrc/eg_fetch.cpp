// eg_fetch.cpp — results back to the host: the records of the last batch, the best run, the best_result fold, the top-K archive and the
// Pareto archive of one context (tracking and fetch), what the context holds in HBM.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "eg_host.h"
#define EG_RM static inline
#include "eg_reduced_math.h"

using namespace eg;

// The top-K fold's first two steps over the n results of the last batch in c->out (global indices first_index..): rank scores and keys
// against the archive at d_state, then every chunk's top-k distinct entries into c->d_tk_blocks (ceil(n / kTopKChunk) blocks).
int eg::topk_select(eg_ctx* c, uint32_t n, uint64_t first_index, int mode, bool use_score_list, const uint8_t* d_state, int k) {
  EG_HIP(c->d_tk_score.reserve(n));
  EG_HIP(c->d_tk_key.reserve(n));
  EG_HIP(c->d_tk_blocks.reserve(topk_chunks(n)));
  int lr = launch_topk_keys(c->out, n, first_index, mode, use_score_list, d_state, c->d_tk_score, c->d_tk_key, nullptr);
  if (lr == 0) lr = launch_topk_select(c->out, n, first_index, c->d_tk_score, c->d_tk_key, k, c->d_tk_blocks, nullptr);
  EG_LAUNCH("k_topk_keys / k_topk_select", lr);
  return EG_OK;
}

int eg::best_result_fold(eg_ctx* c, uint32_t n, uint64_t first_index) {
  EG_LAUNCH("k_fold_best", launch_fold_best(c->out, n, first_index, c->fold_mode == 2, c->d_fold, nullptr));
  return EG_OK;
}

int eg::topk_fold(eg_ctx* c, uint32_t n, uint64_t first_index, bool use_score_list) {
  EG_TRY(topk_select(c, n, first_index, c->topk_mode, use_score_list, c->d_topk, c->topk_k));
  EG_LAUNCH("k_topk_merge", launch_topk_merge(c->d_topk, reinterpret_cast<const uint8_t*>(c->d_tk_blocks.ptr), int(topk_chunks(n)), sizeof(TopKBlock), nullptr,
                                   c->topk_k, c->out, first_index, n, 0u, nullptr));
  return EG_OK;
}

int eg::pareto_fold(eg_ctx* c, uint32_t n, uint64_t first_index) {
  if (n == 0) return EG_OK;
  if (n > c->pareto_work_n || !c->d_pareto_work) {      // (a larger batch than any before: the old buffer is freed behind the launches that use it)
    EG_HIP(c->d_pareto_work.reserve(pareto_work_bytes(n)));
    c->pareto_work_n = n;
  }
  EG_LAUNCH("k_pareto_filter .. k_pareto_finalize", launch_pareto_fold(c->d_pareto, pareto_work(c->d_pareto_work, c->pareto_work_n), c->out, n, first_index, c->pareto_spread, nullptr));
  return EG_OK;
}

// One strided copy per requested field: episode records are rec::stride bytes apart on the device.  The lists of a record have the
// oracle's capacity (4 096 entries: 41.6 KB per episode), an episode fills a fraction of it (a sampled one about 1 KB): the counts
// come first, and every list is then copied only as wide as the longest of the batch needs — the caller's rows keep their full
// pitch, what lies behind an episode's entries is left as the caller passed it — except for the single-record fetches (N == 1:
// eg_fetch_record, eg_fetch_best_run, eg_fetch_best_result), whose rows are zeroed behind the entries: a C caller with an
// uninitialised buffer gets a defined row there, and it costs nothing.  (EIRGRID_FETCH_FULL=1: whole rows, for the
// diagnostic builds that park their cycle stamps at the end of act_log.)
int eg::fetch_records(const uint8_t* d_base, size_t N, eg_episode_out* o) {
#define EG_GET_W(field, count, type, used) \
  if (o->field && (used) > 0) EG_HIP(hipMemcpy2D(o->field, (count) * sizeof(type), d_base + rec::field, rec::stride, (used) * sizeof(type), N, hipMemcpyDeviceToHost)); \
  if (o->field && N == 1 && size_t(used) < size_t(count)) std::memset(o->field + (used), 0, (size_t(count) - size_t(used)) * sizeof(type))      /* one record: its rows end in zeros */
#define EG_GET(field, count, type) EG_GET_W(field, count, type, count)
  EG_GET(metrics, 4, double); EG_GET(yearly, EG_YEARS * EG_YEARLY_FIELDS, double); EG_GET(status, 1, int32_t);
  EG_GET(n_gens, 1, int32_t); EG_GET(n_offsets, 1, int32_t);
  EG_GET(bytes_moved, 1, double);
  EG_GET(n_draws, 1, uint64_t);
  EG_GET(n_chunks, 1, uint32_t);
  const bool full = fetch_full();
  size_t run = EG_RUN_CAP, def = EG_DEF_CAP, act = EG_ACT_CAP, gens = EG_MAX_GENS, offs = EG_MAX_OFFSETS;
  const bool lists = o->run_log || o->def_log || o->act_log || o->gen_cell || o->gen_pack || o->off_pack;
  std::vector<int32_t> cnt;      // n_run | n_def | n_act [26] each, n_gens, n_offsets: the header of a record, contiguous from rec::status on
  if (lists && !full) {
    constexpr size_t kHead = rec::yearly - rec::status;      // status, n_gens, n_offsets, n_chunks, n_run, n_def, n_act
    static_assert(rec::n_gens == rec::status + 4 && rec::n_offsets == rec::status + 8 && rec::n_run == rec::status + 16, "record header");
    cnt.resize(N * (kHead / 4));
    EG_HIP(hipMemcpy2D(cnt.data(), kHead, d_base + rec::status, rec::stride, kHead, N, hipMemcpyDeviceToHost));
    run = def = act = gens = offs = 0;
    for (size_t e = 0; e < N; ++e) {
      const int32_t* h = cnt.data() + e * (kHead / 4);
      size_t r = 0, d = 0, a = 0;
      for (int y = 0; y < EG_YEARS; ++y) { r += size_t(std::max(h[4 + y], 0)); d += size_t(std::max(h[4 + EG_YEARS + y], 0)); a += size_t(std::max(h[4 + 2 * EG_YEARS + y], 0)); }
      run = std::max(run, r); def = std::max(def, d); act = std::max(act, a);
      gens = std::max(gens, size_t(std::max(h[1], 0))); offs = std::max(offs, size_t(std::max(h[2], 0)));
    }
    run = std::min(run, size_t(EG_RUN_CAP)); def = std::min(def, size_t(EG_DEF_CAP)); act = std::min(act, size_t(EG_ACT_CAP));
    gens = std::min(gens, size_t(EG_MAX_GENS)); offs = std::min(offs, size_t(EG_MAX_OFFSETS));
  }
  EG_GET(n_run, EG_YEARS, int32_t); EG_GET(n_def, EG_YEARS, int32_t); EG_GET(n_act, EG_YEARS, int32_t);
  EG_GET_W(run_log, EG_RUN_CAP, uint8_t, run); EG_GET_W(def_log, EG_DEF_CAP, uint8_t, def); EG_GET_W(act_log, EG_ACT_CAP, uint8_t, act);
  EG_GET_W(gen_cell, EG_MAX_GENS, uint16_t, gens); EG_GET_W(gen_pack, EG_MAX_GENS, uint16_t, gens);
  EG_GET_W(off_pack, EG_MAX_OFFSETS, uint16_t, offs);
#undef EG_GET
#undef EG_GET_W
  return EG_OK;
}

namespace {
// an episode that ended with EG_EP_INTERNAL is a defect of the kernel's helper-wave protocol, not a property of the input
int check_internal(const int32_t* status, size_t n) {
  if (!status) return EG_OK;
  for (size_t i = 0; i < n; ++i)
    if (status[i] == EG_EP_INTERNAL) { set_error("k_rollout: helper-wave protocol timed out in episode " + std::to_string(i) + " (EG_EP_INTERNAL)"); return EG_ERR_INTERNAL; }
  return EG_OK;
}
}  // namespace

// row r of a caller's episode-major buffers
eg_episode_out eg::out_row(const eg_episode_out* o, size_t r) {
  eg_episode_out x = *o;
#define EG_ROW(field, count) if (x.field) x.field += r * size_t(count)
  EG_ROW(metrics, 4); EG_ROW(yearly, EG_YEARS * EG_YEARLY_FIELDS); EG_ROW(status, 1); EG_ROW(n_run, EG_YEARS); EG_ROW(n_def, EG_YEARS);
  EG_ROW(n_act, EG_YEARS); EG_ROW(run_log, EG_RUN_CAP); EG_ROW(def_log, EG_DEF_CAP); EG_ROW(act_log, EG_ACT_CAP); EG_ROW(n_gens, 1);
  EG_ROW(gen_cell, EG_MAX_GENS); EG_ROW(gen_pack, EG_MAX_GENS); EG_ROW(n_offsets, 1); EG_ROW(off_pack, EG_MAX_OFFSETS); EG_ROW(n_draws, 1);
  EG_ROW(bytes_moved, 1); EG_ROW(n_chunks, 1);
#undef EG_ROW
  return x;
}

// a context's or a group rank's best_result fold, on the current device: allocated on first use, best_result = None (multi_simulation.rs:384)
int eg::fold_reset(DevBuf<uint8_t>& d_fold) {
  EG_HIP(d_fold.reserve(kFoldBytes));
  EG_HIP(hipMemsetAsync(d_fold, 0, kFoldBytes, nullptr));
  return EG_OK;
}
// ... and its top-K archive: a fresh one of k entries (mode 1 / 2), stream-ordered behind everything enqueued before
int eg::topk_reset(DevBuf<uint8_t>& d_topk, int k, int mode) {
  static_assert(sizeof(TopKState) <= kTopKRecords, "top-k state layout");
  EG_HIP(d_topk.reserve(kTopKBytes));
  TopKState st{};
  st.k = k; st.mode = mode;
  EG_HIP(hipMemcpy(d_topk, &st, sizeof(st), hipMemcpyHostToDevice));
  return EG_OK;
}

int eg::fetch_topk_rows(const char* who, const TopKState& st, const std::function<const uint8_t*(int, const TopKEntry&)>& archive_of,
                        eg_episode_out* o, int32_t* n_held, double* scores, int64_t* global_index) {
  const std::string corrupt = std::string(who) + ": the archive's state is corrupt";
  if (st.n_held < 0 || st.n_held > st.k || st.k > EG_TOPK_MAX) { set_error(corrupt); return EG_ERR_INTERNAL; }
  *n_held = st.n_held;
  for (int i = 0; i < st.n_held; ++i) {
    const TopKEntry& e = st.e[i];
    if (e.slot < 0 || e.slot >= st.k) { set_error(corrupt); return EG_ERR_INTERNAL; }
    if (scores) scores[i] = e.score;
    if (global_index) global_index[i] = e.index;
    const uint8_t* archive = archive_of(i, e);
    if (!archive) return EG_ERR_INTERNAL;
    eg_episode_out row = out_row(o, size_t(i));
    EG_TRY(fetch_records(archive + kTopKRecords + size_t(e.slot) * rec::stride, 1, &row));
  }
  return EG_OK;
}

extern "C" {

uint32_t eg_last_batch_size(const eg_ctx* c) { return c ? c->last_n : 0u; }

int32_t eg_fetch(eg_ctx* c, eg_episode_out* o) {
  if (!c || !o) return EG_ERR_BAD_ARG;
  EG_TRY(eg_sync(c));
  if (c->last_n == 0) return EG_OK;
  EG_TRY(fetch_records(c->out.base, c->last_n, o));
  return check_internal(o->status, c->last_n);
}

int32_t eg_fetch_record(eg_ctx* c, uint32_t episode, eg_episode_out* o) {
  if (!c || !o || episode >= c->last_n) { set_error("eg_fetch_record: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_sync(c));
  EG_TRY(fetch_records(c->out.base + size_t(episode) * rec::stride, 1, o));
  return check_internal(o->status, 1);
}

int32_t eg_fetch_best_run(eg_ctx* c, eg_episode_out* o, int32_t* state) {
  if (!c || !o || !state || !c->snap_valid) { set_error("eg_fetch_best_run: push a policy first"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_sync(c));
  uint32_t word = 0;
  EG_HIP(hipMemcpy(&word, c->d_snap + snap::best_rec_state, sizeof(word), hipMemcpyDeviceToHost));
  *state = (int32_t)word;
  if (word != 1u) return EG_OK;
  return fetch_records(c->d_snap + snap::best_rec, 1, o);
}

int32_t eg_memory_report(const eg_ctx* c, uint64_t* table_bytes, uint64_t* record_bytes, uint64_t* field_pool_bytes) {
  if (!c) return EG_ERR_BAD_ARG;
  if (table_bytes) *table_bytes = uint64_t(tab::total);
  if (record_bytes) *record_bytes = uint64_t(c->d_out.count);
  if (field_pool_bytes) *field_pool_bytes = uint64_t(c->dev.heavy ? c->dev.heavy_slots : 0u) * uint64_t(kRadiusClasses) * 2624u * sizeof(double);
  return EG_OK;
}

int32_t eg_best_result_track(eg_ctx* c, int32_t mode) {
  if (!c || mode < 0 || mode > 2) { set_error("eg_best_result_track: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->group_member && mode != 0) { set_error("eg_best_result_track: the context is a rank of an eg_group (use eg_group_best_result_track)"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  if (mode != 0)
    EG_TRY(fold_reset(c->d_fold));
  c->fold_mode = mode;
  return EG_OK;
}

int32_t eg_fetch_best_result(eg_ctx* c, eg_episode_out* o, int32_t* state, int64_t* global_index) {
  if (!c || !o || !state) { set_error("eg_fetch_best_result: bad argument"); return EG_ERR_BAD_ARG; }
  if (!c->d_fold) { set_error("eg_fetch_best_result: eg_best_result_track first"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_sync(c));
  FoldState st{};
  EG_HIP(hipMemcpy(&st, c->d_fold, sizeof(st), hipMemcpyDeviceToHost));
  *state = st.has ? 1 : 0;
  if (global_index) *global_index = st.has ? int64_t(st.index) : -1;
  if (!st.has) return EG_OK;
  return fetch_records(c->d_fold + kFoldRecord, 1, o);
}

int32_t eg_top_k_track(eg_ctx* c, int32_t k, int32_t mode) {
  if (!c || mode < 0 || mode > 2 || (mode != 0 && (k < 1 || k > EG_TOPK_MAX))) { set_error("eg_top_k_track: bad argument (1 <= k <= EG_TOPK_MAX, mode 0..2)"); return EG_ERR_BAD_ARG; }
  if (c->group_member && mode != 0) { set_error("eg_top_k_track: the context is a rank of an eg_group (use eg_group_top_k_track)"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  if (mode != 0) {
    EG_TRY(topk_reset(c->d_topk, k, mode));
    c->topk_k = k;
  }
  c->topk_mode = mode;
  return EG_OK;
}

int32_t eg_fetch_top_k(eg_ctx* c, eg_episode_out* o, int32_t* n_held, double* scores, int64_t* global_index) {
  if (!c || !o || !n_held) { set_error("eg_fetch_top_k: bad argument"); return EG_ERR_BAD_ARG; }
  if (!c->d_topk) { set_error("eg_fetch_top_k: eg_top_k_track first"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_sync(c));
  TopKState st{};
  EG_HIP(hipMemcpy(&st, c->d_topk, sizeof(st), hipMemcpyDeviceToHost));
  return fetch_topk_rows("eg_fetch_top_k", st, [c](int, const TopKEntry&) -> const uint8_t* { return c->d_topk; }, o, n_held, scores, global_index);
}

int32_t eg_pareto_track(eg_ctx* c, int32_t cap, int32_t objectives, int32_t mode) {
  if (!c) { set_error("eg_pareto_track: bad argument (ctx)"); return EG_ERR_BAD_ARG; }
  if (cap < 0 || cap > EG_PARETO_MAX) { set_error("eg_pareto_track: cap " + std::to_string(cap) + " is outside 0..EG_PARETO_MAX (256)"); return EG_ERR_BAD_ARG; }
  if (cap == 0) { c->pareto_cap = 0; return EG_OK; }
  auto fail = [](const std::string& m) { set_error("eg_pareto_track: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(check_objectives(fail, objectives)); EG_TRY(check_mode(fail, mode));      // (eg_plan_host.cpp: the searches' archives word them alike)
  if (c->group_member) { set_error("eg_pareto_track: the context is a rank of an eg_group (the Pareto archive has no group form)"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  static_assert(sizeof(ParetoState) <= kParetoRecords, "pareto state layout");
  c->pareto_cap = 0;      // (until the new archive stands)
  EG_HIP(c->d_pareto.reserve(kParetoRecords + size_t(cap) * rec::stride));
  ParetoState st{};
  st.cap = cap; st.objectives = objectives; st.mode = pareto_rank_mode(mode); st.pad = pareto_keep_spread(mode) ? kParetoKeepSpread : 0;
  EG_HIP(hipMemcpy(c->d_pareto, &st, sizeof(st), hipMemcpyHostToDevice));
  c->pareto_spread = pareto_keep_spread(mode);
  c->pareto_cap = cap;
  return EG_OK;
}

int32_t eg_pareto_fold_last_batch(eg_ctx* c) {
  if (!c) { set_error("eg_pareto_fold_last_batch: bad argument (ctx)"); return EG_ERR_BAD_ARG; }
  if (c->pareto_cap == 0) { set_error("eg_pareto_fold_last_batch: eg_pareto_track first (tracking is off)"); return EG_ERR_BAD_ARG; }
  if (c->last_n == 0) { set_error("eg_pareto_fold_last_batch: there is no last batch"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  return pareto_fold(c, c->last_n, c->last_first);
}

int32_t eg_fetch_pareto(eg_ctx* c, eg_episode_out* o, int32_t* n_held, int64_t* global_index, double* scores, int64_t* n_dropped) {
  if (!c || !n_held) { set_error("eg_fetch_pareto: bad argument"); return EG_ERR_BAD_ARG; }
  if (!c->d_pareto) { set_error("eg_fetch_pareto: eg_pareto_track first"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_sync(c));
  std::vector<uint8_t> buf(sizeof(ParetoState));
  EG_HIP(hipMemcpy(buf.data(), c->d_pareto, sizeof(ParetoState), hipMemcpyDeviceToHost));
  const ParetoState& st = *reinterpret_cast<const ParetoState*>(buf.data());
  const char* corrupt = "eg_fetch_pareto: the archive's state is corrupt";
  if (st.cap < 1 || st.cap > EG_PARETO_MAX || st.n_held < 0 || st.n_held > st.cap) { set_error(corrupt); return EG_ERR_INTERNAL; }
  *n_held = st.n_held;
  if (n_dropped) *n_dropped = st.n_dropped;
  for (int i = 0; i < st.n_held; ++i) {
    const ParetoEntry& e = st.e[i];
    if (e.slot < 0 || e.slot >= st.cap) { set_error(corrupt); return EG_ERR_INTERNAL; }
    if (scores) scores[i] = e.score;
    if (global_index) global_index[i] = e.index;
    if (!o) continue;
    eg_episode_out row = out_row(o, size_t(i));
    EG_TRY(fetch_records(c->d_pareto + kParetoRecords + size_t(e.slot) * rec::stride, 1, &row));
  }
  return EG_OK;
}

double eg_rank_score(const double m[4], int32_t mode) { return m ? rm::rank_score(m, mode) : std::nan(""); }

int32_t eg_fetch_scores(eg_ctx* c, double* scores) {
  if (!c || !scores) return EG_ERR_BAD_ARG;
  EG_HIP(hipSetDevice(c->device));
  if (c->last_n) EG_HIP(hipMemcpy2D(scores, sizeof(double), c->out.base + rec::score, rec::stride, sizeof(double), c->last_n, hipMemcpyDeviceToHost));
  return EG_OK;
}

int32_t eg_fetch_episode_lists(eg_ctx* c, uint32_t i, double metrics[4], int32_t* n_run, uint8_t* run_log, int32_t* n_def,
                               uint8_t* def_log) {
  if (!c || i >= c->last_n || !metrics || !n_run || !run_log || !n_def || !def_log) { set_error("eg_fetch_episode_lists: bad argument"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_HIP(hipMemcpy(metrics, c->out.metrics(i), 4 * sizeof(double), hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(n_run, c->out.n_run(i), EG_YEARS * sizeof(int32_t), hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(n_def, c->out.n_def(i), EG_YEARS * sizeof(int32_t), hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(run_log, c->out.run_log(i), EG_RUN_CAP, hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(def_log, c->out.def_log(i), EG_DEF_CAP, hipMemcpyDeviceToHost));
  return EG_OK;
}

}  // extern "C"
