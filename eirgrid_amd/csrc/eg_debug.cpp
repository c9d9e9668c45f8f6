// eg_debug.cpp — the crafted-batch test hooks (include/eirgrid_hip.h, debug section): a batch of synthetic records in the context's
// record buffer, and the reductions that decide what a run keeps run over it — the folds launch_batch runs behind a real batch (through the
// helpers it calls), k_pick_best, k_refine_pick_many, k_plan_constraints over crafted yearly rows, k_repair_pick_many behind it — and a crafted generation of eg_breed_plans / eg_explore_plans: tagged plan blocks
// folded into the private archive, gathered and turned over — through the archive functions the entry points run (eg_plan_host.cpp).
// Host code only: no kernel is launched here that a run does not launch — but for eg_debug_tiles_refresh, whose one-wave kernel exists to
// call a device function of the replay kernels (eg_field.h tiles_refresh) on a crafted list and field.
#include <cstring>

#include "eg_host.h"

using namespace eg;

namespace {
int refuse_rank(const eg_ctx* c, const char* who) {
  if (!c->group_member) return EG_OK;
  set_error(std::string(who) + ": the context is a rank of an eg_group (the test hooks have no group form)");
  return EG_ERR_BAD_ARG;
}
// one field of the n records from a host array of `width` bytes per record
int put_field(eg_ctx* c, size_t field, const void* src, size_t width, uint32_t n) {
  EG_HIP(hipMemcpy2D(c->out.base + field, rec::stride, src, width, width, n, hipMemcpyHostToDevice));
  return EG_OK;
}
// k_refine_pick_many over the last batch, cut into n_segs segments that tile it (checked by the callers): tagged plan blocks, edits and
// base blocks as include/eirgrid_hip.h documents them, segment s on base slot s; the entries and the base blocks as the kernel left them.
// repair_weights: k_repair_pick_many in its place, over what k_plan_constraints left for the batch (c->feas_k constraints), with these
// c->feas_k weights, which go up behind the segment table
int refine_pick(eg_ctx* c, int32_t mode, const uint32_t* seg_first, const uint32_t* seg_count, int32_t n_segs, void* entries, uint8_t* base_blocks,
                const double* repair_weights = nullptr) {
  static_assert(sizeof(RefineEntry) == EG_DEBUG_REFINE_ENTRY_BYTES, "the step entry's layout is what the hooks document");
  static_assert(sizeof(RepairEntry) == EG_DEBUG_REPAIR_ENTRY_BYTES, "the repair entry's layout is what the hooks document");
  static_assert(EG_PLAN_BLOCK_BYTES == snap::kPlanStride, "plan block");
  const uint32_t n = c->last_n;
  EG_HIP(hipSetDevice(c->device));
  constexpr size_t kWords = snap::kPlanStride / 4, kOff26 = (snap::best_off - snap::best_mask) / 4 + EG_YEARS, kOffD26 = (snap::bestd_off - snap::best_mask) / 4 + EG_YEARS;
  static_assert(kOff26 == 130 && kOffD26 == 158, "the words of the list totals as the hooks document them");
  const size_t S = size_t(n_segs);
  std::vector<uint32_t> blocks(size_t(n) * kWords), base(S * kWords), in(size_t(n) * 2 + S * 4 + (repair_weights ? 2 * size_t(c->feas_k) : 0));      // in: the packed edits, the segment table, the weights
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t* b = blocks.data() + size_t(j) * kWords;
    for (size_t w = 0; w < kWords; ++w) b[w] = j * 0x9E3779B1u + uint32_t(w);
    b[kOff26] = j % (uint32_t(snap::kBestCap) + 1u); b[kOffD26] = (j / 3u) % (uint32_t(snap::kBestCap) + 1u);
    in[2 * size_t(j)] = j; in[2 * size_t(j) + 1] = ~j;
  }
  for (size_t s = 0; s < S; ++s) {
    uint32_t* b = base.data() + s * kWords;
    for (size_t w = 0; w < kWords; ++w) b[w] = 0xBA5E0000u + (uint32_t(s) << 8) + uint32_t(w);
    b[kOff26] = 7u; b[kOffD26] = 5u;
    uint32_t* t = in.data() + size_t(n) * 2 + s * 4;
    t[0] = seg_first[s]; t[1] = seg_count[s]; t[2] = uint32_t(s); t[3] = 0u;
  }
  static_assert(kRefineSegmentBytes == 16, "segment table entry");
  const size_t at_weights = (size_t(n) * 2 + S * 4) * 4;      // (a multiple of 8)
  if (repair_weights) std::memcpy(in.data() + size_t(n) * 2 + S * 4, repair_weights, sizeof(double) * size_t(c->feas_k));
  EG_HIP(c->d_plans.reserve(size_t(n) * snap::kPlanStride));
  EG_HIP(c->d_refine_bases.reserve(S * snap::kPlanStride));
  EG_HIP(c->d_refine_in.reserve(in.size() * 4));
  EG_HIP(c->d_refine_log.reserve(size_t(kRefineLog) * kRefineEntryStride));
  EG_HIP(hipMemcpy(c->d_plans, blocks.data(), blocks.size() * 4, hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(c->d_refine_bases, base.data(), base.size() * 4, hipMemcpyHostToDevice));
  EG_HIP(hipMemcpy(c->d_refine_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  EG_HIP(hipMemsetAsync(c->d_refine_log, 0, S * kRefineEntryStride, nullptr));
  c->n_plan_blocks = n;
  if (repair_weights)
    EG_LAUNCH("k_repair_pick_many", launch_repair_pick_many(c->out, c->d_refine_in + size_t(n) * 8, uint32_t(n_segs), n, mode, c->d_refine_in, c->d_plans, c->d_refine_bases,
                                                            uint32_t(n_segs), c->d_violated, c->d_excess, uint32_t(c->feas_k),
                                                            reinterpret_cast<const double*>(c->d_refine_in + at_weights), c->d_refine_log, nullptr));
  else
    EG_LAUNCH("k_refine_pick_many", launch_refine_pick_many(c->out, c->d_refine_in + size_t(n) * 8, uint32_t(n_segs), n, mode, c->d_refine_in, c->d_plans, c->d_refine_bases,
                                                            uint32_t(n_segs), c->d_refine_log, nullptr));
  static_assert(sizeof(RefineEntry) == sizeof(RepairEntry), "either entry is read back at the same width");
  EG_HIP(hipMemcpy2D(entries, sizeof(RefineEntry), c->d_refine_log, kRefineEntryStride, sizeof(RefineEntry), S, hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(base_blocks, c->d_refine_bases, S * snap::kPlanStride, hipMemcpyDeviceToHost));
  return EG_OK;
}
}  // namespace

extern "C" {

int32_t eg_debug_load_batch(eg_ctx* c, const double* metrics, const int32_t* status, const int32_t* n_act, const uint8_t* act_log, const double* score_list,
                            uint32_t n, uint64_t first_index) {
  if (!c || !metrics || !status || n == 0) { set_error("eg_debug_load_batch: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_load_batch"));
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_outputs(c, n));
  EG_HIP(hipMemsetAsync(c->out.base, 0, size_t(n) * rec::stride, nullptr));
  EG_HIP(hipMemsetAsync(c->out.score_list, 0, size_t(n) * sizeof(double), nullptr));
  // the tag and the two lists that show where a copied record or candidate came from: the global index g, its eight bytes, those of ~g
  std::vector<uint64_t> tag(n), inv(n);
  std::vector<int32_t> eight(size_t(n) * EG_YEARS, 0);
  for (uint32_t e = 0; e < n; ++e) { tag[e] = first_index + e; inv[e] = ~tag[e]; eight[size_t(e) * EG_YEARS] = EG_DEBUG_LIST_LEN; }
  static_assert(EG_DEBUG_LIST_LEN == sizeof(uint64_t), "the lists are the index's bytes (little-endian)");
  EG_TRY(put_field(c, rec::metrics, metrics, 4 * sizeof(double), n));
  EG_TRY(put_field(c, rec::status, status, sizeof(int32_t), n));
  EG_TRY(put_field(c, rec::n_draws, tag.data(), sizeof(uint64_t), n));
  EG_TRY(put_field(c, rec::n_run, eight.data(), EG_YEARS * sizeof(int32_t), n));
  EG_TRY(put_field(c, rec::n_def, eight.data(), EG_YEARS * sizeof(int32_t), n));
  EG_TRY(put_field(c, rec::run_log, tag.data(), sizeof(uint64_t), n));
  EG_TRY(put_field(c, rec::def_log, inv.data(), sizeof(uint64_t), n));
  if (n_act) EG_TRY(put_field(c, rec::n_act, n_act, EG_YEARS * sizeof(int32_t), n));
  if (act_log) EG_TRY(put_field(c, rec::act_log, act_log, EG_ACT_CAP, n));      // the whole row: also what lies behind the log
  if (score_list) EG_HIP(hipMemcpy(c->out.score_list, score_list, size_t(n) * sizeof(double), hipMemcpyHostToDevice));
  c->last_n = n; c->last_first = first_index; c->feas_k = 0; c->ran = {};
  return EG_OK;
}

// ---- plan constraints over a crafted batch: the rows, then the launch a plan batch ends with (eg_constraints.cpp constrain_batch) ------
int32_t eg_debug_load_yearly(eg_ctx* c, const double* yearly, uint32_t n) {
  if (!c || !yearly) { set_error("eg_debug_load_yearly: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_load_yearly"));
  if (n == 0 || n != c->last_n) { set_error("eg_debug_load_yearly: n = " + std::to_string(n) + ", the last batch holds " + std::to_string(c->last_n) + " records"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  return put_field(c, rec::yearly, yearly, sizeof(double) * EG_YEARS * EG_YEARLY_FIELDS, n);
}

int32_t eg_debug_load_built(eg_ctx* c, const int32_t* n_gens, const uint16_t* gen_pack, const int32_t* n_offsets, const uint16_t* off_pack, uint32_t n) {
  if (!c || !n_gens || !gen_pack || !n_offsets || !off_pack) { set_error("eg_debug_load_built: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_load_built"));
  if (n == 0 || n != c->last_n) { set_error("eg_debug_load_built: n = " + std::to_string(n) + ", the last batch holds " + std::to_string(c->last_n) + " records"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(put_field(c, rec::n_gens, n_gens, sizeof(int32_t), n));
  EG_TRY(put_field(c, rec::n_offsets, n_offsets, sizeof(int32_t), n));
  EG_TRY(put_field(c, rec::gen_pack, gen_pack, sizeof(uint16_t) * EG_MAX_GENS, n));      // the whole rows: also what lies behind the counts
  return put_field(c, rec::off_pack, off_pack, sizeof(uint16_t) * EG_MAX_OFFSETS, n);
}

int32_t eg_debug_constrain_last_batch(eg_ctx* c) {
  if (!c) { set_error("eg_debug_constrain_last_batch: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_constrain_last_batch"));
  if (c->last_n == 0) { set_error("eg_debug_constrain_last_batch: there is no last batch"); return EG_ERR_BAD_ARG; }
  if (c->rows.n + c->builds.n == 0) { set_error("eg_debug_constrain_last_batch: eg_plan_constraints_set first (no constraints are set)"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  return constrain_batch(c, c->last_n);
}

// ---- plan streams over crafted records: the two launches a batch under streams puts behind its passes (eg_streams.cpp) ------
int32_t eg_debug_ensemble_keep(eg_ctx* c, int32_t r) {
  if (!c) { set_error("eg_debug_ensemble_keep: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_ensemble_keep"));
  if (c->last_n == 0) { set_error("eg_debug_ensemble_keep: there is no last batch"); return EG_ERR_BAD_ARG; }
  if (r < 0 || r >= EG_STREAMS_MAX) { set_error("eg_debug_ensemble_keep: r = " + std::to_string(r) + " (a stream 0.." + std::to_string(EG_STREAMS_MAX - 1) + ")"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  return ensemble_keep(c, c->last_n, r, EG_STREAMS_MAX);
}

int32_t eg_debug_ensemble_commit(eg_ctx* c, int32_t n_streams, int32_t tail, int32_t mode) {
  auto fail = [](const std::string& m) { set_error("eg_debug_ensemble_commit: " + m); return EG_ERR_BAD_ARG; };
  if (!c) return fail("bad argument");
  EG_TRY(refuse_rank(c, "eg_debug_ensemble_commit"));
  if (c->last_n == 0) return fail("there is no last batch");
  if (n_streams < 1 || n_streams > EG_STREAMS_MAX) return fail("n_streams = " + std::to_string(n_streams) + " (1.." + std::to_string(EG_STREAMS_MAX) + ")");
  if (tail < 1 || tail > n_streams) return fail("tail = " + std::to_string(tail) + " (1..n_streams = " + std::to_string(n_streams) + ")");
  if (mode != 1 && mode != 2) return fail("mode " + std::to_string(mode) + " is neither 1 (optimization_mode None) nor 2 (cost_only)");
  const uint64_t want = n_streams == 64 ? ~0ull : (1ull << n_streams) - 1ull;
  if (c->ens_kept_n != c->last_n || (c->ens_kept_mask & want) != want)
    return fail("eg_debug_ensemble_keep first (the store does not hold slabs 0.." + std::to_string(n_streams - 1) + " of a batch of " + std::to_string(c->last_n) + " records)");
  EG_HIP(hipSetDevice(c->device));
  return ensemble_commit(c, c->last_n, n_streams, tail, mode);
}

int32_t eg_debug_fold_last_batch(eg_ctx* c, int32_t what, int32_t use_score_list) {
  if (!c || what < 1 || what > (EG_DEBUG_FOLD_BEST_RESULT | EG_DEBUG_FOLD_TOP_K)) { set_error("eg_debug_fold_last_batch: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_fold_last_batch"));
  if (c->last_n == 0) { set_error("eg_debug_fold_last_batch: there is no last batch"); return EG_ERR_BAD_ARG; }
  if ((what & EG_DEBUG_FOLD_BEST_RESULT) && c->fold_mode == 0) { set_error("eg_debug_fold_last_batch: eg_best_result_track first (tracking is off)"); return EG_ERR_BAD_ARG; }
  if ((what & EG_DEBUG_FOLD_TOP_K) && c->topk_mode == 0) { set_error("eg_debug_fold_last_batch: eg_top_k_track first (tracking is off)"); return EG_ERR_BAD_ARG; }
  if ((what & EG_DEBUG_FOLD_TOP_K) && use_score_list && c->topk_mode != 1) {
    set_error("eg_debug_fold_last_batch: use_score_list with top-K mode 2 (the score list holds mode 1's scores)"); return EG_ERR_BAD_ARG;
  }
  EG_HIP(hipSetDevice(c->device));
  if (what & EG_DEBUG_FOLD_BEST_RESULT) EG_TRY(best_result_fold(c, c->last_n, c->last_first));
  if (what & EG_DEBUG_FOLD_TOP_K) EG_TRY(topk_fold(c, c->last_n, c->last_first, use_score_list != 0));
  return EG_OK;
}

int32_t eg_debug_pareto_fold(eg_ctx* c, const double* metrics, const int32_t* status, uint32_t n, uint64_t first_index) {
  if (!c || !metrics || !status || n == 0) { set_error("eg_debug_pareto_fold: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->pareto_cap == 0) { set_error("eg_debug_pareto_fold: eg_pareto_track first (tracking is off)"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_debug_load_batch(c, metrics, status, nullptr, nullptr, nullptr, n, first_index));
  return pareto_fold(c, n, first_index);
}

int32_t eg_debug_pick_best(eg_ctx* c, void* candidate) {
  if (!c || !candidate) { set_error("eg_debug_pick_best: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_pick_best"));
  if (c->last_n == 0) { set_error("eg_debug_pick_best: there is no last batch"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  EG_TRY(ensure_packet(c));
  UpdateCandidate* d_cand = reinterpret_cast<UpdateCandidate*>(c->d_packet.ptr + 8 * EG_STATS_LEN);
  EG_HIP(hipMemsetAsync(d_cand, 0, sizeof(UpdateCandidate), nullptr));      // (what the kernel leaves alone without a winner reads as zeros)
  EG_LAUNCH("k_pick_best", launch_pick_best(c->out, c->last_n, c->last_first, d_cand, nullptr));
  EG_HIP(hipMemcpy(candidate, d_cand, sizeof(UpdateCandidate), hipMemcpyDeviceToHost));
  return EG_OK;
}

int32_t eg_debug_refine_pick(eg_ctx* c, int32_t mode, void* entry, uint8_t* base_block) {
  if (!c || !entry || !base_block || (mode != 1 && mode != 2)) { set_error("eg_debug_refine_pick: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_refine_pick"));
  const uint32_t first = 0, n = c->last_n;
  if (n == 0 || n > EG_REFINE_MAX_VARIANTS) { set_error("eg_debug_refine_pick: the last batch holds " + std::to_string(n) + " records (1..EG_REFINE_MAX_VARIANTS)"); return EG_ERR_BAD_ARG; }
  return refine_pick(c, mode, &first, &n, 1, entry, base_block);      // one segment, base slot 0: its tags are 0xBA5E0000 + w
}

int32_t eg_debug_refine_pick_many(eg_ctx* c, int32_t mode, const uint32_t* seg_first, const uint32_t* seg_count, int32_t n_segs, void* entries, uint8_t* base_blocks) {
  if (!c || !seg_first || !seg_count || !entries || !base_blocks || (mode != 1 && mode != 2)) { set_error("eg_debug_refine_pick_many: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_refine_pick_many"));
  const uint32_t n = c->last_n;
  if (n == 0 || n > EG_REFINE_MAX_VARIANTS) { set_error("eg_debug_refine_pick_many: the last batch holds " + std::to_string(n) + " records (1..EG_REFINE_MAX_VARIANTS)"); return EG_ERR_BAD_ARG; }
  if (n_segs < 1 || n_segs > EG_REFINE_MAX_PLANS) { set_error("eg_debug_refine_pick_many: n_segs = " + std::to_string(n_segs) + " (1..EG_REFINE_MAX_PLANS)"); return EG_ERR_BAD_ARG; }
  {
    uint64_t at = 0;
    for (int32_t s = 0; s < n_segs; ++s) {
      if (seg_first[s] != at || seg_count[s] == 0) { set_error("eg_debug_refine_pick_many: segment " + std::to_string(s) + " does not continue the tiling of the last batch"); return EG_ERR_BAD_ARG; }
      at += seg_count[s];
    }
    if (at != n) { set_error("eg_debug_refine_pick_many: the segments cover " + std::to_string(at) + " of the last batch's " + std::to_string(n) + " records"); return EG_ERR_BAD_ARG; }
  }
  return refine_pick(c, mode, seg_first, seg_count, n_segs, entries, base_blocks);
}

int32_t eg_debug_repair_pick_many(eg_ctx* c, int32_t mode, const double* weights, const uint32_t* seg_first, const uint32_t* seg_count, int32_t n_segs, void* entries,
                                  uint8_t* base_blocks) {
  const char* fn = "eg_debug_repair_pick_many";
  auto fail = [fn](const std::string& m) { set_error(std::string(fn) + ": " + m); return EG_ERR_BAD_ARG; };
  if (!c || !seg_first || !seg_count || !entries || !base_blocks || (mode != 1 && mode != 2)) return fail("bad argument");
  EG_TRY(refuse_rank(c, fn));
  const uint32_t n = c->last_n;
  if (n == 0 || n > EG_REFINE_MAX_VARIANTS) return fail("the last batch holds " + std::to_string(n) + " records (1..EG_REFINE_MAX_VARIANTS)");
  if (c->feas_k == 0) return fail("the last batch was not judged (eg_debug_constrain_last_batch first: the pick reads its masks and excess rows)");
  if (n_segs < 1 || n_segs > EG_REFINE_MAX_PLANS) return fail("n_segs = " + std::to_string(n_segs) + " (1..EG_REFINE_MAX_PLANS)");
  EG_TRY(check_repair_weights(fail, weights, c->feas_k));
  uint64_t at = 0;
  for (int32_t s = 0; s < n_segs; ++s) {
    if (seg_first[s] != at || seg_count[s] == 0) return fail("segment " + std::to_string(s) + " does not continue the tiling of the last batch");
    at += seg_count[s];
  }
  if (at != n) return fail("the segments cover " + std::to_string(at) + " of the last batch's " + std::to_string(n) + " records");
  const std::vector<double> w = weights ? std::vector<double>(weights, weights + c->feas_k) : std::vector<double>(size_t(c->feas_k), 1.0);
  return refine_pick(c, mode, seg_first, seg_count, n_segs, entries, base_blocks, w.data());
}

// ---- the lazy field's catch-up for one pair of tiles: a crafted list and a crafted class field, one wave (k_debug_tiles_refresh: the hook's own kernel
//      around the device function the searches call) ------
int32_t eg_debug_tiles_refresh(eg_ctx* c, const uint16_t* cells, int32_t n_cells, int32_t radius_class, int32_t tile_a, int32_t tile_b, double* field, int32_t* folded) {
  if (!c || !field || !folded || (n_cells > 0 && !cells)) { set_error("eg_debug_tiles_refresh: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_tiles_refresh"));
  auto fail = [](const std::string& m) { set_error("eg_debug_tiles_refresh: " + m); return EG_ERR_BAD_ARG; };
  if (n_cells < 0 || n_cells > EG_MAX_GENS) return fail("n_cells = " + std::to_string(n_cells) + " (0..EG_MAX_GENS)");
  for (int32_t i = 0; i < n_cells; ++i) if (cells[i] >= kCells) return fail("cells[" + std::to_string(i) + "] = " + std::to_string(cells[i]) + " is not a grid cell");
  if (tile_a < 0 || tile_a >= kTiles || tile_b < -1 || tile_b >= kTiles || tile_b == tile_a) return fail("tiles " + std::to_string(tile_a) + ", " + std::to_string(tile_b) + " (0..48, distinct; tile_b -1: none)");
  bool has_class = false;
  for (int t = 0; t < kTypes; ++t) has_class = has_class || c->tables.H.rclass[t] == radius_class;
  if (radius_class < 0 || radius_class >= kRadiusClasses || !has_class) return fail("radius_class " + std::to_string(radius_class) + " is no generator type's");
  EG_HIP(hipSetDevice(c->device));
  DevBuf<double> d_field; DevBuf<uint16_t> d_cells; DevBuf<int> d_out;
  EG_HIP(d_field.reserve(EG_DEBUG_FIELD_DOUBLES)); EG_HIP(d_cells.reserve(size_t(EG_MAX_GENS))); EG_HIP(d_out.reserve(1));
  EG_HIP(hipMemcpy(d_field, field, sizeof(double) * EG_DEBUG_FIELD_DOUBLES, hipMemcpyHostToDevice));
  if (n_cells > 0) EG_HIP(hipMemcpy(d_cells, cells, sizeof(uint16_t) * size_t(n_cells), hipMemcpyHostToDevice));
  EG_LAUNCH("k_debug_tiles_refresh", launch_debug_tiles_refresh(c->dev, d_field, d_cells, n_cells, radius_class, tile_a, tile_b, d_out, nullptr));
  // (synchronous copies on the null stream: they wait for the kernel)
  int out = 0;
  EG_HIP(hipMemcpy(&out, d_out, sizeof(int), hipMemcpyDeviceToHost));
  EG_HIP(hipMemcpy(field, d_field, sizeof(double) * EG_DEBUG_FIELD_DOUBLES, hipMemcpyDeviceToHost));
  if (out < 0) return fail("the device found no generator type of radius class " + std::to_string(radius_class));
  *folded = out;
  return EG_OK;
}

// ---- a crafted generation of eg_breed_plans / eg_explore_plans: the private archive, k_breed_gather and the two turnover kernels ------
static_assert(sizeof(ParetoEntry) == EG_DEBUG_PARETO_ENTRY_BYTES && sizeof(ParetoState) == EG_DEBUG_PARETO_STATE_BYTES && offsetof(ParetoState, e) == 32,
              "the archive's state is what the hooks document");
static_assert(kBreedHeaderBytes == EG_DEBUG_BREED_HEADER_BYTES && kBreedRowBytes == EG_DEBUG_BREED_ROW_BYTES &&
              breed_at::kReadbackBytes == EG_DEBUG_BREED_READBACK_BYTES && snap::best_off - snap::best_mask == EG_DEBUG_BREED_BLOCK_OFFSETS &&
              sizeof(BreedCounters) == 16, "the readback buffer is what the hooks document");

int32_t eg_debug_breed_begin(eg_ctx* c, int32_t cap, int32_t objectives, int32_t mode) {
  if (!c) { set_error("eg_debug_breed_begin: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_breed_begin"));
  auto fail = [](const std::string& m) { set_error("eg_debug_breed_begin: " + m); return EG_ERR_BAD_ARG; };
  EG_TRY(check_cap(fail, cap)); EG_TRY(check_objectives(fail, objectives)); EG_TRY(check_mode(fail, mode));
  EG_HIP(hipSetDevice(c->device));
  c->debug_breed = false;
  static_assert(breed_at::records < breed_at::blocks && breed_at::blocks < breed_at::parents && breed_at::parents < breed_at::readback &&
                breed_at::readback + breed_at::kReadbackBytes == breed_at::counters, "the canary fills what lies between the state and the counters");
  EG_TRY(archive_begin(c, cap, objectives, mode, [c] {
    EG_HIP(hipMemset(c->d_breed + breed_at::records, EG_DEBUG_BREED_CANARY, breed_at::counters - breed_at::records));
    return EG_OK;
  }));
  c->debug_breed = true;
  return EG_OK;
}

int32_t eg_debug_breed_chunk(eg_ctx* c, const double* metrics, const int32_t* status, uint32_t n, uint64_t first_index) {
  if (!c || !metrics || !status) { set_error("eg_debug_breed_chunk: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_breed_chunk"));
  if (!c->debug_breed) { set_error("eg_debug_breed_chunk: eg_debug_breed_begin first"); return EG_ERR_BAD_ARG; }
  if (n == 0 || n > EG_CROSS_MAX_VARIANTS) { set_error("eg_debug_breed_chunk: n = " + std::to_string(n) + " (1..EG_CROSS_MAX_VARIANTS)"); return EG_ERR_BAD_ARG; }
  if (first_index > uint64_t(INT64_MAX) - n) { set_error("eg_debug_breed_chunk: first_index + n passes 2^63 (an entry's index is an int64)"); return EG_ERR_BAD_ARG; }
  EG_TRY(eg_debug_load_batch(c, metrics, status, nullptr, nullptr, nullptr, n, first_index));
  constexpr size_t kWords = snap::kPlanStride / 4;
  std::vector<uint32_t> blocks(size_t(n) * kWords);
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t h = uint32_t(((first_index + j) * EG_DEBUG_BREED_TAG_MUL) >> 32);
    uint32_t* b = blocks.data() + size_t(j) * kWords;
    for (size_t w = 0; w < kWords; ++w) b[w] = h + uint32_t(w);
  }
  EG_HIP(c->d_plans.reserve(size_t(n) * snap::kPlanStride));
  // (a synchronous copy on the null stream: it waits for the previous chunk's gather, which read what it overwrites)
  EG_HIP(hipMemcpy(c->d_plans, blocks.data(), blocks.size() * 4, hipMemcpyHostToDevice));
  c->n_plan_blocks = n;
  return archive_fold(c, n, first_index);
}

int32_t eg_debug_breed_turnover(eg_ctx* c, int32_t kind, int32_t next, int64_t m_first) {
  if (!c) { set_error("eg_debug_breed_turnover: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_breed_turnover"));
  if (!c->debug_breed) { set_error("eg_debug_breed_turnover: eg_debug_breed_begin first"); return EG_ERR_BAD_ARG; }
  if (kind != EG_DEBUG_TURNOVER_BREED && kind != EG_DEBUG_TURNOVER_EXPLORE) { set_error("eg_debug_breed_turnover: kind " + std::to_string(kind) + " is neither EG_DEBUG_TURNOVER_BREED nor EG_DEBUG_TURNOVER_EXPLORE"); return EG_ERR_BAD_ARG; }
  if (next != 0 && next != 1) { set_error("eg_debug_breed_turnover: next = " + std::to_string(next) + " (array 0 | 1)"); return EG_ERR_BAD_ARG; }
  if (kind == EG_DEBUG_TURNOVER_EXPLORE && m_first < 0) { set_error("eg_debug_breed_turnover: m_first = " + std::to_string(m_first) + " (a variant number)"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  if (kind == EG_DEBUG_TURNOVER_BREED) EG_LAUNCH("k_breed_turnover", launch_breed_turnover(c->d_breed, next, nullptr));
  else EG_LAUNCH("k_explore_turnover", launch_explore_turnover(c->d_breed, next, (long long)m_first, nullptr));
  return EG_OK;
}

int32_t eg_debug_breed_fetch(eg_ctx* c, void* state, uint8_t* blocks, uint8_t* array0, uint8_t* array1, uint8_t* readback, void* counters, uint64_t* tags) {
  if (!c) { set_error("eg_debug_breed_fetch: bad argument"); return EG_ERR_BAD_ARG; }
  EG_TRY(refuse_rank(c, "eg_debug_breed_fetch"));
  if (!c->debug_breed) { set_error("eg_debug_breed_fetch: eg_debug_breed_begin first"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  // (synchronous copies on the null stream: they wait for whatever the hooks have launched)
  if (state) EG_HIP(hipMemcpy(state, c->d_breed, sizeof(ParetoState), hipMemcpyDeviceToHost));
  if (blocks) EG_HIP(hipMemcpy(blocks, c->d_breed + breed_at::blocks, breed_at::kParentArray, hipMemcpyDeviceToHost));
  if (array0) EG_HIP(hipMemcpy(array0, c->d_breed + breed_at::parents, breed_at::kParentArray, hipMemcpyDeviceToHost));
  if (array1) EG_HIP(hipMemcpy(array1, c->d_breed + breed_at::parents + breed_at::kParentArray, breed_at::kParentArray, hipMemcpyDeviceToHost));
  if (readback) EG_HIP(hipMemcpy(readback, c->d_breed + breed_at::readback, breed_at::kReadbackBytes, hipMemcpyDeviceToHost));
  if (counters) EG_HIP(hipMemcpy(counters, c->d_breed + breed_at::counters, sizeof(BreedCounters), hipMemcpyDeviceToHost));
  if (tags) EG_HIP(hipMemcpy2D(tags, sizeof(uint64_t), c->d_breed + breed_at::records + rec::n_draws, rec::stride, sizeof(uint64_t), EG_PARETO_MAX, hipMemcpyDeviceToHost));
  return EG_OK;
}

}  // extern "C"
