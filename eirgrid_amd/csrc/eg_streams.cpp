// eg_streams.cpp — plan streams (include/eirgrid_hip.h eg_plan_streams_set): the setting of a context, the two launches eg_plans.cpp
// launch_plans puts behind the passes of a batch (ensemble_keep, ensemble_commit), what the last batch ran under and the two fetches.
// The kernels are eg_ensemble.h's; the crafted-batch hooks that drive them alone are eg_debug.cpp's.
#include <cstring>

#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_ensemble_row) == 128 && offsetof(eg_ensemble_row, committed) == 32 && offsetof(eg_ensemble_row, score_min) == 64 &&
                  offsetof(eg_ensemble_row, n_ok) == 88 && offsetof(eg_ensemble_row, status) == 104 && offsetof(eg_ensemble_row, pad) == 108,
              "eg_ensemble_row is part of the C ABI and what k_ensemble_commit stores");
static_assert(kEnsembleKeptBytes == 4 * sizeof(double) + 2 * sizeof(int32_t), "a kept entry: metrics[4], status, a zero word");

namespace {
int32_t validate(const char* who, int32_t n_streams, int32_t tail, int32_t mode) {
  auto fail = [who](const std::string& m) { set_error(std::string(who) + ": " + m); return EG_ERR_BAD_ARG; };
  if (n_streams < 0 || n_streams > EG_STREAMS_MAX) return fail("n_streams = " + std::to_string(n_streams) + " (0.." + std::to_string(EG_STREAMS_MAX) + "; 0 or 1 clears)");
  if (n_streams < 2) return EG_OK;
  if (tail < 1 || tail > n_streams) return fail("tail = " + std::to_string(tail) + " (1..n_streams = " + std::to_string(n_streams) + ")");
  if (mode != 1 && mode != 2) return fail("mode " + std::to_string(mode) + " is neither 1 (optimization_mode None) nor 2 (cost_only)");
  return EG_OK;
}
int no_streams(const char* who) { set_error(std::string(who) + ": the last batch ran without plan streams"); return EG_ERR_BAD_ARG; }
}  // namespace

int eg::ensemble_keep(eg_ctx* c, uint32_t n, int r, int slabs) {
  bool fresh = false;
  EG_HIP(c->d_ens_kept.reserve(size_t(slabs) * n * kEnsembleKeptBytes, &fresh));
  if (fresh || c->ens_kept_n != n) { c->ens_kept_n = n; c->ens_kept_mask = 0; }      // (a slab's place depends on n: another n lays the store out anew)
  c->ens_kept_mask |= 1ull << r;
  EG_LAUNCH("k_ensemble_keep", launch_ensemble_keep(c->out, n, c->d_ens_kept + size_t(r) * n * kEnsembleKeptBytes, nullptr));
  return EG_OK;
}

int eg::ensemble_commit(eg_ctx* c, uint32_t n, int R, int tail, int mode) {
  EG_HIP(c->d_ens_rows.reserve(n));
  EG_LAUNCH("k_ensemble_commit", launch_ensemble_commit(c->out, n, c->d_ens_kept, uint32_t(R), uint32_t(tail), mode, c->d_ens_rows, nullptr));
  c->ran.n = R; c->ran.tail = tail; c->ran.mode = mode;
  return EG_OK;
}

extern "C" {

int32_t eg_plan_streams_validate(int32_t n_streams, int32_t tail, int32_t mode) { return validate("eg_plan_streams_validate", n_streams, tail, mode); }

int32_t eg_plan_streams_set(eg_ctx* c, int32_t n_streams, int32_t tail, int32_t mode) {
  if (!c) { set_error("eg_plan_streams_set: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->group_member) { set_error("eg_plan_streams_set: the context is a rank of an eg_group (plan batches on a group are not supported)"); return EG_ERR_BAD_ARG; }
  EG_TRY(validate("eg_plan_streams_set", n_streams, tail, mode));
  if (n_streams < 2) c->streams = {};
  else { c->streams.n = n_streams; c->streams.tail = tail; c->streams.mode = mode; }
  return EG_OK;
}

int32_t eg_last_batch_streams(const eg_ctx* c, int32_t* tail, int32_t* mode) {
  if (!c) { set_error("eg_last_batch_streams: bad argument"); return EG_ERR_BAD_ARG; }
  const bool ran = c->last_n > 0 && c->ran.n > 0;
  if (tail) *tail = ran ? c->ran.tail : 0;
  if (mode) *mode = ran ? c->ran.mode : 0;
  return ran ? c->ran.n : 0;
}

int32_t eg_fetch_plan_ensemble(eg_ctx* c, eg_ensemble_row* rows) {
  if (!c || !rows) { set_error("eg_fetch_plan_ensemble: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->ran.n == 0 || c->last_n == 0) return no_streams("eg_fetch_plan_ensemble");
  EG_HIP(hipSetDevice(c->device));
  // (a synchronous copy on the null stream: it waits for the kernel)
  EG_HIP(hipMemcpy(rows, c->d_ens_rows, sizeof(eg_ensemble_row) * c->last_n, hipMemcpyDeviceToHost));
  return EG_OK;
}

int32_t eg_fetch_plan_streams(eg_ctx* c, double* metrics, int32_t* status) {
  if (!c) { set_error("eg_fetch_plan_streams: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->ran.n == 0 || c->last_n == 0) return no_streams("eg_fetch_plan_streams");
  EG_HIP(hipSetDevice(c->device));
  const size_t entries = size_t(c->ran.n) * c->last_n;      // the slabs lie back to back: one copy, split on the host
  std::vector<uint8_t> kept(entries * kEnsembleKeptBytes);
  EG_HIP(hipMemcpy(kept.data(), c->d_ens_kept, kept.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < entries; ++i) {
    const uint8_t* e = kept.data() + i * kEnsembleKeptBytes;
    if (metrics) std::memcpy(metrics + 4 * i, e, 4 * sizeof(double));
    if (status) std::memcpy(status + i, e + 4 * sizeof(double), sizeof(int32_t));
  }
  return EG_OK;
}

}  // extern "C"
