// eg_constraints.cpp — the constraints of a context, both kinds (include/eirgrid_hip.h eg_plan_constraints_set, eg_build_constraints_set):
// the upload (set_kind), the launch behind a plan batch (constrain_batch, which eg_plans.cpp launch_plans calls), the copy of what the
// last batch was judged under (last_batch_kind) and the fetch of the two side buffers.  What a constraint may hold and its text form are
// eg_constraint_text.cpp's, the kernels eg_plan_constraints.h's and eg_build_constraints.h's.
#include <cstring>

#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_plan_constraint) == 16 && offsetof(eg_plan_constraint, to_year) == 4 && offsetof(eg_plan_constraint, bound) == 8,
              "eg_plan_constraint is part of the C ABI and what k_plan_constraints unpacks");
static_assert(sizeof(eg_build_constraint) == 168 && offsetof(eg_build_constraint, to_year) == 3 && offsetof(eg_build_constraint, bound) == 8 &&
                  offsetof(eg_build_constraint, weight) == 16,
              "eg_build_constraint is part of the C ABI and what k_build_constraints unpacks");
static_assert(EG_CONSTRAINTS_MAX <= 32, "a record's violated constraints are a 32-bit mask");

namespace {
// n constraints of one kind (c->rows | c->builds) onto the device and into the host copy; `other_kind` is what the messages call the other
template <class T> int32_t set_kind(const char* who, eg_ctx* c, ConstraintSet<T> eg_ctx::*kind, const char* other_kind, const T* constraints, int32_t n) {
  auto fail = [who](const std::string& m) { set_error(std::string(who) + ": " + m); return EG_ERR_BAD_ARG; };
  if (!c) return fail("bad argument");
  if (c->group_member) return fail("the context is a rank of an eg_group (plan batches on a group are not supported)");
  EG_TRY(validate_constraints(who, constraints, n));
  ConstraintSet<T>& mine = c->*kind;
  const int others = c->rows.n + c->builds.n - mine.n;
  if (n + others > EG_CONSTRAINTS_MAX)
    return fail("n = " + std::to_string(n) + " with " + std::to_string(others) + " " + other_kind + " constraints set (together at most " + std::to_string(EG_CONSTRAINTS_MAX) + ")");
  if (n == 0) { mine.n = 0; return EG_OK; }
  EG_HIP(hipSetDevice(c->device));
  // the pad bytes go up as zeros whatever the caller left in them
  static_assert(sizeof(mine.set) == sizeof(T) * EG_CONSTRAINTS_MAX, "the host copy is what goes up");
  std::vector<T> up(EG_CONSTRAINTS_MAX, T{});
  for (int32_t i = 0; i < n; ++i) { up[i] = constraints[i]; std::memset(up[i].pad, 0, sizeof(up[i].pad)); }
  mine.n = 0;      // (a failure below leaves none set)
  EG_HIP(mine.dev.reserve(sizeof(mine.set)));
  // (a synchronous copy on the null stream: it waits for the launch that may still read the previous constraints)
  EG_HIP(hipMemcpy(mine.dev, up.data(), sizeof(mine.set), hipMemcpyHostToDevice));
  std::memcpy(mine.set, up.data(), sizeof(mine.set));
  mine.n = n;
  return EG_OK;
}

// the constraints of one kind the last batch was judged under — `first`: the first excess columns, else the last feas_builds — into out
// (NULL: the count alone)
template <class T> int32_t last_batch_kind(const char* who, const eg_ctx* c, ConstraintSet<T> eg_ctx::*kind, bool first, T* out) {
  if (!c) { set_error(std::string(who) + ": bad argument"); return EG_ERR_BAD_ARG; }
  const int32_t k = c->last_n > 0 && c->feas_k > 0 ? (first ? c->feas_k - c->feas_builds : c->feas_builds) : 0;
  if (out) std::memcpy(out, (c->*kind).judged, sizeof(T) * size_t(k));
  return k;
}
}  // namespace

int eg::constrain_batch(eg_ctx* c, uint32_t n) {
  const uint32_t k_rows = uint32_t(c->rows.n), k_builds = uint32_t(c->builds.n), k = k_rows + k_builds;
  EG_HIP(c->d_violated.reserve(n));
  EG_HIP(c->d_excess.reserve(size_t(n) * k));
  // with no build constraint set: the launch as it always was; with one, the kernel that judges both kinds in one pass
  if (k_builds == 0) EG_LAUNCH("k_plan_constraints", launch_plan_constraints(c->out, n, c->rows.dev, k, c->d_violated, c->d_excess, nullptr));
  else EG_LAUNCH("k_build_constraints", launch_build_constraints(c->out, n, c->rows.dev, k_rows, c->builds.dev, k_builds, c->d_violated, c->d_excess, nullptr));
  std::memcpy(c->rows.judged, c->rows.set, sizeof(c->rows.judged));
  std::memcpy(c->builds.judged, c->builds.set, sizeof(c->builds.judged));
  c->feas_k = int(k); c->feas_builds = int(k_builds);
  return EG_OK;
}

extern "C" {

int32_t eg_plan_constraints_set(eg_ctx* c, const eg_plan_constraint* constraints, int32_t n) {
  return set_kind("eg_plan_constraints_set", c, &eg_ctx::rows, "build", constraints, n);
}
int32_t eg_build_constraints_set(eg_ctx* c, const eg_build_constraint* constraints, int32_t n) {
  return set_kind("eg_build_constraints_set", c, &eg_ctx::builds, "plan", constraints, n);
}

// (the row constraints are the first columns of an excess row, the build constraints the last feas_builds)
int32_t eg_last_batch_constraints(const eg_ctx* c, eg_plan_constraint* out) { return last_batch_kind("eg_last_batch_constraints", c, &eg_ctx::rows, true, out); }
int32_t eg_last_batch_build_constraints(const eg_ctx* c, eg_build_constraint* out) { return last_batch_kind("eg_last_batch_build_constraints", c, &eg_ctx::builds, false, out); }

int32_t eg_fetch_plan_feasibility(eg_ctx* c, uint32_t* violated, double* excess) {
  if (!c) { set_error("eg_fetch_plan_feasibility: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->feas_k == 0 || c->last_n == 0) { set_error("eg_fetch_plan_feasibility: the last batch ran without plan constraints"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  // (synchronous copies on the null stream: they wait for the kernel)
  if (violated) EG_HIP(hipMemcpy(violated, c->d_violated, sizeof(uint32_t) * c->last_n, hipMemcpyDeviceToHost));
  if (excess) EG_HIP(hipMemcpy(excess, c->d_excess, sizeof(double) * size_t(c->last_n) * size_t(c->feas_k), hipMemcpyDeviceToHost));
  return EG_OK;
}

}  // extern "C"
