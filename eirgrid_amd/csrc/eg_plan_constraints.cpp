// eg_plan_constraints.cpp — plan constraints (include/eirgrid_hip.h eg_plan_constraints_set): the checks, the upload, the launch behind a plan
// batch (constrain_batch, which eg_plans.cpp launch_plans calls), the fetch of the two side buffers, and the one parser and formatter of a
// constraint's text form that every front end goes through.  The kernel is eg_plan_constraints.h's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_plan_constraint) == 16 && offsetof(eg_plan_constraint, to_year) == 4 && offsetof(eg_plan_constraint, bound) == 8,
              "eg_plan_constraint is part of the C ABI and what k_plan_constraints unpacks");
static_assert(EG_CONSTRAINTS_MAX <= 32, "a record's violated constraints are a 32-bit mask");

namespace {
// the lower-case EG_Y_* names, in column order
const char* const kColumn[EG_YEARLY_FIELDS] = {"year", "pop", "usage", "gen", "balance", "opinion", "yearly_capital", "total_capital", "inflation", "co2", "offset",
                                               "net_co2", "yearly_credit", "total_credit", "yearly_sales", "total_sales", "active_gens", "upgrade_costs",
                                               "closure_costs", "yearly_total_cost", "total_cost"};
constexpr int kFirstYear = 2025;

// what is wrong with constraint c, or "" ("<field> <value> (<what it may be>)")
std::string defect(const eg_plan_constraint& c) {
  if (c.column >= EG_YEARLY_FIELDS) return "column " + std::to_string(int(c.column)) + " (an EG_Y_* column 0.." + std::to_string(EG_YEARLY_FIELDS - 1) + ")";
  if (c.aggregate > EG_AGG_SUM) return "aggregate " + std::to_string(int(c.aggregate)) + " (0 EG_AGG_EVERY, 1 EG_AGG_SUM)";
  if (c.op > EG_OP_GE) return "op " + std::to_string(int(c.op)) + " (0 EG_OP_LE, 1 EG_OP_GE)";
  if (c.to_year > EG_YEARS) return "to_year " + std::to_string(int(c.to_year)) + " (at most " + std::to_string(EG_YEARS) + ")";
  if (c.from_year >= c.to_year) return "from_year " + std::to_string(int(c.from_year)) + " >= to_year " + std::to_string(int(c.to_year)) + " (an empty window)";
  if (!std::isfinite(c.bound)) return "bound " + std::to_string(c.bound) + " (a finite number)";
  return "";
}
int validate(const char* who, const eg_plan_constraint* cs, int32_t n) {
  auto fail = [who](const std::string& m) { set_error(std::string(who) + ": " + m); return EG_ERR_BAD_ARG; };
  if (n < 0 || n > EG_CONSTRAINTS_MAX) return fail("n = " + std::to_string(n) + " (0.." + std::to_string(EG_CONSTRAINTS_MAX) + ")");
  if (n > 0 && !cs) return fail("NULL constraints with n = " + std::to_string(n));
  for (int32_t i = 0; i < n; ++i) {
    const std::string d = defect(cs[i]);
    if (!d.empty()) return fail("constraint " + std::to_string(i) + ": " + d);
  }
  return EG_OK;
}
}  // namespace

int eg::constrain_batch(eg_ctx* c, uint32_t n) {
  const uint32_t k_rows = uint32_t(c->n_constraints), k_builds = uint32_t(c->n_build_constraints), k = k_rows + k_builds;
  EG_HIP(c->d_violated.reserve(n));
  EG_HIP(c->d_excess.reserve(size_t(n) * k));
  // with no build constraint set: the launch as it always was; with one, the kernel that judges both kinds in one pass
  if (k_builds == 0) EG_LAUNCH("k_plan_constraints", launch_plan_constraints(c->out, n, c->d_constraints, k, c->d_violated, c->d_excess, nullptr));
  else EG_LAUNCH("k_build_constraints", launch_build_constraints(c->out, n, c->d_constraints, k_rows, c->d_build_constraints, k_builds, c->d_violated, c->d_excess, nullptr));
  std::memcpy(c->judged, c->constraints, sizeof(c->judged));
  std::memcpy(c->build_judged, c->build_constraints, sizeof(c->build_judged));
  c->feas_k = int(k); c->feas_builds = int(k_builds);
  return EG_OK;
}

extern "C" {

int32_t eg_plan_constraints_validate(const eg_plan_constraint* constraints, int32_t n) { return validate("eg_plan_constraints_validate", constraints, n); }

int32_t eg_plan_constraints_set(eg_ctx* c, const eg_plan_constraint* constraints, int32_t n) {
  if (!c) { set_error("eg_plan_constraints_set: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->group_member) { set_error("eg_plan_constraints_set: the context is a rank of an eg_group (plan batches on a group are not supported)"); return EG_ERR_BAD_ARG; }
  EG_TRY(validate("eg_plan_constraints_set", constraints, n));
  if (n + c->n_build_constraints > EG_CONSTRAINTS_MAX) {
    set_error("eg_plan_constraints_set: n = " + std::to_string(n) + " with " + std::to_string(c->n_build_constraints) + " build constraints set (together at most " + std::to_string(EG_CONSTRAINTS_MAX) + ")");
    return EG_ERR_BAD_ARG;
  }
  if (n == 0) { c->n_constraints = 0; return EG_OK; }
  EG_HIP(hipSetDevice(c->device));
  // the pad bytes go up as zeros whatever the caller left in them
  eg_plan_constraint up[EG_CONSTRAINTS_MAX] = {};
  for (int32_t i = 0; i < n; ++i) { up[i] = constraints[i]; std::memset(up[i].pad, 0, sizeof(up[i].pad)); }
  c->n_constraints = 0;      // (a failure below leaves none set)
  EG_HIP(c->d_constraints.reserve(sizeof(up)));
  // (a synchronous copy on the null stream: it waits for the launch that may still read the previous constraints)
  EG_HIP(hipMemcpy(c->d_constraints, up, sizeof(up), hipMemcpyHostToDevice));
  std::memcpy(c->constraints, up, sizeof(up));
  c->n_constraints = n;
  return EG_OK;
}

int32_t eg_last_batch_constraints(const eg_ctx* c, eg_plan_constraint* out) {
  if (!c) { set_error("eg_last_batch_constraints: bad argument"); return EG_ERR_BAD_ARG; }
  const int32_t k = c->last_n > 0 && c->feas_k > 0 ? c->feas_k - c->feas_builds : 0;      // (the row constraints: the first columns)
  if (out) std::memcpy(out, c->judged, sizeof(eg_plan_constraint) * size_t(k));
  return k;
}

int32_t eg_fetch_plan_feasibility(eg_ctx* c, uint32_t* violated, double* excess) {
  if (!c) { set_error("eg_fetch_plan_feasibility: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->feas_k == 0 || c->last_n == 0) { set_error("eg_fetch_plan_feasibility: the last batch ran without plan constraints"); return EG_ERR_BAD_ARG; }
  EG_HIP(hipSetDevice(c->device));
  // (synchronous copies on the null stream: they wait for the kernel)
  if (violated) EG_HIP(hipMemcpy(violated, c->d_violated, sizeof(uint32_t) * c->last_n, hipMemcpyDeviceToHost));
  if (excess) EG_HIP(hipMemcpy(excess, c->d_excess, sizeof(double) * size_t(c->last_n) * size_t(c->feas_k), hipMemcpyDeviceToHost));
  return EG_OK;
}

int32_t eg_plan_constraint_parse(const char* spec, eg_plan_constraint* out) {
  auto fail = [](const std::string& m) { set_error("eg_plan_constraint_parse: " + m); return EG_ERR_BAD_ARG; };
  if (!spec || !out) return fail("NULL argument");
  const std::string whole = spec;
  const char* p = spec;
  auto skip = [&] { while (*p == ' ' || *p == '\t') ++p; };
  auto word = [&](const char* stop) { const char* b = p; while (*p && !std::strchr(stop, *p)) ++p; return std::string(b, p); };
  eg_plan_constraint c{};
  skip();
  if (!*p) return fail("an empty constraint (\"[sum(]COLUMN[)] (<=|>=) BOUND [@FROM[:TO]]\")");
  if (std::strncmp(p, "sum(", 4) == 0) { c.aggregate = EG_AGG_SUM; p += 4; skip(); }
  const std::string name = word(" \t()<>=@");
  int col = -1;
  for (int i = 0; i < EG_YEARLY_FIELDS; ++i) if (name == kColumn[i]) col = i;
  if (col < 0) return fail("unknown column \"" + name + "\" in \"" + whole + "\" (a lower-case EG_Y_* name: net_co2, balance, yearly_total_cost, ...)");
  c.column = uint8_t(col);
  skip();
  if (c.aggregate == EG_AGG_SUM) {
    if (*p != ')') return fail("expected \")\" behind \"sum(" + name + "\", found \"" + std::string(p) + "\"");
    ++p; skip();
  }
  if (std::strncmp(p, "<=", 2) == 0) c.op = EG_OP_LE;
  else if (std::strncmp(p, ">=", 2) == 0) c.op = EG_OP_GE;
  else return fail("expected \"<=\" or \">=\" behind \"" + name + "\", found \"" + word(" \t") + "\"");
  p += 2; skip();
  const std::string number = word(" \t@");
  char* end = nullptr;
  c.bound = std::strtod(number.c_str(), &end);
  if (number.empty() || *end != '\0') return fail("bound \"" + number + "\" is not a number");
  if (!std::isfinite(c.bound)) return fail("bound \"" + number + "\" is not finite");
  skip();
  c.from_year = 0; c.to_year = EG_YEARS;
  if (*p == '@') {
    ++p;
    auto year = [&](const std::string& t, int* y) {
      char* e = nullptr;
      const long v = std::strtol(t.c_str(), &e, 10);
      if (t.empty() || *e != '\0' || v < kFirstYear || v >= kFirstYear + EG_YEARS) return false;
      *y = int(v - kFirstYear);
      return true;
    };
    const std::string from = word(" \t:");
    int y0 = 0, y1 = EG_YEARS - 1;
    if (!year(from, &y0)) return fail("year \"" + from + "\" (a calendar year 2025..2050)");
    if (*p == ':') {
      ++p;
      const std::string to = word(" \t");
      if (!year(to, &y1)) return fail("year \"" + to + "\" (a calendar year 2025..2050)");
      if (y1 < y0) return fail("window \"" + from + ":" + to + "\" ends before it starts");
    }
    c.from_year = uint8_t(y0); c.to_year = uint8_t(y1 + 1);
    skip();
  }
  if (*p) return fail("unexpected \"" + std::string(p) + "\" behind the constraint in \"" + whole + "\"");
  *out = c;
  return EG_OK;
}

int32_t eg_plan_constraint_format(const eg_plan_constraint* c, char* buf, int32_t len) {
  auto fail = [](const std::string& m) { set_error("eg_plan_constraint_format: " + m); return EG_ERR_BAD_ARG; };
  if (!c || !buf || len < 1) return fail("bad argument");
  const std::string d = defect(*c);
  if (!d.empty()) return fail(d);
  char number[40], window[16] = "";
  std::snprintf(number, sizeof(number), "%.17g", c->bound);
  if (c->to_year < EG_YEARS) std::snprintf(window, sizeof(window), " @%d:%d", kFirstYear + c->from_year, kFirstYear + c->to_year - 1);
  else if (c->from_year > 0) std::snprintf(window, sizeof(window), " @%d", kFirstYear + c->from_year);
  const std::string s = std::string(c->aggregate == EG_AGG_SUM ? "sum(" : "") + kColumn[c->column] + (c->aggregate == EG_AGG_SUM ? ")" : "") +
                        (c->op == EG_OP_GE ? " >= " : " <= ") + number + window;
  static_assert(4 + 17 + 1 + 4 + 25 + 11 < EG_CONSTRAINT_SPEC_MAX, "the longest spec fits EG_CONSTRAINT_SPEC_MAX");
  if (s.size() + 1 > size_t(len)) return fail("the buffer holds " + std::to_string(len) + " bytes (" + std::to_string(s.size() + 1) + " needed)");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return EG_OK;
}

}  // extern "C"
