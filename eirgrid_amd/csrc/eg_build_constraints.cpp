// eg_build_constraints.cpp — build constraints (include/eirgrid_hip.h eg_build_constraints_set): the checks, the upload, the copy of what the
// last batch was judged under, and the one parser and formatter of a build constraint's text form.  The launch is eg_plan_constraints.cpp
// constrain_batch's, the kernel eg_build_constraints.h's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "eg_host.h"

using namespace eg;

static_assert(sizeof(eg_build_constraint) == 168 && offsetof(eg_build_constraint, to_year) == 3 && offsetof(eg_build_constraint, bound) == 8 &&
                  offsetof(eg_build_constraint, weight) == 16,
              "eg_build_constraint is part of the C ABI and what k_build_constraints unpacks");

namespace {
// the classes in index order: eg_checkpoint.cpp kTypeName, then its kOffsetName
const char* const kClass[EG_BUILD_CLASSES] = {"OnshoreWind", "OffshoreWind", "DomesticSolar", "CommercialSolar", "UtilitySolar", "Nuclear", "CoalPlant",
                                              "GasCombinedCycle", "GasPeaker", "Biomass", "HydroDam", "PumpedStorage", "BatteryStorage", "TidalGenerator",
                                              "WaveEnergy", "Forest", "Wetland", "ActiveCapture", "CarbonCredit"};
constexpr int kGens = EG_N_TYPES;
constexpr int kFirstYear = 2025;
constexpr double kWeightMax = 1e300;
const char* const kGrammar = "\"[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]\"";

// what is wrong with constraint c, or "" ("<field> <value> (<what it may be>)")
std::string defect(const eg_build_constraint& c) {
  if (c.aggregate > EG_AGG_SUM) return "aggregate " + std::to_string(int(c.aggregate)) + " (0 EG_AGG_EVERY, 1 EG_AGG_SUM)";
  if (c.op > EG_OP_GE) return "op " + std::to_string(int(c.op)) + " (0 EG_OP_LE, 1 EG_OP_GE)";
  if (c.to_year > EG_YEARS) return "to_year " + std::to_string(int(c.to_year)) + " (at most " + std::to_string(EG_YEARS) + ")";
  if (c.from_year >= c.to_year) return "from_year " + std::to_string(int(c.from_year)) + " >= to_year " + std::to_string(int(c.to_year)) + " (an empty window)";
  if (!std::isfinite(c.bound)) return "bound " + std::to_string(c.bound) + " (a finite number)";
  bool any = false;
  for (int q = 0; q < EG_BUILD_CLASSES; ++q) {
    if (!std::isfinite(c.weight[q]) || std::fabs(c.weight[q]) > kWeightMax) {
      char v[40];
      if (std::isnan(c.weight[q])) std::snprintf(v, sizeof(v), "nan");      // (whatever its sign bit)
      else std::snprintf(v, sizeof(v), "%g", c.weight[q]);
      return "weight[" + std::to_string(q) + "] " + v + " (finite, at most 1e300 in magnitude)";
    }
    any = any || c.weight[q] != 0.0;
  }
  if (!any) return "weights all zero (at least one class counts)";
  return "";
}
int validate(const char* who, const eg_build_constraint* cs, int32_t n) {
  auto fail = [who](const std::string& m) { set_error(std::string(who) + ": " + m); return EG_ERR_BAD_ARG; };
  if (n < 0 || n > EG_CONSTRAINTS_MAX) return fail("n = " + std::to_string(n) + " (0.." + std::to_string(EG_CONSTRAINTS_MAX) + ")");
  if (n > 0 && !cs) return fail("NULL constraints with n = " + std::to_string(n));
  for (int32_t i = 0; i < n; ++i) {
    const std::string d = defect(cs[i]);
    if (!d.empty()) return fail("constraint " + std::to_string(i) + ": " + d);
  }
  return EG_OK;
}
std::string g17(double v) {
  char number[40];
  std::snprintf(number, sizeof(number), "%.17g", v);
  return number;
}
}  // namespace

extern "C" {

int32_t eg_build_constraints_validate(const eg_build_constraint* constraints, int32_t n) { return validate("eg_build_constraints_validate", constraints, n); }

int32_t eg_build_constraints_set(eg_ctx* c, const eg_build_constraint* constraints, int32_t n) {
  if (!c) { set_error("eg_build_constraints_set: bad argument"); return EG_ERR_BAD_ARG; }
  if (c->group_member) { set_error("eg_build_constraints_set: the context is a rank of an eg_group (plan batches on a group are not supported)"); return EG_ERR_BAD_ARG; }
  EG_TRY(validate("eg_build_constraints_set", constraints, n));
  if (n + c->n_constraints > EG_CONSTRAINTS_MAX) {
    set_error("eg_build_constraints_set: n = " + std::to_string(n) + " with " + std::to_string(c->n_constraints) + " plan constraints set (together at most " + std::to_string(EG_CONSTRAINTS_MAX) + ")");
    return EG_ERR_BAD_ARG;
  }
  if (n == 0) { c->n_build_constraints = 0; return EG_OK; }
  EG_HIP(hipSetDevice(c->device));
  // the pad bytes go up as zeros whatever the caller left in them
  static_assert(sizeof(c->build_constraints) == sizeof(eg_build_constraint) * EG_CONSTRAINTS_MAX, "the host copy is what goes up");
  std::vector<eg_build_constraint> up(EG_CONSTRAINTS_MAX, eg_build_constraint{});
  for (int32_t i = 0; i < n; ++i) { up[i] = constraints[i]; std::memset(up[i].pad, 0, sizeof(up[i].pad)); }
  c->n_build_constraints = 0;      // (a failure below leaves none set)
  EG_HIP(c->d_build_constraints.reserve(sizeof(c->build_constraints)));
  // (a synchronous copy on the null stream: it waits for the launch that may still read the previous constraints)
  EG_HIP(hipMemcpy(c->d_build_constraints, up.data(), sizeof(c->build_constraints), hipMemcpyHostToDevice));
  std::memcpy(c->build_constraints, up.data(), sizeof(c->build_constraints));
  c->n_build_constraints = n;
  return EG_OK;
}

int32_t eg_last_batch_build_constraints(const eg_ctx* c, eg_build_constraint* out) {
  if (!c) { set_error("eg_last_batch_build_constraints: bad argument"); return EG_ERR_BAD_ARG; }
  const int32_t k = c->last_n > 0 && c->feas_k > 0 ? c->feas_builds : 0;
  if (out) std::memcpy(out, c->build_judged, sizeof(eg_build_constraint) * size_t(k));
  return k;
}

int32_t eg_build_constraint_parse(const char* spec, eg_build_constraint* out) {
  auto fail = [](const std::string& m) { set_error("eg_build_constraint_parse: " + m); return EG_ERR_BAD_ARG; };
  if (!spec || !out) return fail("NULL argument");
  const std::string whole = spec;
  const char* p = spec;
  auto skip = [&] { while (*p == ' ' || *p == '\t') ++p; };
  auto word = [&](const char* stop) { const char* b = p; while (*p && !std::strchr(stop, *p)) ++p; return std::string(b, p); };
  eg_build_constraint c{};
  bool named[EG_BUILD_CLASSES] = {};
  skip();
  if (!*p) return fail(std::string("an empty constraint (") + kGrammar + ")");
  if (std::strncmp(p, "sum(", 4) == 0) { c.aggregate = EG_AGG_SUM; p += 4; skip(); }
  if (std::strncmp(p, "built(", 6) != 0) return fail("expected \"built(\", found \"" + word(" \t") + "\" in \"" + whole + "\" (" + kGrammar + ")");
  p += 6;
  for (bool first = true;; first = false) {
    skip();
    double sign = 1.0;
    if (!first) {
      if (*p == ')') break;
      if (*p != '+' && *p != '-') return fail("expected \"+\", \"-\" or \")\" behind a class, found \"" + word(" \t") + "\" in \"" + whole + "\"");
      sign = *p == '-' ? -1.0 : 1.0;
      ++p; skip();
    }
    // [W*]CLASS: a term's text up to the next separator; in a token that starts as a number a sign in front and behind an exponent's
    // 'e' belongs to it ("-1", "1e+3"), in a name no sign does ("BatteryStorage-OnshoreWind")
    const char* b = p;
    const bool numeric = (*p >= '0' && *p <= '9') || *p == '.' || *p == '+' || *p == '-';
    while (*p && !std::strchr(" \t()<>=@*", *p) && !((*p == '+' || *p == '-') && !(numeric && (p == b || p[-1] == 'e' || p[-1] == 'E')))) ++p;
    std::string token(b, p);
    double weight = 1.0;
    skip();
    if (*p == '*') {
      char* end = nullptr;
      weight = std::strtod(token.c_str(), &end);
      if (token.empty() || *end != '\0') return fail("weight \"" + token + "\" is not a number");
      if (!std::isfinite(weight) || std::fabs(weight) > kWeightMax) return fail("weight \"" + token + "\" (finite, at most 1e300 in magnitude)");
      ++p; skip();
      token = word(" \t()<>=@*+-");
    }
    weight = sign * weight;
    int lo = -1, hi = -1;
    if (token == "any") { lo = 0; hi = kGens; }
    for (int q = 0; q < EG_BUILD_CLASSES; ++q) if (token == kClass[q]) { lo = q; hi = q + 1; }
    if (lo < 0) return fail("unknown class \"" + token + "\" in \"" + whole + "\" (a generator type — OnshoreWind, GasPeaker, Nuclear, ... —, Forest, Wetland, ActiveCapture, CarbonCredit or any)");
    for (int q = lo; q < hi; ++q) {
      if (named[q]) return fail("class \"" + std::string(kClass[q]) + "\" is named twice in \"" + whole + "\"" + (token == "any" ? " (any names every generator type)" : ""));
      named[q] = true;
      c.weight[q] = weight;
    }
  }
  ++p; skip();      // the ")" of built(
  if (c.aggregate == EG_AGG_SUM) {
    if (*p != ')') return fail("expected \")\" behind \"sum(built(...)\", found \"" + std::string(p) + "\"");
    ++p; skip();
  }
  if (std::strncmp(p, "<=", 2) == 0) c.op = EG_OP_LE;
  else if (std::strncmp(p, ">=", 2) == 0) c.op = EG_OP_GE;
  else return fail("expected \"<=\" or \">=\" behind \"built(...)\", found \"" + word(" \t") + "\"");
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
  const std::string d = defect(c);      // (weights that cancel to nothing: "0*Nuclear")
  if (!d.empty()) return fail(d + " in \"" + whole + "\"");
  *out = c;
  return EG_OK;
}

int32_t eg_build_constraint_format(const eg_build_constraint* c, char* buf, int32_t len) {
  auto fail = [](const std::string& m) { set_error("eg_build_constraint_format: " + m); return EG_ERR_BAD_ARG; };
  if (!c || !buf || len < 1) return fail("bad argument");
  const std::string d = defect(*c);
  if (!d.empty()) return fail(d);
  bool any = c->weight[0] != 0.0;
  for (int q = 1; q < kGens; ++q) any = any && c->weight[q] == c->weight[0];
  for (int q = kGens; q < EG_BUILD_CLASSES; ++q) any = any && c->weight[q] == 0.0;
  std::string terms;
  auto term = [&](double w, const char* name) {
    if (terms.empty()) terms = (w == 1.0 ? std::string() : g17(w) + "*") + name;
    else terms += std::string(w < 0.0 ? " - " : " + ") + (std::fabs(w) == 1.0 ? std::string() : g17(std::fabs(w)) + "*") + name;
  };
  if (any) term(c->weight[0], "any");
  else for (int q = 0; q < EG_BUILD_CLASSES; ++q) if (c->weight[q] != 0.0) term(c->weight[q], kClass[q]);
  char window[16] = "";
  if (c->to_year < EG_YEARS) std::snprintf(window, sizeof(window), " @%d:%d", kFirstYear + c->from_year, kFirstYear + c->to_year - 1);
  else if (c->from_year > 0) std::snprintf(window, sizeof(window), " @%d", kFirstYear + c->from_year);
  const std::string s = std::string(c->aggregate == EG_AGG_SUM ? "sum(" : "") + "built(" + terms + ")" + (c->aggregate == EG_AGG_SUM ? ")" : "") +
                        (c->op == EG_OP_GE ? " >= " : " <= ") + g17(c->bound) + window;
  // the longest: 19 terms of " - " + 24 digits + "*" + 16 letters, "sum(built(" + "))", the operator, 24 digits, the window
  static_assert(EG_BUILD_CLASSES * (3 + 24 + 1 + 16) + 10 + 2 + 4 + 24 + 11 < EG_BUILD_SPEC_MAX, "the longest spec fits EG_BUILD_SPEC_MAX");
  if (s.size() + 1 > size_t(len)) return fail("the buffer holds " + std::to_string(len) + " bytes (" + std::to_string(s.size() + 1) + " needed)");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return EG_OK;
}

}  // extern "C"
