// eg_constraint_text.cpp — what a constraint of either kind (include/eirgrid_hip.h eg_plan_constraint, eg_build_constraint) may hold and how
// it is written: the checks (validate_constraints, which the setters in eg_constraints.cpp call too) and the one parser and formatter of
// the text form that every front end goes through.  The two kinds differ in their head — a column of the yearly rows, or built(...) with
// its weighted classes —; the aggregate around it and everything behind it ("(<=|>=) BOUND [@FROM[:TO]]") is one grammar, written once
// (Cursor, parse_sum_prefix, parse_tail, format_tail).  Plain C++: no HIP, nothing of a context.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "eg_internal.h"

using namespace eg;

namespace {
// the lower-case EG_Y_* names, in column order
const char* const kColumn[EG_YEARLY_FIELDS] = {"year", "pop", "usage", "gen", "balance", "opinion", "yearly_capital", "total_capital", "inflation", "co2", "offset",
                                               "net_co2", "yearly_credit", "total_credit", "yearly_sales", "total_sales", "active_gens", "upgrade_costs",
                                               "closure_costs", "yearly_total_cost", "total_cost"};
// the classes in index order: eg_checkpoint.cpp kTypeName, then its kOffsetName
const char* const kClass[EG_BUILD_CLASSES] = {"OnshoreWind", "OffshoreWind", "DomesticSolar", "CommercialSolar", "UtilitySolar", "Nuclear", "CoalPlant",
                                              "GasCombinedCycle", "GasPeaker", "Biomass", "HydroDam", "PumpedStorage", "BatteryStorage", "TidalGenerator",
                                              "WaveEnergy", "Forest", "Wetland", "ActiveCapture", "CarbonCredit"};
constexpr int kGens = EG_N_TYPES;
constexpr int kFirstYear = 2025;
constexpr double kWeightMax = 1e300;
const char* const kGrammar = "\"[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]\"";

// ---- the checks: what is wrong with a constraint, or "" ("<field> <value> (<what it may be>)") ----------------------------------------------
// the fields both kinds hold
std::string window_defect(uint8_t aggregate, uint8_t op, uint8_t from_year, uint8_t to_year, double bound) {
  if (aggregate > EG_AGG_SUM) return "aggregate " + std::to_string(int(aggregate)) + " (0 EG_AGG_EVERY, 1 EG_AGG_SUM)";
  if (op > EG_OP_GE) return "op " + std::to_string(int(op)) + " (0 EG_OP_LE, 1 EG_OP_GE)";
  if (to_year > EG_YEARS) return "to_year " + std::to_string(int(to_year)) + " (at most " + std::to_string(EG_YEARS) + ")";
  if (from_year >= to_year) return "from_year " + std::to_string(int(from_year)) + " >= to_year " + std::to_string(int(to_year)) + " (an empty window)";
  if (!std::isfinite(bound)) return "bound " + std::to_string(bound) + " (a finite number)";
  return "";
}
// (the column is the first field of the struct and the first that is named)
std::string defect(const eg_plan_constraint& c) {
  if (c.column >= EG_YEARLY_FIELDS) return "column " + std::to_string(int(c.column)) + " (an EG_Y_* column 0.." + std::to_string(EG_YEARLY_FIELDS - 1) + ")";
  return window_defect(c.aggregate, c.op, c.from_year, c.to_year, c.bound);
}
std::string defect(const eg_build_constraint& c) {
  const std::string d = window_defect(c.aggregate, c.op, c.from_year, c.to_year, c.bound);
  if (!d.empty()) return d;
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
}  // namespace

template <class T> int eg::validate_constraints(const char* who, const T* cs, int32_t n) {
  auto fail = [who](const std::string& m) { set_error(std::string(who) + ": " + m); return EG_ERR_BAD_ARG; };
  if (n < 0 || n > EG_CONSTRAINTS_MAX) return fail("n = " + std::to_string(n) + " (0.." + std::to_string(EG_CONSTRAINTS_MAX) + ")");
  if (n > 0 && !cs) return fail("NULL constraints with n = " + std::to_string(n));
  for (int32_t i = 0; i < n; ++i) {
    const std::string d = defect(cs[i]);
    if (!d.empty()) return fail("constraint " + std::to_string(i) + ": " + d);
  }
  return EG_OK;
}
template int eg::validate_constraints(const char*, const eg_plan_constraint*, int32_t);
template int eg::validate_constraints(const char*, const eg_build_constraint*, int32_t);

namespace {
// ---- the text form -----------------------------------------------------------------------------------------------------------------------
struct Cursor {
  const char* p;
  void skip() { while (*p == ' ' || *p == '\t') ++p; }
  // the text up to the next character of `stop` (or the end), taken
  std::string word(const char* stop) { const char* b = p; while (*p && !std::strchr(stop, *p)) ++p; return std::string(b, p); }
  bool take(const char* literal) { const size_t n = std::strlen(literal); if (std::strncmp(p, literal, n) != 0) return false; p += n; return true; }
};

// "[sum(]" in front of the head: the aggregate
uint8_t parse_sum_prefix(Cursor& t) {
  if (!t.take("sum(")) return EG_AGG_EVERY;
  t.skip();
  return EG_AGG_SUM;
}

// behind the head: "[)] (<=|>=) BOUND [@FROM[:TO]]" and nothing more, into c's op, bound and window (c->aggregate says whether a ")" closes
// a sum).  `head` is how the messages name what stands in front, `whole` the spec.  Returns what is wrong, or ""
template <class T> std::string parse_tail(Cursor& t, const std::string& head, const std::string& whole, T* c) {
  if (c->aggregate == EG_AGG_SUM) {
    if (*t.p != ')') return "expected \")\" behind \"sum(" + head + "\", found \"" + std::string(t.p) + "\"";
    ++t.p; t.skip();
  }
  if (t.take("<=")) c->op = EG_OP_LE;
  else if (t.take(">=")) c->op = EG_OP_GE;
  else return "expected \"<=\" or \">=\" behind \"" + head + "\", found \"" + t.word(" \t") + "\"";
  t.skip();
  const std::string number = t.word(" \t@");
  char* end = nullptr;
  c->bound = std::strtod(number.c_str(), &end);
  if (number.empty() || *end != '\0') return "bound \"" + number + "\" is not a number";
  if (!std::isfinite(c->bound)) return "bound \"" + number + "\" is not finite";
  t.skip();
  c->from_year = 0; c->to_year = EG_YEARS;
  if (*t.p == '@') {
    ++t.p;
    // a calendar year as a year index, or what is wrong with it
    auto year = [](const std::string& s, int* y) -> std::string {
      char* e = nullptr;
      const long v = std::strtol(s.c_str(), &e, 10);
      if (s.empty() || *e != '\0' || v < kFirstYear || v >= kFirstYear + EG_YEARS) return "year \"" + s + "\" (a calendar year 2025..2050)";
      *y = int(v - kFirstYear);
      return "";
    };
    const std::string from = t.word(" \t:");
    int y0 = 0, y1 = EG_YEARS - 1;
    std::string d = year(from, &y0);
    if (!d.empty()) return d;
    if (*t.p == ':') {
      ++t.p;
      const std::string to = t.word(" \t");
      d = year(to, &y1);
      if (!d.empty()) return d;
      if (y1 < y0) return "window \"" + from + ":" + to + "\" ends before it starts";
    }
    c->from_year = uint8_t(y0); c->to_year = uint8_t(y1 + 1);
    t.skip();
  }
  if (*t.p) return "unexpected \"" + std::string(t.p) + "\" behind the constraint in \"" + whole + "\"";
  return "";
}

std::string g17(double v) {
  char number[40];
  std::snprintf(number, sizeof(number), "%.17g", v);
  return number;
}

// the spec of a valid constraint whose head is written `head`: the aggregate around it, then the operator, the bound and the window
template <class T> std::string format_tail(const T& c, const std::string& head) {
  char window[16] = "";
  if (c.to_year < EG_YEARS) std::snprintf(window, sizeof(window), " @%d:%d", kFirstYear + c.from_year, kFirstYear + c.to_year - 1);
  else if (c.from_year > 0) std::snprintf(window, sizeof(window), " @%d", kFirstYear + c.from_year);
  return (c.aggregate == EG_AGG_SUM ? "sum(" + head + ")" : head) + (c.op == EG_OP_GE ? " >= " : " <= ") + g17(c.bound) + window;
}

std::string head_of(const eg_plan_constraint& c) { return kColumn[c.column]; }
std::string head_of(const eg_build_constraint& c) {
  bool any = c.weight[0] != 0.0;
  for (int q = 1; q < kGens; ++q) any = any && c.weight[q] == c.weight[0];
  for (int q = kGens; q < EG_BUILD_CLASSES; ++q) any = any && c.weight[q] == 0.0;
  std::string terms;
  auto term = [&](double w, const char* name) {
    if (terms.empty()) terms = (w == 1.0 ? std::string() : g17(w) + "*") + name;
    else terms += std::string(w < 0.0 ? " - " : " + ") + (std::fabs(w) == 1.0 ? std::string() : g17(std::fabs(w)) + "*") + name;
  };
  if (any) term(c.weight[0], "any");
  else for (int q = 0; q < EG_BUILD_CLASSES; ++q) if (c.weight[q] != 0.0) term(c.weight[q], kClass[q]);
  return "built(" + terms + ")";
}

// the longest row spec: "sum(" 17 letters ")" the operator, 25 characters of bound, the window
static_assert(4 + 17 + 1 + 4 + 25 + 11 < EG_CONSTRAINT_SPEC_MAX, "the longest spec fits EG_CONSTRAINT_SPEC_MAX");
// the longest build spec: 19 terms of " - " + 24 digits + "*" + 16 letters, "sum(built(" + "))", the operator, 24 digits, the window
static_assert(EG_BUILD_CLASSES * (3 + 24 + 1 + 16) + 10 + 2 + 4 + 24 + 11 < EG_BUILD_SPEC_MAX, "the longest spec fits EG_BUILD_SPEC_MAX");

template <class T> int32_t format_constraint(const char* who, const T* c, char* buf, int32_t len) {
  auto fail = [who](const std::string& m) { set_error(std::string(who) + ": " + m); return EG_ERR_BAD_ARG; };
  if (!c || !buf || len < 1) return fail("bad argument");
  const std::string d = defect(*c);
  if (!d.empty()) return fail(d);
  const std::string s = format_tail(*c, head_of(*c));
  if (s.size() + 1 > size_t(len)) return fail("the buffer holds " + std::to_string(len) + " bytes (" + std::to_string(s.size() + 1) + " needed)");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return EG_OK;
}
}  // namespace

extern "C" {

int32_t eg_plan_constraints_validate(const eg_plan_constraint* constraints, int32_t n) { return validate_constraints("eg_plan_constraints_validate", constraints, n); }
int32_t eg_build_constraints_validate(const eg_build_constraint* constraints, int32_t n) { return validate_constraints("eg_build_constraints_validate", constraints, n); }

int32_t eg_plan_constraint_parse(const char* spec, eg_plan_constraint* out) {
  auto fail = [](const std::string& m) { set_error("eg_plan_constraint_parse: " + m); return EG_ERR_BAD_ARG; };
  if (!spec || !out) return fail("NULL argument");
  const std::string whole = spec;
  Cursor t{spec};
  eg_plan_constraint c{};
  t.skip();
  if (!*t.p) return fail("an empty constraint (\"[sum(]COLUMN[)] (<=|>=) BOUND [@FROM[:TO]]\")");
  c.aggregate = parse_sum_prefix(t);
  const std::string name = t.word(" \t()<>=@");
  int col = -1;
  for (int i = 0; i < EG_YEARLY_FIELDS; ++i) if (name == kColumn[i]) col = i;
  if (col < 0) return fail("unknown column \"" + name + "\" in \"" + whole + "\" (a lower-case EG_Y_* name: net_co2, balance, yearly_total_cost, ...)");
  c.column = uint8_t(col);
  t.skip();
  const std::string d = parse_tail(t, name, whole, &c);
  if (!d.empty()) return fail(d);
  *out = c;
  return EG_OK;
}

int32_t eg_build_constraint_parse(const char* spec, eg_build_constraint* out) {
  auto fail = [](const std::string& m) { set_error("eg_build_constraint_parse: " + m); return EG_ERR_BAD_ARG; };
  if (!spec || !out) return fail("NULL argument");
  const std::string whole = spec;
  Cursor t{spec};
  const char*& p = t.p;
  eg_build_constraint c{};
  bool named[EG_BUILD_CLASSES] = {};
  t.skip();
  if (!*p) return fail(std::string("an empty constraint (") + kGrammar + ")");
  c.aggregate = parse_sum_prefix(t);
  if (!t.take("built(")) return fail("expected \"built(\", found \"" + t.word(" \t") + "\" in \"" + whole + "\" (" + kGrammar + ")");
  for (bool first = true;; first = false) {
    t.skip();
    double sign = 1.0;
    if (!first) {
      if (*p == ')') break;
      if (*p != '+' && *p != '-') return fail("expected \"+\", \"-\" or \")\" behind a class, found \"" + t.word(" \t") + "\" in \"" + whole + "\"");
      sign = *p == '-' ? -1.0 : 1.0;
      ++p; t.skip();
    }
    // [W*]CLASS: a term's text up to the next separator; in a token that starts as a number a sign in front and behind an exponent's
    // 'e' belongs to it ("-1", "1e+3"), in a name no sign does ("BatteryStorage-OnshoreWind")
    const char* b = p;
    const bool numeric = (*p >= '0' && *p <= '9') || *p == '.' || *p == '+' || *p == '-';
    while (*p && !std::strchr(" \t()<>=@*", *p) && !((*p == '+' || *p == '-') && !(numeric && (p == b || p[-1] == 'e' || p[-1] == 'E')))) ++p;
    std::string token(b, p);
    double weight = 1.0;
    t.skip();
    if (*p == '*') {
      char* end = nullptr;
      weight = std::strtod(token.c_str(), &end);
      if (token.empty() || *end != '\0') return fail("weight \"" + token + "\" is not a number");
      if (!std::isfinite(weight) || std::fabs(weight) > kWeightMax) return fail("weight \"" + token + "\" (finite, at most 1e300 in magnitude)");
      ++p; t.skip();
      token = t.word(" \t()<>=@*+-");
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
  ++p; t.skip();      // the ")" of built(
  std::string d = parse_tail(t, "built(...)", whole, &c);
  if (!d.empty()) return fail(d);
  d = defect(c);      // (weights that cancel to nothing: "0*Nuclear")
  if (!d.empty()) return fail(d + " in \"" + whole + "\"");
  *out = c;
  return EG_OK;
}

int32_t eg_plan_constraint_format(const eg_plan_constraint* c, char* buf, int32_t len) { return format_constraint("eg_plan_constraint_format", c, buf, len); }
int32_t eg_build_constraint_format(const eg_build_constraint* c, char* buf, int32_t len) { return format_constraint("eg_build_constraint_format", c, buf, len); }

}  // extern "C"
