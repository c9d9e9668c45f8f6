"""CPU: the host side of plan constraints (include/eirgrid_hip.h eg_plan_constraints_set) — the struct, what eg_plan_constraints_validate
accepts and refuses, the one parser and formatter, the definition of a constraint's excess restated twice (Constraint.excess, and
`excess_bytes` below, which the GPU tests import), and a refinement over the tabled oracle that the constraint turns another way."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.constraints import Constraint, constraint_array
from tests.test_refine import CASES, apply_edit, oracle_run, refine_restated, round_edits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BYTES = struct.pack("<Q", 0x7FF8000000000000)


# ---------------------------------------------------------------- the definition, restated (plain Python floats, no numpy arithmetic)
def excess_bytes(rows, c):
    """the eight bytes of constraint c's excess over one record's rows [26][21], by the header's literal order"""
    v = [float(rows[y][c.column]) for y in range(26)]
    b = float(c.bound)
    if c.aggregate == "sum":
        s = v[c.from_year]
        for y in range(c.from_year + 1, c.to_year):
            s = s + v[y]
        e = b - s if c.op == ">=" else s - b
    else:
        x = [b - t if c.op == ">=" else t - b for t in v]
        e = x[c.from_year]
        for y in range(c.from_year + 1, c.to_year):
            if e != e:
                continue
            if x[y] != x[y] or x[y] > e:
                e = x[y]
    return NAN_BYTES if e != e else struct.pack("<d", e)


def judge(yearly, status, constraints):
    """what a plan batch leaves for records with these rows [n,26,21] and statuses: (status', violated [n] u32, excess bytes [n][k])"""
    n, out = len(status), np.array(status, np.int32)
    violated, rows_out = np.zeros(n, np.uint32), []
    for j in range(n):
        if status[j] != N.EG_EP_OK:
            rows_out.append([NAN_BYTES] * len(constraints))
            continue
        ex = [excess_bytes(yearly[j], c) for c in constraints]
        for i, e in enumerate(ex):
            if not struct.unpack("<d", e)[0] <= 0.0:
                violated[j] |= np.uint32(1 << i)
        if violated[j]:
            out[j] = N.EG_EP_INFEASIBLE
        rows_out.append(ex)
    return out, violated, rows_out


# ---------------------------------------------------------------- struct and ABI
def test_struct_constants_header_and_exports_agree(built):
    assert C.sizeof(N.EgPlanConstraint) == 16
    f = N.EgPlanConstraint
    assert (f.column.offset, f.aggregate.offset, f.op.offset, f.from_year.offset, f.to_year.offset, f.pad.offset, f.bound.offset) == (0, 1, 2, 3, 4, 5, 8)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert ("typedef struct { uint8_t column /* EG_Y_*, 0..20 */, aggregate, op, from_year, to_year /* 0 <= from < to <= 26 */, pad[3]; "
            "double bound /* finite */; } eg_plan_constraint; /* 16 bytes */") in header
    for name, value, mine in (("EG_CONSTRAINTS_MAX", "32", N.CONSTRAINTS_MAX), ("EG_AGG_EVERY", "0", N.AGG_EVERY), ("EG_AGG_SUM", "1", N.AGG_SUM),
                              ("EG_OP_LE", "0", N.OP_LE), ("EG_OP_GE", "1", N.OP_GE), ("EG_EP_INFEASIBLE", r"\(-4\)", N.EG_EP_INFEASIBLE),
                              ("EG_CONSTRAINT_SPEC_MAX", "96", N.CONSTRAINT_SPEC_MAX)):
        assert re.search(rf"#define {name} {value}(\s|$)", header), name
        assert int(value.strip("\\()")) == mine, name
    L = N.lib()
    for name in ("eg_plan_constraints_validate", "eg_plan_constraints_set", "eg_fetch_plan_feasibility", "eg_last_batch_constraints", "eg_plan_constraint_parse",
                 "eg_plan_constraint_format", "eg_debug_load_yearly", "eg_debug_constrain_last_batch"):
        assert name in N.EXPORTS and hasattr(L, name), name
        assert len(re.findall(rf"^int32_t {name}\(", header, flags=re.M)) == 1, name
    # the column names are the header's EG_Y_* enumerators, lower-cased, in order
    enum = re.search(r"enum \{\s*(EG_Y_YEAR = 0.*?)\};", header, flags=re.S).group(1)
    names = [t.strip().split(" ")[0][len("EG_Y_"):].lower() for t in enum.split(",")]
    assert tuple(names) == N.YEARLY_COLUMNS and len(names) == N.YEARLY_FIELDS


# ---------------------------------------------------------------- validation
def _validate(cs, n=None):
    L = N.lib()
    arr, k = constraint_array(cs)
    rc = L.eg_plan_constraints_validate(arr, k if n is None else n)
    return rc, L.eg_last_error().decode()


def test_validate_accepts_what_the_definition_allows(built):
    assert _validate([])[0] == N.EG_OK
    assert N.lib().eg_plan_constraints_validate(None, 0) == N.EG_OK
    assert _validate([Constraint("net_co2", "<=", 0.0)])[0] == N.EG_OK
    assert _validate([Constraint(i % 21, "<=" if i & 1 else ">=", float(i) - 7.5, i % 26, i % 26 + 1, "sum" if i % 3 else "every") for i in range(32)])[0] == N.EG_OK
    for lo, hi in ((0, 1), (25, 26), (0, 26)):
        for agg in ("every", "sum"):
            rc, msg = _validate([Constraint("balance", ">=", -1e300, lo, hi, agg)])
            assert rc == N.EG_OK, msg


def _raw(**kw):
    s = Constraint("balance", "<=", 1.0).struct()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize("kw, expect", [
    (dict(column=21), "constraint 1: column 21 (an EG_Y_* column 0..20)"),
    (dict(column=255), "constraint 1: column 255 (an EG_Y_* column 0..20)"),
    (dict(aggregate=2), "constraint 1: aggregate 2 (0 EG_AGG_EVERY, 1 EG_AGG_SUM)"),
    (dict(op=2), "constraint 1: op 2 (0 EG_OP_LE, 1 EG_OP_GE)"),
    (dict(from_year=5, to_year=5), "constraint 1: from_year 5 >= to_year 5 (an empty window)"),
    (dict(from_year=9, to_year=3), "constraint 1: from_year 9 >= to_year 3 (an empty window)"),
    (dict(from_year=0, to_year=0), "constraint 1: from_year 0 >= to_year 0 (an empty window)"),
    (dict(to_year=27), "constraint 1: to_year 27 (at most 26)"),
    (dict(bound=float("inf")), "constraint 1: bound inf (a finite number)"),
    (dict(bound=float("-inf")), "constraint 1: bound -inf (a finite number)"),
    (dict(bound=float("nan")), "constraint 1: bound nan (a finite number)"),
])
def test_validate_names_the_constraint_and_the_field(built, kw, expect):
    L = N.lib()
    arr = (N.EgPlanConstraint * 2)(_raw(), _raw(**kw))
    assert L.eg_plan_constraints_validate(arr, 2) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_plan_constraints_validate: " + expect


def test_validate_refuses_counts_and_null(built):
    L = N.lib()
    arr = (N.EgPlanConstraint * 33)(*[_raw() for _ in range(33)])
    assert L.eg_plan_constraints_validate(arr, 32) == N.EG_OK
    assert L.eg_plan_constraints_validate(arr, 33) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_constraints_validate: n = 33 (0..32)"
    assert L.eg_plan_constraints_validate(arr, -1) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_constraints_validate: n = -1 (0..32)"
    assert L.eg_plan_constraints_validate(None, 2) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_constraints_validate: NULL constraints with n = 2"
    # the entry points that need a context check theirs before any device
    assert L.eg_plan_constraints_set(None, arr, 1) == N.EG_ERR_BAD_ARG and "eg_plan_constraints_set: bad argument" in L.eg_last_error().decode()
    assert L.eg_fetch_plan_feasibility(None, None, None) == N.EG_ERR_BAD_ARG
    assert L.eg_last_batch_constraints(None, None) == N.EG_ERR_BAD_ARG and "eg_last_batch_constraints: bad argument" in L.eg_last_error().decode()
    assert L.eg_debug_load_yearly(None, None, 0) == N.EG_ERR_BAD_ARG and L.eg_debug_constrain_last_batch(None) == N.EG_ERR_BAD_ARG


# ---------------------------------------------------------------- the parser
@pytest.mark.parametrize("op", ["<=", ">="])
@pytest.mark.parametrize("agg", ["every", "sum"])
def test_parse_and_format_round_trip_for_every_column_and_window_form(built, op, agg):
    for col, name in enumerate(N.YEARLY_COLUMNS):
        for (lo, hi), tail in (((0, 26), ""), ((15, 26), " @2040"), ((5, 15), " @2030:2039"), ((0, 1), " @2025:2025"), ((25, 26), " @2050")):
            bound = (-1) ** col * (col + 0.1) * 10.0 ** (3 * col - 20)
            c = Constraint(col, op, bound, lo, hi, agg)
            text = str(c)
            head = f"sum({name})" if agg == "sum" else name
            assert text.startswith(f"{head} {op} ") and text.endswith(tail) and ("@" in text) == bool(tail), text
            back = Constraint.parse(text)
            assert back == c and struct.pack("<d", back.bound) == struct.pack("<d", bound), (text, back)
            assert len(text) < N.CONSTRAINT_SPEC_MAX


def test_parse_reads_the_documented_forms(built):
    assert Constraint.parse("net_co2 <= 0 @2040") == Constraint(11, "<=", 0.0, 15, 26, "every")
    assert Constraint.parse("sum(net_co2) <= 4e8") == Constraint(11, "<=", 4e8, 0, 26, "sum")
    assert Constraint.parse("balance >= 500 @2030:2039") == Constraint(4, ">=", 500.0, 5, 15, "every")
    assert Constraint.parse("  sum( yearly_total_cost )>=-1.5e9@2025:2050 ") == Constraint(19, ">=", -1.5e9, 0, 26, "sum")
    assert Constraint.parse("balance>=0@2050") == Constraint(4, ">=", 0.0, 25, 26)
    assert str(Constraint("balance", ">=", 0.0, 0, 26)) == "balance >= 0" and str(Constraint(4, "<=", 2.5, 1, 26, "sum")) == "sum(balance) <= 2.5 @2026"


@pytest.mark.parametrize("spec, expect", [
    ("foo <= 1", 'unknown column "foo"'),
    ("Balance <= 1", 'unknown column "Balance"'),
    ("sum(nope) <= 1", 'unknown column "nope"'),
    ("balance < 1", 'expected "<=" or ">=" behind "balance", found "<"'),
    ("balance == 1", 'found "=="'),
    ("balance", 'expected "<=" or ">=" behind "balance", found ""'),
    ("balance <= abc", 'bound "abc" is not a number'),
    ("balance <= ", 'bound "" is not a number'),
    ("balance <= 1e999", 'bound "1e999" is not finite'),
    ("balance <= inf", 'bound "inf" is not finite'),
    ("balance <= nan", 'bound "nan" is not finite'),
    ("balance <= 1 @2024", 'year "2024" (a calendar year 2025..2050)'),
    ("balance <= 1 @2030:2051", 'year "2051" (a calendar year 2025..2050)'),
    ("balance <= 1 @20x0", 'year "20x0"'),
    ("balance <= 1 @", 'year ""'),
    ("balance <= 1 @2040:2030", 'window "2040:2030" ends before it starts'),
    ("sum(balance <= 1", 'expected ")" behind "sum(balance"'),
    ("balance <= 1 extra", 'unexpected "extra"'),
    ("", "an empty constraint"),
])
def test_parse_names_the_offending_token(built, spec, expect):
    L = N.lib()
    out = N.EgPlanConstraint()
    assert L.eg_plan_constraint_parse(spec.encode(), C.byref(out)) == N.EG_ERR_BAD_ARG
    msg = L.eg_last_error().decode()
    assert msg.startswith("eg_plan_constraint_parse: ") and expect in msg, msg


def test_format_refuses_bad_constraints_and_short_buffers(built):
    L = N.lib()
    buf = C.create_string_buffer(N.CONSTRAINT_SPEC_MAX)
    bad = _raw(column=30)
    assert L.eg_plan_constraint_format(C.byref(bad), buf, len(buf)) == N.EG_ERR_BAD_ARG and "column 30" in L.eg_last_error().decode()
    ok = Constraint("yearly_total_cost", ">=", -1.2345678901234567e-300, 3, 9, "sum").struct()
    assert L.eg_plan_constraint_format(C.byref(ok), buf, 8) == N.EG_ERR_BAD_ARG and "the buffer holds 8 bytes" in L.eg_last_error().decode()
    assert L.eg_plan_constraint_format(C.byref(ok), buf, len(buf)) == N.EG_OK
    assert buf.value.decode() == "sum(yearly_total_cost) >= %.17g @2028:2033" % -1.2345678901234567e-300      # (17 significant digits)
    assert buf.value.decode().startswith("sum(yearly_total_cost) >= -1.23456789012345") and len(buf.value) + 1 <= N.CONSTRAINT_SPEC_MAX
    assert L.eg_plan_constraint_parse(None, None) == N.EG_ERR_BAD_ARG and L.eg_plan_constraint_format(None, None, 0) == N.EG_ERR_BAD_ARG


# ---------------------------------------------------------------- the restatement, twice
def _rows(col, values, fill=1.0):
    rows = np.full((26, 21), fill)
    rows[:len(values), col] = values
    return rows


NAN, INF = float("nan"), float("inf")
CRAFTED = [
    # (column values from year 0, constraint, the excess it must give)
    ([NAN, 1.0, 2.0], Constraint(4, "<=", 5.0, 0, 3), NAN),                     # NaN first
    ([1.0, NAN, 9.0], Constraint(4, "<=", 5.0, 0, 3), NAN),                     # ... in the middle: it sticks, the 9 behind it does not replace it
    ([1.0, 9.0, NAN], Constraint(4, "<=", 5.0, 0, 3), NAN),                     # ... last
    ([1.0, 9.0, NAN], Constraint(4, "<=", 5.0, 0, 2), 4.0),                     # ... outside the window
    ([1.0, NAN, 2.0], Constraint(4, ">=", 5.0, 0, 3, "sum"), NAN),
    ([INF, 1.0], Constraint(4, "<=", 5.0, 0, 2), INF),
    ([-INF, 1.0], Constraint(4, "<=", 5.0, 0, 2), -4.0),
    ([-INF, -INF], Constraint(4, ">=", 5.0, 0, 2), INF),
    ([INF, -INF], Constraint(4, "<=", 5.0, 0, 2, "sum"), NAN),                  # inf + -inf
    ([INF, INF], Constraint(4, ">=", 5.0, 0, 2, "sum"), -INF),
    ([-0.0, 0.0], Constraint(4, "<=", 0.0, 0, 2), -0.0),                        # -0.0 - 0.0 = -0.0 first; 0.0 is not greater: it stays
    ([0.0, -0.0], Constraint(4, "<=", 0.0, 0, 2), 0.0),
    ([-0.0, -0.0], Constraint(4, ">=", 0.0, 0, 2), 0.0),                        # 0.0 - -0.0 = 0.0
    ([-0.0, -0.0], Constraint(4, "<=", 0.0, 0, 2, "sum"), -0.0),
    ([5.0, 5.0, 5.0], Constraint(4, "<=", 5.0, 0, 3), 0.0),                     # value == bound: satisfied
    ([5.0, 5.0, 5.0], Constraint(4, ">=", 5.0, 0, 3), 0.0),
    ([2.0, 3.0], Constraint(4, "<=", 5.0, 0, 2, "sum"), 0.0),
    ([7.0, 1.0, 8.0], Constraint(4, "<=", 5.0, 1, 2), -4.0),                    # a window of one year
    ([7.0, 1.0, 8.0], Constraint(4, ">=", 5.0, 1, 2, "sum"), 4.0),
    ([0.1, 0.2, 0.3], Constraint(4, "<=", 0.0, 0, 3, "sum"), (0.1 + 0.2) + 0.3),      # year order: not 0.1 + (0.2 + 0.3)
    ([1e16, 1.0, 1.0, -1e16], Constraint(4, ">=", 0.0, 0, 4, "sum"), 0.0),      # every addition rounds: the ones are lost
]


@pytest.mark.parametrize("k", range(len(CRAFTED)))
def test_excess_is_the_definition_on_crafted_rows(k):
    values, c, want = CRAFTED[k]
    rows = _rows(4, values)
    got = c.excess(rows)
    assert struct.pack("<d", got) == excess_bytes(rows, c) == (NAN_BYTES if want != want else struct.pack("<d", want)), (got, want)
    assert c.violated(rows) == (not want <= 0.0)


def test_excess_agrees_with_the_second_loop_on_seeded_rows():
    rng = np.random.default_rng(11)
    special = np.array([NAN, INF, -INF, -0.0, 0.0, 3.0])
    for trial in range(200):
        rows = rng.normal(0.0, 10.0, (26, 21)).round(1)
        hit = rng.random((26, 21)) < 0.08
        rows[hit] = rng.choice(special, int(hit.sum()))
        lo = int(rng.integers(0, 26)); hi = int(rng.integers(lo + 1, 27))
        c = Constraint(int(rng.integers(0, 21)), "<=" if trial & 1 else ">=", float(rng.choice([3.0, 0.0, -0.0, 12.5])), lo, hi, "sum" if trial % 3 == 0 else "every")
        assert struct.pack("<d", c.excess(rows)) == excess_bytes(rows, c), (trial, c)


def test_constraint_refuses_what_it_cannot_mean():
    for bad in (lambda: Constraint("nope", "<=", 0), lambda: Constraint(0, "<", 0), lambda: Constraint(0, "<=", 0, aggregate="max")):
        with pytest.raises(ValueError):
            bad()
    assert Constraint("balance", ">=", 1).column == 4 and isinstance(Constraint("balance", ">=", 1).bound, float)


# ---------------------------------------------------------------- constrained refinement over the tabled oracle
class Demoting:
    """an evaluator for refine_restated that demotes, as a plan batch with `constraints` set does: a variant that ended EG_EP_OK and whose
    rows violate one comes back EG_EP_INFEASIBLE.  rows_of(plan) gives a plan's rows [26][21]."""

    def __init__(self, evaluate, rows_of, constraints):
        self.evaluate, self.rows_of, self.constraints = evaluate, rows_of, constraints
        self.rounds = []      # per round: the statuses as demoted

    def __call__(self, plan, edits):
        status, metrics = self.evaluate(plan, edits)
        status = np.array(status, np.int32)
        for j, e in enumerate(edits):
            if status[j] == N.EG_EP_OK and any(c.violated(self.rows_of(apply_edit(plan, e))) for c in self.constraints):
                status[j] = N.EG_EP_INFEASIBLE
        self.rounds.append(status)
        return status, metrics


def test_a_reserve_on_the_balance_turns_the_short_refinement_another_way(world):
    name = "short, mode 2"
    pol, base, ev, (plan, steps, stop, start, ties) = oracle_run(world, name)
    case = CASES[name]
    rows = {}

    def rows_of(p):
        key = (repr(p.best_actions), repr(p.best_deficit_actions))
        if key not in rows:
            rows[key] = np.array(ev.record(p).yearly, np.float64).reshape(26, 21).copy()
        return rows[key]

    floor = float(rows_of(base)[:, 4].min())      # the base's own minimum balance over the 26 years
    assert 1190.42 < floor < 1190.43
    c = Constraint("balance", ">=", floor)
    ev2 = Demoting(ev, rows_of, [c])
    plan2, steps2, stop2, start2, ties2 = refine_restated(ev2, base, case["mode"], 1, case["replace_with"])
    first = ev2.rounds[0]
    assert len(first) == 239 and first[0] == N.EG_EP_OK                       # (the base satisfies its own minimum: excess 0)
    feasible = int((first == N.EG_EP_OK).sum())
    assert 0 < feasible < 239 and feasible == 229
    assert steps and steps2 and steps2[0][1] != steps[0][1] and (steps[0][1], steps2[0][1]) == (1, 2)
    assert steps2[0][0] == round_edits(base, case["replace_with"])[2] and steps2[0][0].kind == "delete" and (steps2[0][0].year, steps2[0][0].pos) == (0, 1)
    assert steps2[0][3] == 10                                                 # n_failed counts the infeasible variants
    assert first[1] == N.EG_EP_INFEASIBLE and math.floor(rows_of(apply_edit(base, steps[0][0]))[:, 4].min()) == 398      # the unconstrained winner's dip
    assert start2 == start
