"""Plan constraints (include/eirgrid_hip.h eg_plan_constraints_set): a bound on one column of the yearly rows over a window of years, judged
on the device behind every plan batch of an Engine that has them set.  The text form is the library's (eg_plan_constraint_parse /
_format); `Constraint.excess` restates the definition for users who filter BatchResult.yearly on the host."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _native as N

_NAN = float("nan")      # the canonical quiet NaN a NaN excess is reported as


@dataclass(frozen=True)
class Constraint:
    """`column` (an EG_Y_* index or its lower-case name) `op` ("<=" | ">=") `bound` over the years from_year <= y < to_year (year INDICES,
    0 = 2025), for every year of the window (aggregate "every") or for the window's sum ("sum")."""
    column: "int | str"
    op: str
    bound: float
    from_year: int = 0
    to_year: int = N.YEARS
    aggregate: str = "every"

    def __post_init__(self):
        if isinstance(self.column, str):
            if self.column not in N.YEARLY_COLUMNS:
                raise ValueError(f"unknown column {self.column!r} (one of {', '.join(N.YEARLY_COLUMNS)})")
            object.__setattr__(self, "column", N.YEARLY_COLUMNS.index(self.column))
        if self.op not in ("<=", ">="):
            raise ValueError(f"op {self.op!r} ('<=' | '>=')")
        if self.aggregate not in ("every", "sum"):
            raise ValueError(f"aggregate {self.aggregate!r} ('every' | 'sum')")
        object.__setattr__(self, "bound", float(self.bound))

    def struct(self) -> N.EgPlanConstraint:
        for name in ("column", "from_year", "to_year"):
            if not 0 <= int(getattr(self, name)) <= 255:
                raise ValueError(f"{name} {getattr(self, name)} does not fit a byte")
        return N.EgPlanConstraint(int(self.column), N.AGG_SUM if self.aggregate == "sum" else N.AGG_EVERY, N.OP_GE if self.op == ">=" else N.OP_LE,
                                  int(self.from_year), int(self.to_year), (C.c_uint8 * 3)(), self.bound)

    @staticmethod
    def _from_struct(s: N.EgPlanConstraint) -> "Constraint":
        return Constraint(int(s.column), ">=" if s.op == N.OP_GE else "<=", float(s.bound), int(s.from_year), int(s.to_year),
                          "sum" if s.aggregate == N.AGG_SUM else "every")

    @staticmethod
    def parse(spec: str) -> "Constraint":
        """"[sum(]COLUMN[)] (<=|>=) BOUND [@FROM[:TO]]" with calendar years 2025..2050, inclusive (eg_plan_constraint_parse)."""
        s = N.EgPlanConstraint()
        N.check(N.lib().eg_plan_constraint_parse(str(spec).encode(), C.byref(s)), "eg_plan_constraint_parse")
        return Constraint._from_struct(s)

    def __str__(self) -> str:
        buf = C.create_string_buffer(N.CONSTRAINT_SPEC_MAX)
        s = self.struct()
        N.check(N.lib().eg_plan_constraint_format(C.byref(s), buf, len(buf)), "eg_plan_constraint_format")
        return buf.value.decode()

    def excess(self, rows) -> float:
        """The excess of this constraint over one record's rows [26][21], the header's definition restated literally: satisfied iff the
        result is <= 0 (NaN violates); a negative excess is the slack."""
        v = np.asarray(rows, dtype=np.float64).reshape(N.YEARS, N.YEARLY_FIELDS)[:, int(self.column)]
        bound, ge = np.float64(self.bound), self.op == ">="
        with np.errstate(all="ignore"):
            if self.aggregate == "sum":
                s = v[self.from_year]
                for y in range(self.from_year + 1, self.to_year):
                    s = s + v[y]
                e = bound - s if ge else s - bound
            else:
                e = bound - v[self.from_year] if ge else v[self.from_year] - bound
                for y in range(self.from_year + 1, self.to_year):
                    x = bound - v[y] if ge else v[y] - bound
                    if not math.isnan(e) and (math.isnan(x) or x > e):
                        e = x
        return _NAN if math.isnan(e) else float(e)

    def violated(self, rows) -> bool:
        return not self.excess(rows) <= 0.0

    @staticmethod
    def violation(excess_row, weights=None) -> float:
        """The violation measure V of one variant's row of the excess matrix under `weights` (None: 1.0 each): `violation` below."""
        return violation(excess_row, weights)


def violation(excess_row, weights=None) -> float:
    """The violation measure V of one variant (include/eirgrid_hip.h eg_repair_plans), the header's definition restated literally: over
    the variant's row of the excess matrix, in constraint order from +0.0, +inf for a NaN excess, weight * excess for an excess > 0 (one
    rounding), +0.0 otherwise, one rounding per addition.  weights: one per constraint, each finite and > 0; None: 1.0 each."""
    row = [float(e) for e in np.asarray(excess_row, dtype=np.float64).reshape(-1)]
    w = [1.0] * len(row) if weights is None else [float(x) for x in weights]
    if len(w) != len(row):
        raise ValueError(f"{len(w)} weights for {len(row)} constraints")
    for i, x in enumerate(w):
        if not (math.isfinite(x) and x > 0.0):
            raise ValueError(f"weights[{i}] = {x} (finite and > 0)")
    v = 0.0
    for e, x in zip(row, w):
        if e != e:
            t = math.inf
        elif e > 0.0:
            t = x * e
        else:
            t = 0.0
        v = v + t
    return v


def constraint_list(constraints) -> "list[Constraint]":
    """Constraints and specs (any iterable, walked once; None: none) as a list of Constraint"""
    return [c if isinstance(c, Constraint) else Constraint.parse(c) for c in (constraints if constraints is not None else ())]


def constraint_array(constraints):
    """(ctypes array or None, n) of a list of Constraints and specs"""
    cs = constraint_list(constraints)
    if not cs:
        return None, 0
    return (N.EgPlanConstraint * len(cs))(*[c.struct() for c in cs]), len(cs)


def add_constraint_arguments(parser) -> None:
    """--constraint SPEC (repeatable) for a script's argparse parser; apply_constraints puts them on the engine"""
    parser.add_argument("--constraint", action="append", default=[], metavar="SPEC",
                        help="a bound on the yearly rows every plan must meet, \"[sum(]COLUMN[)] (<=|>=) BOUND [@FROM[:TO]]\" with calendar years, e.g. "
                             "\"net_co2 <= 0 @2040\", \"sum(net_co2) <= 4e8\", \"balance >= 500 @2030:2039\"; repeatable (at most 32)")


def apply_constraints(engine, args) -> "list[Constraint]":
    """the --constraint specs of `args` parsed (eg_plan_constraint_parse) and set on `engine`; returns them (none given: nothing is set)"""
    cs = [Constraint.parse(spec) for spec in args.constraint]
    if cs:
        engine.set_constraints(cs)
    return cs
