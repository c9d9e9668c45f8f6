"""Plan constraints (include/eirgrid_hip.h eg_plan_constraints_set): a bound on one column of the yearly rows over a window of years, judged
on the device behind every plan batch of an Engine that has them set; and build constraints (eg_build_constraints_set, BuildConstraint): a
bound on the weighted count of what an episode built, per year or over a window, judged with them.  The text form is the library's (eg_plan_constraint_parse /
_format); `Constraint.excess` restates the definition for users who filter BatchResult.yearly on the host."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _native as N

_NAN = float("nan")      # the canonical quiet NaN a NaN excess is reported as


# ---- what Constraint and BuildConstraint share: the fields behind the head and the fold of an "every" window ---------------------------
def _check_tail(c) -> None:
    """op and aggregate of a new constraint of either kind checked, its bound made a float"""
    if c.op not in ("<=", ">="):
        raise ValueError(f"op {c.op!r} ('<=' | '>=')")
    if c.aggregate not in ("every", "sum"):
        raise ValueError(f"aggregate {c.aggregate!r} ('every' | 'sum')")
    object.__setattr__(c, "bound", float(c.bound))


def _bytes(c, *names) -> "list[int]":
    """the named fields of c as ints that fit a byte"""
    for name in names:
        if not 0 <= int(getattr(c, name)) <= 255:
            raise ValueError(f"{name} {getattr(c, name)} does not fit a byte")
    return [int(getattr(c, name)) for name in names]


def _codes(c) -> "tuple[int, int]":
    """(aggregate, op) of c as the struct holds them"""
    return N.AGG_SUM if c.aggregate == "sum" else N.AGG_EVERY, N.OP_GE if c.op == ">=" else N.OP_LE


def _names(s) -> "tuple[str, str]":
    """(op, aggregate) of a struct of either kind as the classes hold them"""
    return ">=" if s.op == N.OP_GE else "<=", "sum" if s.aggregate == N.AGG_SUM else "every"


def _largest(excesses) -> float:
    """the largest of a window's yearly excesses, a NaN sticky: the first year's value, then year by year in order"""
    it = iter(excesses)
    e = next(it, None)      # (None: no year at all)
    for x in it:
        if not math.isnan(e) and (math.isnan(x) or x > e):
            e = x
    return e


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
        _check_tail(self)

    def struct(self) -> N.EgPlanConstraint:
        column, from_year, to_year = _bytes(self, "column", "from_year", "to_year")
        return N.EgPlanConstraint(column, *_codes(self), from_year, to_year, (C.c_uint8 * 3)(), self.bound)

    @staticmethod
    def _from_struct(s: N.EgPlanConstraint) -> "Constraint":
        op, aggregate = _names(s)
        return Constraint(int(s.column), op, float(s.bound), int(s.from_year), int(s.to_year), aggregate)

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
                years = (self.from_year, *range(self.from_year + 1, self.to_year))      # (from_year itself whatever to_year is, as the sum)
                e = _largest(bound - v[y] if ge else v[y] - bound for y in years)
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


def _class_index(key) -> int:
    if isinstance(key, str):
        if key not in N.BUILD_CLASS_NAMES:
            raise ValueError(f"unknown class {key!r} (one of {', '.join(N.BUILD_CLASS_NAMES)})")
        return N.BUILD_CLASS_NAMES.index(key)
    if not 0 <= int(key) < N.BUILD_CLASSES:
        raise ValueError(f"class {key} (0..{N.BUILD_CLASSES - 1})")
    return int(key)


@dataclass(frozen=True)
class BuildConstraint:
    """A bound on what an episode BUILT (include/eirgrid_hip.h eg_build_constraints_set): the weighted count of the entries of its record's
    gen_pack / off_pack lists per class — `weights`: a dict of class name or index -> weight ("any": the 15 generator types), or 19
    numbers in N.BUILD_CLASS_NAMES order — `op` ("<=" | ">=") `bound`, for every year of the window from_year <= y < to_year (year
    INDICES, 0 = 2025; aggregate "every": a build rate) or for the window's total ("sum")."""
    weights: "dict | tuple"
    op: str
    bound: float
    from_year: int = 0
    to_year: int = N.YEARS
    aggregate: str = "every"

    def __post_init__(self):
        if isinstance(self.weights, dict):
            w = [0.0] * N.BUILD_CLASSES
            for key, x in self.weights.items():
                for q in (range(15) if key == "any" else (_class_index(key),)):
                    w[q] = float(x)
        else:
            w = [float(x) for x in self.weights]
            if len(w) != N.BUILD_CLASSES:
                raise ValueError(f"{len(w)} weights ({N.BUILD_CLASSES}: one per class)")
        object.__setattr__(self, "weights", tuple(w))
        _check_tail(self)

    def struct(self) -> N.EgBuildConstraint:
        from_year, to_year = _bytes(self, "from_year", "to_year")
        return N.EgBuildConstraint(*_codes(self), from_year, to_year, (C.c_uint8 * 4)(), self.bound, (C.c_double * N.BUILD_CLASSES)(*self.weights))

    @staticmethod
    def _from_struct(s: N.EgBuildConstraint) -> "BuildConstraint":
        op, aggregate = _names(s)
        return BuildConstraint(tuple(s.weight[:]), op, float(s.bound), int(s.from_year), int(s.to_year), aggregate)

    @staticmethod
    def parse(spec: str) -> "BuildConstraint":
        """"[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]" with calendar years (eg_build_constraint_parse)."""
        s = N.EgBuildConstraint()
        N.check(N.lib().eg_build_constraint_parse(str(spec).encode(), C.byref(s)), "eg_build_constraint_parse")
        return BuildConstraint._from_struct(s)

    def __str__(self) -> str:
        buf = C.create_string_buffer(N.BUILD_SPEC_MAX)
        s = self.struct()
        N.check(N.lib().eg_build_constraint_format(C.byref(s), buf, len(buf)), "eg_build_constraint_format")
        return buf.value.decode()

    @staticmethod
    def counts(gen_pack, n_gens, off_pack, n_offsets) -> np.ndarray:
        """c[26][19] of one record's lists, the header's definition restated: the entries in front of the counts (clamped to the lists), a
        class or a year out of range counts nowhere."""
        c = np.zeros((N.YEARS, N.BUILD_CLASSES), np.int64)
        for pack, count, base, classes in ((gen_pack, n_gens, 0, 15), (off_pack, n_offsets, 15, 4)):
            pack = np.asarray(pack).reshape(-1)
            for pk in pack[:min(max(int(count), 0), len(pack))].tolist():
                q, y = int(pk) & 15, (int(pk) >> 4) & 31
                if q < classes and y < N.YEARS:
                    c[y, base + q] += 1
        return c

    def value(self, m) -> float:
        """value(m) of a count vector m[19]: from +0.0, s = s + weight[q] * m[q] in class order, each product and each sum rounded once"""
        s = 0.0
        for q in range(N.BUILD_CLASSES):
            s = s + self.weights[q] * float(int(m[q]))
        return s

    def excess(self, gen_pack, n_gens, off_pack, n_offsets) -> float:
        """The excess of this constraint over one record's lists, the header's definition restated in plain Python floats: satisfied iff
        the result is <= 0; a negative excess is the slack."""
        c = self.counts(gen_pack, n_gens, off_pack, n_offsets)
        ge = self.op == ">="
        if self.aggregate == "sum":
            s = self.value(c[self.from_year:self.to_year].sum(axis=0))
            e = self.bound - s if ge else s - self.bound
        else:
            values = (self.value(c[y]) for y in range(self.from_year, self.to_year))
            e = _largest(self.bound - s if ge else s - self.bound for s in values)
        return _NAN if math.isnan(e) else float(e)

    def violated(self, gen_pack, n_gens, off_pack, n_offsets) -> bool:
        return not self.excess(gen_pack, n_gens, off_pack, n_offsets) <= 0.0


def constraint_list(constraints) -> "list[Constraint | BuildConstraint]":
    """Constraints and specs (any iterable, walked once; None: none) as a list of Constraint and BuildConstraint: a spec that contains
    "built(" is a build constraint's"""
    def one(c):
        if isinstance(c, (Constraint, BuildConstraint)):
            return c
        return BuildConstraint.parse(c) if "built(" in str(c) else Constraint.parse(c)
    return [one(c) for c in (constraints if constraints is not None else ())]


def record_violates(c, result, e: int) -> bool:
    """whether episode e of a BatchResult violates the constraint c of either kind, by the host restatements"""
    if isinstance(c, BuildConstraint):
        return c.violated(result.gen_pack[e], result.n_gens[e], result.off_pack[e], result.n_offsets[e])
    return c.violated(result.yearly[e])


def split_constraints(constraints) -> "tuple[list[Constraint], list[BuildConstraint]]":
    """(row constraints, build constraints) of a mixed list, which holds the row constraints first — mask bits, excess columns and repair
    weights follow the list's order, so a row constraint behind a build constraint is refused, not moved"""
    cs = constraint_list(constraints)
    n_rows = next((i for i, c in enumerate(cs) if isinstance(c, BuildConstraint)), len(cs))
    for i, c in enumerate(cs[n_rows:], n_rows):
        if isinstance(c, Constraint):
            raise ValueError(f"constraint {i} ({c}) is a row constraint behind a build constraint ({cs[n_rows]}): list the row constraints first "
                             "(mask bits, excess columns and weights follow the list's order)")
    return cs[:n_rows], cs[n_rows:]


def struct_array(cs, ctype):
    """(ctypes array of `ctype` or None, n) of a list of constraints of one kind"""
    cs = list(cs)
    if not cs:
        return None, 0
    return (ctype * len(cs))(*[c.struct() for c in cs]), len(cs)


def build_constraint_array(constraints):
    """(ctypes array or None, n) of a list of BuildConstraints"""
    return struct_array(constraints, N.EgBuildConstraint)


def constraint_array(constraints):
    """(ctypes array or None, n) of a list of Constraints and specs"""
    return struct_array(constraint_list(constraints), N.EgPlanConstraint)


def add_constraint_arguments(parser) -> None:
    """--constraint SPEC (repeatable) for a script's argparse parser; apply_constraints puts them on the engine"""
    parser.add_argument("--constraint", action="append", default=[], metavar="SPEC",
                        help="a bound on the yearly rows every plan must meet, \"[sum(]COLUMN[)] (<=|>=) BOUND [@FROM[:TO]]\" with calendar years, e.g. "
                             "\"net_co2 <= 0 @2040\", \"sum(net_co2) <= 4e8\", \"balance >= 500 @2030:2039\", or on what it builds, "
                             "\"[sum(]built([W*]CLASS {(+|-) [W*]CLASS})[)] (<=|>=) BOUND [@FROM[:TO]]\", e.g. \"built(GasPeaker + GasCombinedCycle) <= 0\", "
                             "\"sum(built(Nuclear)) <= 2\"; repeatable (at most 32, the row constraints first)")


def apply_constraints(engine, args) -> "list[Constraint]":
    """the --constraint specs of `args` parsed (constraint_list: eg_plan_constraint_parse, eg_build_constraint_parse) and set on `engine`;
    returns them (none given: nothing is set)"""
    cs = constraint_list(args.constraint)
    if cs:
        engine.set_constraints(cs)
    return cs
