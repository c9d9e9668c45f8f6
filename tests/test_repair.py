"""CPU: the host side of plan repair (include/eirgrid_hip.h eg_repair_plans) — the definition restated in plain Python from the header
alone (`violation_bytes`, `pick_restated` for one round, `repair_restated` for the loop; the GPU tests import them), the pick rule on
hand-made rounds, Constraint.violation against the struct-level restatement, and the struct and what eg_repair_plans_validate accepts and
refuses through the ABI."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.constraints import Constraint, violation
from eirgrid_amd.engine import Plan, PlanMove, PlanSet, _refine_opts, rank_score
from tests.test_plan_edits import _base
from tests.test_plan_moves import apply_move, round_moves
from tests.test_refine import apply_edit, round_edits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INFEASIBLE = N.EG_EP_OK, N.EG_EP_INFEASIBLE
HAS_V = (OK, INFEASIBLE)      # the statuses of a record that has a violation measure
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- the definition, restated (plain Python floats: one rounding per operation)
def _row_bytes(row):
    """an excess row as a list of 8-byte values, whichever way it came (bytes as tests/test_plan_constraints.py judge gives them, or floats)"""
    return [e if isinstance(e, (bytes, bytearray)) else struct.pack("<d", float(e)) for e in row]


def violation_bytes(row, weights=None):
    """the eight bytes of V for one variant's excess row, by the header's literal order"""
    v = 0.0
    for i, b in enumerate(_row_bytes(row)):
        (e,) = struct.unpack("<d", b)
        w = 1.0 if weights is None else float(weights[i])
        if e != e:
            t = INF
        elif e > 0.0:
            t = w * e
        else:
            t = 0.0
        v = v + t
    return struct.pack("<d", v)


def mask_of(row):
    """the violated mask of a judged record's excess row: bit i iff constraint i is not satisfied (NaN violates)"""
    m = 0
    for i, b in enumerate(_row_bytes(row)):
        if not struct.unpack("<d", b)[0] <= 0.0:
            m |= 1 << i
    return m


def pick_restated(status, metrics, excess, mode, weights=None):
    """One round over the variants' statuses [n], metrics [n][4] and excess rows [n][k], as judged.  Returns a dict: winner (-1: the base
    is no candidate; 0: the base is feasible, or nothing lies strictly below it), n_failed, n_feasible, base_ok, stop ("base_failed",
    "feasible", "stuck" or None: the winner moves the plan), and per variant V (None where the record has none), score and candidacy."""
    n = len(status)
    score = [rank_score(np.ascontiguousarray(metrics[j], dtype=np.float64), mode == 2) for j in range(n)]
    cand = [int(status[j]) in HAS_V and score[j] == score[j] for j in range(n)]
    V = [struct.unpack("<d", violation_bytes(excess[j], weights))[0] if int(status[j]) in HAS_V else None for j in range(n)]
    out = dict(n_failed=sum(not c for c in cand), n_feasible=sum(1 for j in range(n) if cand[j] and V[j] == 0.0), base_ok=int(cand[0]), V=V, score=score, cand=cand)
    if not cand[0]:
        return dict(out, winner=-1, stop="base_failed")
    if V[0] == 0.0:
        return dict(out, winner=0, stop="feasible")
    below = [j for j in range(n) if cand[j] and V[j] < V[0]]      # (inf < inf is false)
    if not below:
        return dict(out, winner=0, stop="stuck")
    return dict(out, winner=min(below, key=lambda j: (V[j], -score[j], j)), stop=None)


def repair_restated(evaluate, base, mode=1, max_rounds=64, replace_with=(), append_with=(), max_shift=0, weights=None):
    """include/eirgrid_hip.h eg_repair_plans for one plan, literally.  `evaluate(plan, edits, moves)` gives the round's variants — the
    edits, then the moves — as judged: (status [n], metrics [n][4], excess rows [n][k]).  Returns (plan, steps, stop, start V, final V);
    a step is (edit or move, variant, n_variants, n_failed, n_feasible, mask, V, score, metrics)."""
    plan, steps, start, final = base, [], NAN, NAN
    while True:
        edits, moves = round_edits(plan, replace_with, append_with), round_moves(plan, max_shift) if max_shift else []
        variants = edits + moves
        assert len(variants) <= N.REFINE_MAX_VARIANTS
        status, metrics, excess = evaluate(plan, edits, moves)
        assert len(status) == len(variants)
        r = pick_restated(status, metrics, excess, mode, weights)
        if not steps and r["base_ok"]:
            start = final = r["V"][0]
        if r["stop"] is not None:
            return plan, steps, r["stop"], start, final
        w = r["winner"]
        v = variants[w]
        steps.append((v, w, len(variants), r["n_failed"], r["n_feasible"], mask_of(excess[w]), r["V"][w], r["score"][w], np.array(metrics[w], np.float64)))
        plan, final = (apply_move(plan, v) if isinstance(v, PlanMove) else apply_edit(plan, v)), r["V"][w]
        if final == 0.0:
            return plan, steps, "feasible", start, final
        if len(steps) == max_rounds:
            return plan, steps, "max_rounds", start, final


# ---------------------------------------------------------------- the pick on hand-made rounds
def _metrics(levels):
    """metrics whose mode-1 score rises strictly with the level (tests/test_crafted_folds.py level_metrics)"""
    level = np.asarray(levels, np.float64)
    return np.stack([500000.0 - level, np.full(level.shape, 0.5), 1e11 - 1e6 * level, np.ones(level.shape)], axis=1)


def _round(V, levels, status=None):
    """a round of one constraint whose excess IS the wanted V (weight 1)"""
    status = [OK if v <= 0 else INFEASIBLE for v in V] if status is None else status      # (NaN violates)
    return np.array(status, np.int32), _metrics(levels), [[v] for v in V]


def test_the_smallest_violation_below_the_base_wins(built):
    r = pick_restated(*_round([5.0, 7.0, 2.0, 3.0, 5.0], [9, 9, 1, 9, 9]), 1)
    assert (r["winner"], r["stop"], r["n_failed"], r["n_feasible"], r["base_ok"]) == (2, None, 0, 0, 1)
    r = pick_restated(*_round([5.0, 0.0, 2.0, 0.0], [9, 1, 9, 1]), 1)
    assert (r["winner"], r["n_feasible"]) == (1, 2)      # V == 0 is the smallest of all


def test_ties_on_v_go_to_the_score_then_to_the_index(built):
    r = pick_restated(*_round([5.0, 2.0, 2.0, 2.0], [0, 3, 8, 4]), 1)
    assert r["winner"] == 2 and r["score"][2] > r["score"][3] > r["score"][1]
    r = pick_restated(*_round([5.0, 2.0, 2.0, 2.0, 2.0], [0, 3, 8, 8, 4]), 1)
    assert r["winner"] == 2 and r["score"][2] == r["score"][3]      # tied on both: the lowest index
    r = pick_restated(*_round([5.0, 2.0, 2.0], [0, 3, 3]), 2)
    assert r["winner"] == 1


def test_a_base_at_infinity_moves_only_to_a_finite_v(built):
    r = pick_restated(*_round([NAN, NAN, INF, 9.0, 1e300], [0, 9, 9, 1, 9]), 1)
    assert r["V"][:3] == [INF, INF, INF] and (r["winner"], r["stop"]) == (3, None)
    r = pick_restated(*_round([NAN, INF, NAN], [0, 9, 9]), 1)
    assert (r["winner"], r["stop"]) == (0, "stuck")      # inf < inf is false


def test_nan_scores_and_failed_records_are_no_candidates(built):
    status, m, ex = _round([5.0, 1.0, 2.0, 3.0], [0, 9, 9, 1])
    m[1, :2] = (-1.0, NAN)      # a NaN score in mode 1
    status[2] = -2              # failed on its own: no V
    ex[2] = [NAN]
    r = pick_restated(status, m, ex, 1)
    assert math.isnan(r["score"][1]) and r["V"][2] is None and (r["winner"], r["n_failed"]) == (3, 2)
    assert pick_restated(status, m, ex, 2)["winner"] in (1, 3)      # (mode 2 does not read the NaN: variant 1 is a candidate there)


def test_nothing_strictly_below_the_base_is_stuck(built):
    r = pick_restated(*_round([5.0, 5.0, 6.0, INF, 5.0], [0, 9, 9, 9, 9]), 1)
    assert (r["winner"], r["stop"], r["n_feasible"]) == (0, "stuck", 0)


def test_a_feasible_base_stops_the_round(built):
    r = pick_restated(*_round([0.0, 0.0, 3.0], [0, 9, 9]), 1)
    assert (r["winner"], r["stop"], r["n_feasible"]) == (0, "feasible", 2)
    r = pick_restated(*_round([-0.0, -4.0, 3.0], [0, 9, 9]), 1)      # slack and -0.0 are no violation
    assert r["stop"] == "feasible" and r["V"][:2] == [0.0, 0.0]


def test_a_base_that_is_no_candidate_fails(built):
    for status0 in (-1, -2, -3):
        status, m, ex = _round([5.0, 1.0], [0, 9])
        status[0] = status0
        r = pick_restated(status, m, ex, 1)
        assert (r["winner"], r["stop"], r["base_ok"], r["n_failed"]) == (-1, "base_failed", 0, 1)
    status, m, ex = _round([5.0, 1.0], [0, 9])
    m[0, :2] = (-1.0, NAN)
    assert pick_restated(status, m, ex, 1)["stop"] == "base_failed"


# ---------------------------------------------------------------- the loop over a toy evaluator
def _toy(weights_of_action):
    """an evaluator whose one constraint's excess is the sum of its best_actions' weights minus 10: deleting entries repairs the plan"""
    def evaluate(plan, edits, moves):
        rows = []
        for v in edits + moves:
            p = apply_move(plan, v) if isinstance(v, PlanMove) else apply_edit(plan, v)
            rows.append(float(sum(weights_of_action[a] for l in p.best_actions for a in l)) - 10.0)
        status = np.array([INFEASIBLE if e > 0 else OK for e in rows], np.int32)
        return status, _metrics(np.arange(len(rows)) % 7), [[e] for e in rows]
    return evaluate


def _toy_plan(actions):
    empty = [[] for _ in range(26)]
    return Plan([list(actions)] + empty[1:], empty)


def test_the_loop_descends_to_feasible_and_reports_every_stop(built):
    w = {1: 4.0, 2: 5.0, 3: 6.0}
    plan, steps, stop, start, final = repair_restated(_toy(w), _toy_plan([1, 2, 3, 3]), 1, 8)
    assert stop == "feasible" and (start, final) == (11.0, 0.0) and [s[6] for s in steps] == [5.0, 0.0]      # 21 - 10, minus a 6, minus a 6
    assert [s[0].kind for s in steps] == ["delete", "delete"] and plan == _toy_plan([1, 2]) and steps[0][1] == 4      # (tied on V with variant 3: the larger score)
    assert repair_restated(_toy(w), _toy_plan([1, 2, 3, 3]), 1, 1)[2:] == ("max_rounds", 11.0, 5.0)
    assert repair_restated(_toy(w), _toy_plan([1, 2]), 1, 8)[1:] == ([], "feasible", 0.0, 0.0)
    n_of = lambda edits, moves: len(edits) + len(moves)
    constant = lambda plan, edits, moves: (np.full(n_of(edits, moves), INFEASIBLE, np.int32), _metrics(np.zeros(n_of(edits, moves))), [[11.0]] * n_of(edits, moves))
    assert repair_restated(constant, _toy_plan([1]), 1, 8)[1:] == ([], "stuck", 11.0, 11.0)
    failing = lambda plan, edits, moves: (np.full(n_of(edits, moves), -2, np.int32), _metrics(np.zeros(n_of(edits, moves))), [[NAN]] * n_of(edits, moves))
    plan, steps, stop, start, final = repair_restated(failing, _toy_plan([1]), 1, 8)
    assert (steps, stop) == ([], "base_failed") and math.isnan(start) and math.isnan(final)
    moved = repair_restated(_toy(w), _toy_plan([1, 2, 3, 3]), 1, 8, max_shift=1)      # moves keep the sum: the deletes win as before
    assert moved[2] == "feasible" and [s[2] for s in moved[1]] == [5 + 4, 4 + 3]


# ---------------------------------------------------------------- Constraint.violation against the struct-level restatement
CASES = [
    # (excess row, weights, the V it must give)
    ([-0.0], None, 0.0),
    ([0.0], None, 0.0),                                   # a value on its bound: excess 0, satisfied
    ([-3.5], None, 0.0),                                  # slack does not offset anything
    ([-3.5, 2.0], None, 2.0),
    ([INF], None, INF),
    ([-INF], None, 0.0),
    ([NAN], None, INF),
    ([NAN, -1.0], [1e-300, 5.0], INF),                    # a NaN excess is +inf whatever its weight
    ([2.0], [0.5], 1.0),
    ([0.1, 0.2, 0.3], None, (0.1 + 0.2) + 0.3),           # constraint order: not 0.1 + (0.2 + 0.3)
    ([0.3, 0.2, 0.1], None, (0.3 + 0.2) + 0.1),
    ([1.0, 1.0, 1.0], [1e16, 1.0, 1.0], 1e16),            # every addition rounds: the ones are lost behind 1e16
    ([1.0, 1.0, 1.0], [1.0, 1.0, 1e16], 1e16 + 2.0),      # ... and kept in front of it
    ([2.0 ** -53, 1 + 2.0 ** -30], [1.0, 1 + 2.0 ** -30], 1 + 2.0 ** -29),      # the product rounds once, then the sum: a fused multiply-add gives one ulp more
    ([1e308, 1e308], [2.0, 1.0], INF),                    # a product that overflows
    ([5e-324], [0.25], 0.0),                              # ... and one that underflows to zero: the rounds go by V
]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_violation_is_the_definition_on_crafted_rows(k):
    row, weights, want = CASES[k]
    got = Constraint.violation(row, weights)
    assert struct.pack("<d", got) == violation_bytes(row, weights) == struct.pack("<d", want), (row, weights, got, want)
    assert violation(np.array(row), weights) == got or got != got


def test_the_rounding_order_is_visible():
    assert (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)                                    # (what the two sum cases above rest on)
    from fractions import Fraction
    x = 1 + 2.0 ** -30
    assert float(Fraction(2.0 ** -53) + Fraction(x) * Fraction(x)) == 1 + 2.0 ** -29 + 2.0 ** -52 != 2.0 ** -53 + x * x == 1 + 2.0 ** -29      # fused != unfused
    assert Constraint.violation([1.0] * 32, [1e16] + [1.0] * 31) == 1e16 and Constraint.violation([1.0] * 32, [1.0] * 31 + [1e16]) == 1e16 + 32.0


@pytest.mark.parametrize("k", [1, 32])
def test_violation_agrees_with_the_second_loop_on_seeded_rows(k):
    rng = np.random.default_rng(100 + k)
    special = np.array([NAN, INF, -INF, -0.0, 0.0, 1e16, 1.0, -1.0])
    for trial in range(300):
        row = rng.normal(0.0, 10.0, k).round(1)
        hit = rng.random(k) < 0.15
        row[hit] = rng.choice(special, int(hit.sum()))
        weights = None if trial % 3 == 0 else (10.0 ** rng.integers(-3, 17, k)) * rng.choice([1.0, 3.0, 0.1], k)
        got = Constraint.violation(row, weights)
        assert struct.pack("<d", got) == violation_bytes(row, weights), (trial, row, weights)
        assert (got == 0.0) == (mask_of(row) == 0) and not math.isnan(got)


def test_violation_refuses_weights_it_cannot_mean():
    for bad in ([0.0], [-1.0], [INF], [NAN]):
        with pytest.raises(ValueError, match="finite and > 0"):
            Constraint.violation([1.0], bad)
    with pytest.raises(ValueError, match="2 weights for 1 constraints"):
        Constraint.violation([1.0], [1.0, 2.0])


# ---------------------------------------------------------------- struct and ABI
def test_struct_constants_header_and_exports_agree(built):
    f = N.EgRepairStep
    assert C.sizeof(f) == 96
    assert (f.is_move.offset, f.edit.offset, f.move.offset, f.variant.offset, f.n_variants.offset, f.n_failed.offset, f.n_feasible.offset, f.violated.offset,
            f.violation.offset, f.score.offset, f.metrics.offset) == (0, 4, 16, 28, 32, 36, 40, 44, 48, 56, 64)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert re.search(r"typedef struct \{ int32_t is_move; eg_plan_edit edit; eg_plan_move move; int32_t variant, n_variants, n_failed, n_feasible;\s+"
                     r"uint32_t violated; double violation, score, metrics\[4\]; \} eg_repair_step;", header)
    for name, value, mine in (("EG_REPAIR_FEASIBLE", 0, N.REPAIR_FEASIBLE), ("EG_REPAIR_MAX_ROUNDS", 1, N.REPAIR_MAX_ROUNDS),
                              ("EG_REPAIR_BASE_FAILED", 2, N.REPAIR_BASE_FAILED), ("EG_REPAIR_STUCK", 3, N.REPAIR_STUCK),
                              ("EG_DEBUG_REPAIR_ENTRY_BYTES", 112, C.sizeof(N.EgDebugRepairEntry))):
        assert re.search(rf"#define {name} {value}\b", header) and mine == value, name
    L = N.lib()
    for name in ("eg_repair_plans_validate", "eg_repair_plans", "eg_debug_repair_pick_many"):
        assert name in N.EXPORTS and hasattr(L, name), name
        assert len(re.findall(rf"^int32_t {name}\(", header, flags=re.M)) == 1, name
    from eirgrid_amd.engine import REPAIR_STOP
    assert REPAIR_STOP == ("feasible", "max_rounds", "base_failed", "stuck")


def _validate(plans, weights=None, k=1, max_shift=None, **kw):
    L = N.lib()
    args = dict(mode=1, max_rounds=4, replace_with=None, append_with=None); args.update(kw)
    ro, keep = _refine_opts(**args)
    ps = PlanSet(plans)
    mo = None if max_shift is None else N.EgRefineMoveOpts(max_shift)
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    rc = L.eg_repair_plans_validate(C.byref(ps.s), C.byref(ro), None if mo is None else C.byref(mo), None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)), k)
    return rc, L.eg_last_error().decode()


def test_validate_accepts_what_the_definition_allows(built):
    for kw in (dict(), dict(k=32, weights=[0.5] * 32), dict(max_shift=0), dict(max_shift=25, mode=2), dict(weights=[1e-300]), dict(weights=[1e300]),
               dict(replace_with=[0, 60], append_with=[12], max_rounds=10**6), dict(k=3, weights=[1.0, 2.0, 3.0], max_shift=1)):
        rc, msg = _validate([_base(), _base()], **kw)
        assert rc == N.EG_OK, (kw, msg)


@pytest.mark.parametrize("kw, expect", [
    (dict(k=0), "no plan constraints are set"),
    (dict(k=-1), "no plan constraints are set"),
    (dict(k=33), "k = 33 constraints (at most 32)"),
    (dict(k=2, weights=[1.0, 0.0]), "weights[1] = 0.000000 (finite and > 0)"),
    (dict(k=2, weights=[-2.0, 1.0]), "weights[0] = -2.000000 (finite and > 0)"),
    (dict(k=3, weights=[1.0, 1.0, INF]), "weights[2] = inf (finite and > 0)"),
    (dict(weights=[NAN]), "weights[0] = nan (finite and > 0)"),
    (dict(max_shift=26), "max_shift = 26 (0..25 years; 0: no moves)"),
    (dict(max_shift=-1), "max_shift = -1 ("),
    (dict(mode=0), "mode 0 (1: optimization_mode None, 2: cost_only)"),
    (dict(max_rounds=0), "max_rounds = 0 (at least 1)"),
    (dict(replace_with=[3, 61]), "replace_with[1]: action 61 >= 61"),
])
def test_validate_names_the_cause(built, kw, expect):
    rc, msg = _validate([_base()], **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_repair_plans_validate: ") and expect in msg, msg


def test_validate_refuses_bad_sets_and_the_entry_points_their_null_arguments(built):
    L = N.lib()
    rc, msg = _validate([_base()] * (N.REFINE_MAX_PLANS + 1))
    assert rc == N.EG_ERR_BAD_ARG and "eg_repair_plans_validate: the set holds 257 plans (at most 256)" in msg, msg
    assert _validate([_base()] * N.REFINE_MAX_PLANS)[0] == N.EG_OK
    ro, keep = _refine_opts(1, 4, None, None)
    assert L.eg_repair_plans_validate(None, C.byref(ro), None, None, 1) == N.EG_ERR_BAD_ARG and "NULL plan set" in L.eg_last_error().decode()
    bad = _base(); bad.best_actions[0][1] = 61
    rc, msg = _validate([_base(), bad])
    assert rc == N.EG_ERR_BAD_ARG and "best_actions year 2025 entry 1: 61 >= 61" in msg, msg
    big = Plan([[60] * 160 for _ in range(25)] + [[]], [[24] for _ in range(26)])      # 1 + 4 000 + 26 variants; every entry moves two ways
    rc, msg = _validate([_base(), big], max_shift=2)
    assert rc == N.EG_ERR_BAD_ARG and re.search(r"plan 1: round 0 enumerates \d+ variants \(at most 16384\)", msg), msg
    assert _validate([_base(), big], max_shift=1)[0] == N.EG_OK
    assert L.eg_repair_plans(None, None, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_repair_plans: bad argument" in L.eg_last_error().decode()
    assert L.eg_debug_repair_pick_many(None, 1, None, None, None, 1, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_debug_repair_pick_many: bad argument" in L.eg_last_error().decode()
