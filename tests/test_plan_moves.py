"""CPU: the host side of plan moves (include/eirgrid_hip.h eg_evaluate_plan_moves, eg_refine_plans_moves) — the struct layouts, what the
two validators accept and refuse, PlanMove.apply against a restatement written out here (`apply_move`, which the GPU tests import), the
order of a round's move variants, and which entry point Engine.refine_plans binds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import Engine, Plan, PlanMove, PlanSet, _move_array, _refine_opts, refine_moves
from tests.test_plan_edits import _base
from tests.test_plans import _empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one plan, "edit optimum": where the deletes of eg_refine_plans (mode 1, no replaces or appends) leave the 67-action plan of
# tests/test_refine.py short_policy — no one-entry edit improves it, a move does
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_move_base.jsonl")


def apply_move(plan, m):
    """Move m applied to a copy of `plan`, written out once more (not PlanMove.apply: the tests' own restatement): the entry is taken
    out, then put back in front of entry to_pos of the target year's list as it stands after the removal."""
    lists = ([list(l) for l in plan.best_actions], [list(l) for l in plan.best_deficit_actions])
    which = lists[m.list]
    entry = which[m.year][m.pos]
    which[m.year] = which[m.year][:m.pos] + which[m.year][m.pos + 1:]
    which[m.to_year] = which[m.to_year][:m.to_pos] + [entry] + which[m.to_year][m.to_pos:]
    return Plan(lists[0], lists[1], plan.name)


def round_moves(plan, max_shift):
    """The move variants of a round, written out once more: per best_actions entry in (year, position) order the shifts -1, +1, -2, +2,
    ... that stay inside the 26 years, the entry put behind the target year's last one."""
    out = []
    for y in range(26):
        for i in range(len(plan.best_actions[y])):
            for s in range(1, max_shift + 1):
                if y - s >= 0:
                    out.append(PlanMove(0, y, i, y - s, len(plan.best_actions[y - s])))
                if y + s <= 25:
                    out.append(PlanMove(0, y, i, y + s, len(plan.best_actions[y + s])))
    return out


def _validate(base_set, moves, n=None):
    L = N.lib()
    arr, k = _move_array(moves)
    rc = L.eg_plan_moves_validate(C.byref(base_set.s) if base_set is not None else None, arr, k if n is None else n)
    return rc, L.eg_last_error().decode()


# ---------------------------------------------------------------- layouts
def test_struct_layouts_are_the_headers(built):
    assert C.sizeof(N.EgPlanMove) == 12
    assert (N.EgPlanMove.list.offset, N.EgPlanMove.to_year.offset, N.EgPlanMove.year.offset, N.EgPlanMove.pos.offset, N.EgPlanMove.to_pos.offset) == (0, 1, 2, 4, 8)
    assert C.sizeof(N.EgRefineMoveOpts) == 4 and C.sizeof(N.EgRefineMoveStep) == 80
    S = N.EgRefineMoveStep
    assert (S.is_move.offset, S.edit.offset, S.move.offset, S.variant.offset, S.n_variants.offset, S.n_failed.offset, S.score.offset, S.metrics.offset) == \
        (0, 4, 16, 28, 32, 36, 40, 48)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert "typedef struct { uint8_t list, to_year; uint16_t year; uint32_t pos, to_pos; } eg_plan_move;" in header
    assert "typedef struct { int32_t max_shift; } eg_refine_move_opts;" in header
    assert re.search(r"typedef struct \{ int32_t is_move; eg_plan_edit edit; eg_plan_move move; int32_t variant, n_variants, n_failed;\s+double score; "
                     r"double metrics\[4\]; \} eg_refine_move_step;", header)
    # the library's side of sizeof(eg_plan_move): it steps through an array of two moves as ctypes laid them out, and names the second
    rc, msg = _validate(PlanSet([_base()]), [PlanMove(0, 0, 0, 25, 2), PlanMove(1, 6, 1, 6, 2)])
    assert rc == N.EG_ERR_BAD_ARG and "move 1: to_pos 2 outside best_deficit_actions year 2031 (1 entries after the removal)" in msg, msg


# ---------------------------------------------------------------- eg_plan_moves_validate
def test_validate_accepts_every_well_formed_move(built):
    base = _base()
    moves = []
    for which, lists in enumerate((base.best_actions, base.best_deficit_actions)):
        for y, l in enumerate(lists):
            for i in range(len(l)):
                for ty in range(26):
                    moves += [PlanMove(which, y, i, ty, tp) for tp in range(len(lists[ty]) - (ty == y) + 1)]
    assert PlanMove(0, 0, 1, 0, 1) in moves and PlanMove(0, 6, 0, 6, 0) in moves and PlanMove(0, 0, 0, 3, 0) in moves      # identities, an empty target
    rc, msg = _validate(PlanSet([base]), moves)
    assert rc == N.EG_OK, msg
    full = [[60] * 157 for _ in range(26)]
    full[0] += [60] * (4096 - 26 * 157)
    rc, msg = _validate(PlanSet([Plan(full, full)]), [PlanMove(w, 0, 0, 25, 157) for w in (0, 1)])      # a full list still takes a move
    assert rc == N.EG_OK, msg


@pytest.mark.parametrize("move, expect", [
    (PlanMove(0, 0, 3, 1, 0), "move 2: pos 3 outside best_actions year 2025 (3 entries): 0..len-1"),
    (PlanMove(1, 6, 2, 0, 0), "move 2: pos 2 outside best_deficit_actions year 2031 (2 entries): 0..len-1"),
    (PlanMove(0, 3, 0, 4, 0), "move 2: pos 0 outside best_actions year 2028 (0 entries): 0..len-1"),
    (PlanMove(0, 0, 0, 6, 2), "move 2: to_pos 2 outside best_actions year 2031 (1 entries after the removal)"),
    (PlanMove(0, 25, 0, 6, 4), "move 2: to_pos 4 outside best_actions year 2031 (1 entries after the removal)"),
    (PlanMove(0, 0, 1, 0, 3), "move 2: to_pos 3 outside best_actions year 2025 (2 entries after the removal)"),
    (PlanMove(0, 6, 0, 6, 1), "move 2: to_pos 1 outside best_actions year 2031 (0 entries after the removal)"),
    (PlanMove(1, 0, 0, 3, 1), "move 2: to_pos 1 outside best_deficit_actions year 2028 (0 entries after the removal)"),
    (PlanMove(0, 26, 0, 0, 0), "move 2: year 26 (a year index 0..25)"),
    (PlanMove(0, 0, 0, 26, 0), "move 2: to_year 26 (a year index 0..25)"),
    (PlanMove(2, 0, 0, 1, 0), "move 2: list 2 (0 best_actions, 1 best_deficit_actions)"),
])
def test_validate_names_the_move_and_the_field(built, move, expect):
    rc, msg = _validate(PlanSet([_base()]), [PlanMove(0, 0, 0, 0, 0), PlanMove(0, 0, 0, 25, 2), move])
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_plan_moves_validate: ") and expect in msg, msg


def test_validate_refuses_empty_batches_null_moves_and_bad_bases(built):
    ps = PlanSet([_base()])
    L = N.lib()
    rc, msg = _validate(ps, [], 0)
    assert rc == N.EG_ERR_BAD_ARG and "n_moves = 0 (at least 1)" in msg, msg
    rc, msg = _validate(ps, [PlanMove()], -3)
    assert rc == N.EG_ERR_BAD_ARG and "n_moves = -3 (at least 1)" in msg, msg
    assert L.eg_plan_moves_validate(C.byref(ps.s), None, 1) == N.EG_ERR_BAD_ARG and "eg_plan_moves_validate: NULL moves" in L.eg_last_error().decode()
    rc, msg = _validate(PlanSet([_base(), _base()]), [PlanMove()])
    assert rc == N.EG_ERR_BAD_ARG and "the base holds 2 plans (exactly 1)" in msg, msg
    rc, msg = _validate(None, [PlanMove()])
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    bad = _base(); bad.best_actions[0][1] = 61
    rc, msg = _validate(PlanSet([bad]), [PlanMove()])
    assert rc == N.EG_ERR_BAD_ARG and "best_actions year 2025 entry 1: 61 >= 61" in msg, msg


def test_evaluate_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_evaluate_plan_moves(None, None, None, None, None, 1, 0, 0, 1, None) == N.EG_ERR_BAD_ARG
    assert "eg_evaluate_plan_moves: bad argument" in L.eg_last_error().decode()
    assert L.eg_refine_plans_moves(None, None, None, None, None, None, 0, 0, None, None, None, None, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_refine_plans_moves: bad argument" in L.eg_last_error().decode()


# ---------------------------------------------------------------- eg_refine_plans_moves_validate
def _validate_refine(plans, max_shift=1, null_moves=False, **kw):
    L = N.lib()
    args = dict(mode=1, max_rounds=4, replace_with=None, append_with=None); args.update(kw)
    ro, keep = _refine_opts(**args)
    ps = PlanSet(plans) if plans is not None else None
    mo = N.EgRefineMoveOpts(max_shift)
    rc = L.eg_refine_plans_moves_validate(C.byref(ps.s) if ps is not None else None, C.byref(ro), None if null_moves else C.byref(mo))
    return rc, L.eg_last_error().decode()


def test_refine_validate_accepts_and_refuses(built):
    base = _base()
    for shift in (0, 1, 25):
        rc, msg = _validate_refine([base, base], shift, replace_with=[12], append_with=[3])
        assert rc == N.EG_OK, (shift, msg)
    for shift, expect in ((-1, "max_shift = -1 (0..25 years; 0: no moves)"), (26, "max_shift = 26 (0..25 years; 0: no moves)")):
        rc, msg = _validate_refine([base], shift)
        assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_refine_plans_moves_validate: ") and expect in msg, msg
    rc, msg = _validate_refine([base], null_moves=True)
    assert rc == N.EG_ERR_BAD_ARG and "eg_refine_plans_moves_validate: NULL move options" in msg, msg
    # eg_refine_plans_validate's refusals, under this validator's name
    rc, msg = _validate_refine([base], mode=3)
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_refine_plans_moves_validate: mode 3 ("), msg
    rc, msg = _validate_refine([base], max_rounds=0)
    assert rc == N.EG_ERR_BAD_ARG and "max_rounds = 0 (at least 1)" in msg, msg
    rc, msg = _validate_refine([base], replace_with=[61])
    assert rc == N.EG_ERR_BAD_ARG and "replace_with[0]: action 61 >= 61" in msg, msg
    rc, msg = _validate_refine([base] * 257)
    assert rc == N.EG_ERR_BAD_ARG and "the set holds 257 plans (at most 256)" in msg, msg
    rc, msg = _validate_refine(None)
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    L = N.lib()
    ps = PlanSet([base]); mo = N.EgRefineMoveOpts(1)
    assert L.eg_refine_plans_moves_validate(C.byref(ps.s), None, C.byref(mo)) == N.EG_ERR_BAD_ARG and "NULL options" in L.eg_last_error().decode()


def test_refine_validate_counts_edits_and_moves_together(built):
    # 25 years of 160 entries, the last year empty: 1 + 4 000 + 26 deletes; a shift of 2 adds 4 moves per entry, but years 0, 1 and 24 lose
    # directions (year 25 holds nothing): 4 000 * 4 - 160 * (2 + 1 + 1) = 15 360 moves
    big = Plan([[60] * 160 for _ in range(25)] + [[]], [[24] for _ in range(26)])
    assert len(refine_moves(big, 2)) == 15360 and len(refine_moves(big, 1)) == 2 * 4000 - 160
    rc, msg = _validate_refine([_base(), big], 2)
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_refine_plans_moves_validate: plan 1: round 0 enumerates 19387 variants (at most 16384)", msg
    assert _validate_refine([_base(), big], 1)[0] == N.EG_OK      # 4 027 + 7 840
    rc, msg = _validate_refine([big], 1, replace_with=[0, 3])      # 4 027 + 8 000 + 7 840
    assert rc == N.EG_ERR_BAD_ARG and "plan 0: round 0 enumerates 19867 variants (at most 16384)" in msg, msg
    assert _validate_refine([big], 0, replace_with=[0, 3, 6])[0] == N.EG_OK      # no moves: eg_refine_plans_validate's count


# ---------------------------------------------------------------- PlanMove.apply
def _plan():
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[6] = [3]; run[7] = [9, 10, 11, 12]; run[25] = [45, 0]
    dfc[0] = [24]; dfc[6] = [24, 60, 21]
    return Plan(run, dfc, "p")


@pytest.mark.parametrize("move, which, years", [
    (PlanMove(0, 0, 1, 7, 2), 0, {0: [5, 60], 7: [9, 10, 12, 11, 12]}),        # a later year, into the middle
    (PlanMove(0, 0, 0, 25, 2), 0, {0: [12, 60], 25: [45, 0, 5]}),              # ... behind the last entry
    (PlanMove(0, 25, 1, 6, 0), 0, {25: [45], 6: [0, 3]}),                      # an earlier year, in front of the first entry
    (PlanMove(1, 6, 2, 0, 1), 1, {6: [24, 60], 0: [24, 21]}),                  # ... on the deficit list
    (PlanMove(0, 7, 0, 7, 3), 0, {7: [10, 11, 12, 9]}),                        # the same year, forward: to_pos counts after the removal
    (PlanMove(0, 7, 1, 7, 2), 0, {7: [9, 11, 10, 12]}),
    (PlanMove(0, 7, 3, 7, 0), 0, {7: [12, 9, 10, 11]}),                        # the same year, backward
    (PlanMove(0, 7, 2, 7, 1), 0, {7: [9, 11, 10, 12]}),
    (PlanMove(0, 7, 2, 7, 2), 0, {}),                                          # the identity
    (PlanMove(0, 6, 0, 6, 0), 0, {}),                                          # ... of a year's only entry
    (PlanMove(0, 6, 0, 3, 0), 0, {6: [], 3: [3]}),                             # an empty target year; the source year is left empty
    (PlanMove(1, 0, 0, 25, 0), 1, {0: [], 25: [24]}),
])
def test_apply_is_the_restatement(move, which, years):
    base = _plan()
    got = move.apply(base)
    assert got == apply_move(base, move) and got.name == "p"
    want = ([list(l) for l in base.best_actions], [list(l) for l in base.best_deficit_actions])
    for y, l in years.items():
        want[which][y] = l
    assert (got.best_actions, got.best_deficit_actions) == (want[0], want[1])
    assert base == _plan()      # (a copy: the base is left alone)
    assert len(got) == len(base)


def test_apply_on_random_moves_is_the_restatement():
    rng = np.random.default_rng(12)
    for _ in range(200):
        plan = Plan([[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 5)))] for _ in range(26)],
                    [[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 3)))] for _ in range(26)])
        which = int(rng.integers(0, 2))
        lists = (plan.best_actions, plan.best_deficit_actions)[which]
        years = [y for y in range(26) if lists[y]]
        if not years:
            continue
        y = int(rng.choice(years)); ty = int(rng.integers(0, 26))
        m = PlanMove(which, y, int(rng.integers(0, len(lists[y]))), ty, int(rng.integers(0, len(lists[ty]) - (ty == y) + 1)))
        got = m.apply(plan)
        assert got == apply_move(plan, m), m
        assert sorted(a for l in got.best_actions for a in l) == sorted(a for l in plan.best_actions for a in l)
        ps = PlanSet([plan])
        assert N.lib().eg_plan_moves_validate(C.byref(ps.s), _move_array([m])[0], 1) == N.EG_OK


# ---------------------------------------------------------------- the order of a round's moves
def test_move_order_and_count_follow_the_formula():
    base = _plan()      # entries in years 0 (3), 6 (1), 7 (4) and 25 (2)
    assert refine_moves(base, 0) == []
    one = refine_moves(base, 1)
    assert one[:3] == [PlanMove(0, 0, 0, 1, 0), PlanMove(0, 0, 1, 1, 0), PlanMove(0, 0, 2, 1, 0)]      # year 0: no year before it
    assert one[3:5] == [PlanMove(0, 6, 0, 5, 0), PlanMove(0, 6, 0, 7, 4)]                             # -1 before +1; behind year 7's four entries
    assert one[5:7] == [PlanMove(0, 7, 0, 6, 1), PlanMove(0, 7, 0, 8, 0)]
    assert one[-2:] == [PlanMove(0, 25, 0, 24, 0), PlanMove(0, 25, 1, 24, 0)]                         # year 25: no year behind it
    three = refine_moves(base, 3)
    assert three[:3] == [PlanMove(0, 0, 0, 1, 0), PlanMove(0, 0, 0, 2, 0), PlanMove(0, 0, 0, 3, 0)]
    assert three[9:15] == [PlanMove(0, 6, 0, 5, 0), PlanMove(0, 6, 0, 7, 4), PlanMove(0, 6, 0, 4, 0), PlanMove(0, 6, 0, 8, 0), PlanMove(0, 6, 0, 3, 0), PlanMove(0, 6, 0, 9, 0)]
    assert [m.to_year for m in three[-3:]] == [24, 23, 22] and all(m.pos == 1 and m.year == 25 for m in three[-3:])
    for shift in (1, 2, 3, 25):
        moves = refine_moves(base, shift)
        assert moves == round_moves(base, shift)
        count = sum(len(l) * (min(shift, y) + min(shift, 25 - y)) for y, l in enumerate(base.best_actions))
        assert len(moves) == count == len(set(moves)), shift
        assert all(m.list == 0 and m.to_year != m.year and m.to_pos == len(base.best_actions[m.to_year]) for m in moves)
        assert [(m.year, m.pos) for m in moves] == sorted((m.year, m.pos) for m in moves)      # entries in (year, position) order
        ps = PlanSet([base])
        assert N.lib().eg_plan_moves_validate(C.byref(ps.s), _move_array(moves)[0], len(moves)) == N.EG_OK
    assert len(refine_moves(base, 25)) == 10 * 25      # every entry to every other year
    assert refine_moves(Plan(_empty(), base.best_deficit_actions), 3) == []      # deficit entries are not moved


# ---------------------------------------------------------------- which entry point refine_plans binds
class _Recorder:
    """stands in for the library: records the entry point Engine.refine_plans calls, and fails the call"""

    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        def call(*args):
            self.called.append((name, len(args)))
            return N.EG_ERR_BAD_ARG
        return call


@pytest.mark.parametrize("kw, entry, n_args", [({}, "eg_refine_plans", 13), ({"max_shift": 0}, "eg_refine_plans", 13), ({"max_shift": 2}, "eg_refine_plans_moves", 14)])
def test_refine_plans_binds_the_old_entry_point_without_a_shift(built, monkeypatch, kw, entry, n_args):
    from eirgrid_amd.engine import ActionWeights
    pol = ActionWeights()
    rec = _Recorder()
    eng = Engine.__new__(Engine)      # (no device: the call is intercepted before it reaches one)
    eng.h = None
    real = N.lib()
    monkeypatch.setattr(N, "lib", lambda: rec)

    def check(rc, what=""):      # (the policy's snapshot passes; the refinement call reports which one it was)
        if what.startswith("eg_refine"):
            raise RuntimeError(what)
    monkeypatch.setattr(N, "check", check)
    try:
        with pytest.raises(RuntimeError, match=f"^{entry}$"):
            eng.refine_plans(pol, [_base()], 1, **kw)
    finally:
        monkeypatch.undo()
    assert [c for c in rec.called if c[0].startswith("eg_refine")] == [(entry, n_args)]
    assert N.lib() is real


# ---------------------------------------------------------------- the fixture: a plan only a move improves (the tabled oracle)
FIXTURE_STEPS = {1: PlanMove(0, 6, 0, 5, 2), 3: PlanMove(0, 6, 0, 3, 2)}      # max_shift: the first step of the fixture's plan


def test_the_fixture_is_an_edit_optimum_that_a_move_improves(world):
    from eirgrid_amd.engine import rank_score
    from tests.test_refine import OracleEvaluator, apply_edit, refine_restated, round_edits, short_policy
    pol = short_policy()
    ev = OracleEvaluator(world, pol)
    base = Plan.load(FIXTURE)[0]
    assert base.name == "edit optimum" and len(base) == 62
    plan, steps, stop, start, ties = refine_restated(ev, Plan.from_policy(pol), 1, 64)
    assert (stop, len(steps)) == ("local_optimum", 5) and plan == base      # where the fixture comes from

    def score(p):
        status, metrics = ev.one(p)
        assert status == 0
        return rank_score(metrics)
    edits = round_edits(base)
    scores = [score(apply_edit(base, e)) for e in edits]
    assert len(edits) == 167 and max(scores) == scores[0]      # no edit is better than the plan itself (many tie with it: the base wins those)
    for shift, first in FIXTURE_STEPS.items():
        moves = round_moves(base, shift)
        moved = [score(apply_move(base, m)) for m in moves]
        assert len(moves) == {1: 118, 3: 338}[shift]
        assert max(moved) > scores[0] and moved.count(max(moved)) == 1 and moves[moved.index(max(moved))] == first, shift
