"""GPU: refinement with moves (include/eirgrid_hip.h eg_refine_plans_moves; csrc/eg_refine.cpp, csrc/eg_plan_moves.h).  With max_shift == 0
the call is eg_refine_plans field for field; with moves it is compared, plan by plan, with the definition written out here as a greedy
loop over Engine.evaluate_plan_edits and Engine.evaluate_plan_moves; and on the base of tests/golden/plan_move_base.jsonl — a plan no
one-entry edit improves, found with the tabled oracle (tests/test_plan_moves.py checks that on the CPU) — a move must be the step taken."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, BatchResult, Plan, PlanEdit, PlanMove, PlanSet, _refine_opts, rank_score
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plan_edits import _sized_plan
from tests.test_plan_moves import FIXTURE, FIXTURE_STEPS, apply_move, round_moves
from tests.test_refine import SEED, apply_edit, round_edits, short_policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
LAUNCH = "EIRGRID_REFINE_LAUNCH_VARIANTS"
METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")


def bits(x):
    return np.float64(x).tobytes()


def _plans():
    """(the policy the calls run under, four short plans: the fixture's edit optimum, the short base it was refined from, a plan of
    another shape, and the short base once more under another name)"""
    pol = short_policy()
    short = Plan.from_policy(pol, "short")
    fixture = Plan.load(FIXTURE)[0]
    assert fixture.name == "edit optimum" and len(fixture) == 62 and len(short) == 67
    return pol, [fixture, short, _sized_plan(40), Plan(short.best_actions, short.best_deficit_actions, "short again")]


def refine_restated(eng, pol, base, seed, index, mode, max_rounds, max_shift, replace_with=(), append_with=()):
    """include/eirgrid_hip.h eg_refine_plans_moves for one plan, literally: per round the edits of eg_refine_plans, then the moves, all at
    the same global index; the candidate with the largest score wins, ties to the lowest variant — the base first, an edit before a move.
    Returns (refined plan, steps, stop reason, start score); a step is (edit or move, variant, n_variants, n_failed, score, metrics)."""
    plan, steps, start = base, [], float("nan")
    while True:
        edits = round_edits(plan, replace_with, append_with)
        moves = round_moves(plan, max_shift)
        variants = edits + moves
        assert len(variants) <= N.REFINE_MAX_VARIANTS
        res = [eng.evaluate_plan_edits(pol, plan, edits, seed, index, same_index=True)]
        if moves:
            res.append(eng.evaluate_plan_moves(pol, plan, moves, seed, index, same_index=True))
        status = np.concatenate([res[0].status[:len(edits)]] + ([res[1].status[:len(moves)]] if moves else []))
        metrics = np.concatenate([res[0].metrics[:len(edits)]] + ([res[1].metrics[:len(moves)]] if moves else []))
        score = np.array([rank_score(np.ascontiguousarray(metrics[j]), mode == 2) if status[j] == N.EG_EP_OK else np.nan for j in range(len(variants))])
        cand = (status == N.EG_EP_OK) & ~np.isnan(score)
        if not steps and cand[0]:
            start = float(score[0])
        if not cand[0]:
            return plan, steps, "base_failed", start
        top = np.nanmax(np.where(cand, score, np.nan))
        winner = int(np.flatnonzero(cand & (score == top))[0])
        if winner == 0:
            return plan, steps, "local_optimum", start
        v = variants[winner]
        steps.append((v, winner, len(variants), int((~cand).sum()), float(score[winner]), metrics[winner].copy()))
        plan = apply_move(plan, v) if isinstance(v, PlanMove) else apply_edit(plan, v)
        if len(steps) == max_rounds:
            return plan, steps, "max_rounds", start


def _assert_is_the_restatement(got, want, what):
    plan, steps, stop, start, rec = got
    wplan, wsteps, wstop, wstart = want
    assert stop == wstop and len(steps) == len(wsteps), (what, stop, wstop, len(steps), len(wsteps))
    assert bits(start) == bits(wstart) or (np.isnan(start) and np.isnan(wstart)), (what, start, wstart)
    for r, (s, w) in enumerate(zip(steps, wsteps)):
        assert type(s.edit) is type(w[0]) and s.edit == w[0], (what, r, s.edit, w[0])
        assert (s.variant, s.n_variants, s.n_failed) == w[1:4], (what, r, s, w)
        assert bits(s.score) == bits(w[4]) and s.metrics.tobytes() == np.ascontiguousarray(w[5]).tobytes(), (what, r, s, w)
    assert plan == wplan, what
    if rec is not None and steps and stop == "max_rounds":      # the refined plan's record is the last winner's
        assert rec.metrics[0].tobytes() == steps[-1].metrics.tobytes() and rec.status[0] == 0, what


def _raw(eng, pol, plans, seed, index, mode, max_rounds, max_shift, replace_with=None, append_with=None):
    """eg_refine_plans_moves as the library exports it: (refined plans, the step structs [n][max_rounds], n_steps, stop, start, out)"""
    ps = PlanSet(plans)
    n = len(plans)
    ro, keep = _refine_opts(mode, max_rounds, replace_with, append_with)
    mo = N.EgRefineMoveOpts(max_shift)
    steps = (N.EgRefineMoveStep * (n * max_rounds))()
    n_steps = np.zeros(n, np.int32); stop = np.zeros(n, np.int32); start = np.zeros(n)
    res = BatchResult.alloc(n)
    snap = pol.snapshot(); opts = eng._opts(True, False, True); out = res.struct()
    refined = C.POINTER(N.EgPlanSet)()
    N.check(N.lib().eg_refine_plans_moves(eng.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(ro), C.byref(mo), C.c_uint64(seed), C.c_uint64(index),
                                          C.byref(refined), steps, n_steps.ctypes.data_as(C.POINTER(C.c_int32)), stop.ctypes.data_as(C.POINTER(C.c_int32)),
                                          start.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out)), "eg_refine_plans_moves")
    return Plan._take_set(refined), steps, n_steps, stop, start, res


# ---------------------------------------------------------------- max_shift == 0 is eg_refine_plans
@pytest.mark.parametrize("mode", [1, 2])
def test_without_a_shift_every_field_is_eg_refine_plans(world, engine, mode):
    pol, plans = _plans()
    rounds = 3
    want = engine.refine_plans(pol, plans, SEED, 0, mode, rounds, replace_with=[12], append_with=[14])
    refined, steps, n_steps, stop, start, res = _raw(engine, pol, plans, SEED, 0, mode, rounds, 0, [12], [14])
    assert sum(len(w[1]) for w in want) >= 3
    for p, (wplan, wsteps, wstop, wstart, wrec) in enumerate(want):
        assert refined[p] == wplan and refined[p].name == wplan.name == plans[p].name
        assert ("local_optimum", "max_rounds", "base_failed")[int(stop[p])] == wstop and int(n_steps[p]) == len(wsteps)
        assert bits(start[p]) == bits(wstart)
        for r, w in enumerate(wsteps):
            s = steps[p * rounds + r]
            assert s.is_move == 0 and bytes(s.move) == bytes(12), (p, r)
            e = s.edit
            assert PlanEdit(PlanEdit.KINDS[e.kind], e.list, e.year, e.pos, e.action) == w.edit, (p, r)
            assert (s.variant, s.n_variants, s.n_failed) == (w.variant, w.n_variants, w.n_failed), (p, r)
            assert bits(s.score) == bits(w.score) and bytes(s.metrics) == w.metrics.tobytes(), (p, r)
        for name in _ALL_FIELDS + ("n_chunks",):
            assert _used(res, name)[p:p + 1].tobytes() == _used(wrec, name).tobytes(), (p, "the refined plan's record", name)


# ---------------------------------------------------------------- the definition, and a move that wins
@pytest.mark.parametrize("max_shift, launch", [(1, None), (3, None), (1, "400")])
def test_every_plan_follows_the_restated_loop(world, engine, monkeypatch, max_shift, launch):
    pol, plans = _plans()
    if launch is None:
        monkeypatch.delenv(LAUNCH, raising=False)
    else:      # 285 + 300 > 400: no two of these plans share a launch, so a round takes several
        monkeypatch.setenv(LAUNCH, launch)
    got = engine.refine_plans(pol, plans, SEED, 0, 1, 3, max_shift=max_shift)
    monkeypatch.delenv(LAUNCH, raising=False)
    assert len(got) == len(plans) and [g[0].name for g in got] == [p.name for p in plans]
    for p, plan in enumerate(plans):
        want = refine_restated(engine, pol, plan, SEED, 0, 1, 3, max_shift)
        _assert_is_the_restatement(got[p], want, (max_shift, launch, "plan", p))
    # the fixture's plan: no edit improves it, so its first step is a move — the one the tabled oracle found on the CPU
    first = got[0][1][0]
    assert isinstance(first.edit, PlanMove) and first.edit == FIXTURE_STEPS[max_shift], first
    assert first.n_variants == len(round_edits(plans[0])) + len(round_moves(plans[0], max_shift)) and first.variant >= len(round_edits(plans[0]))
    assert first.score > got[0][3]
    assert got[0][0] != plans[0] and len(got[0][0]) == len(plans[0]) - sum(1 for s in got[0][1] if isinstance(s.edit, PlanEdit) and s.edit.kind == "delete")
    # the duplicate gives the duplicate's result
    assert got[3][0] == got[1][0] and [s.edit for s in got[3][1]] == [s.edit for s in got[1][1]] and got[3][2] == got[1][2]


def test_the_raw_steps_say_which_of_edit_and_move_they_hold(world, engine):
    pol, plans = _plans()
    refined, steps, n_steps, stop, start, res = _raw(engine, pol, plans[:2], SEED, 0, 1, 3, 1)
    want = engine.refine_plans(pol, plans[:2], SEED, 0, 1, 3, max_shift=1)
    kinds = set()
    for p in range(2):
        assert int(n_steps[p]) == len(want[p][1]) and refined[p] == want[p][0]
        for r, w in enumerate(want[p][1]):
            s = steps[p * 3 + r]
            kinds.add(s.is_move)
            if s.is_move:
                assert s.is_move == 1 and bytes(s.edit) == bytes(12) and PlanMove(s.move.list, s.move.year, s.move.pos, s.move.to_year, s.move.to_pos) == w.edit
            else:
                assert bytes(s.move) == bytes(12) and PlanEdit(PlanEdit.KINDS[s.edit.kind], s.edit.list, s.edit.year, s.edit.pos, s.edit.action) == w.edit
    assert kinds == {0, 1}, kinds      # the short base starts with edits, the fixture's plan with a move


# ---------------------------------------------------------------- the script
def g17(x):
    return "%.17g" % x


def test_the_front_script_without_shift_writes_the_bytes_it_always_wrote(built, tmp_path):
    """scripts/refine_front.py without --shift: index.csv and trajectories.csv are, byte for byte, the format the script has had since it
    exists — written out here once more from Engine.refine_plans' result — and with --shift a move has its kind and its two columns."""
    from eirgrid_amd.engine import Engine
    from eirgrid_amd.world import World
    import json
    wd = World.from_json_dict(json.load(open(WORLD)))
    pol, plans = _plans()
    bases = plans[:2]
    ckpt = str(tmp_path / "policy.json")
    pol.save_to_file(ckpt)
    pol = ActionWeights.load_from_file(ckpt)
    plan_file = str(tmp_path / "bases.jsonl")
    Plan.save(plan_file, bases)
    outs = {}
    for shift in (0, 1):
        out_dir = str(tmp_path / f"front{shift}")
        run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "refine_front.py"), "--world", WORLD, "--plans", plan_file, "--policy", ckpt, "--seed", str(SEED),
                              "--rounds", "2", "--out", out_dir] + (["--shift", "1"] if shift else ["--replace", "12"]), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout + run.stderr
        outs[shift] = os.path.join(out_dir, "refine")
    eng = Engine(wd, device=0)
    try:
        # (with the replaces a replace is the fixture's plan's best step; without them no edit improves it and the move is taken)
        want = {shift: eng.refine_plans(pol, bases, SEED, 0, 1, 2, replace_with=None if shift else [12], max_shift=shift) for shift in (0, 1)}
    finally:
        eng.close()
    lists = ("best_actions", "best_deficit_actions")
    for shift in (0, 1):
        index = "plan,name,stop,steps,start_score,final_score," + ",".join(METRICS) + "\n"
        traj = "plan,round,kind,list,year,pos,action,variant,n_variants,n_failed,score," + ",".join(METRICS) + (",to_year,to_pos" if shift else "") + "\n"
        for p, (plan, steps, stop, start, rec) in enumerate(want[shift]):
            index += ",".join([str(p), bases[p].name, stop, str(len(steps)), g17(start), g17(steps[-1].score if steps else start)] + [g17(v) for v in rec.metrics[0]]) + "\n"
            traj += f"{p},start,none,,,,,0,,,{g17(start)},,,," + (",," if shift else "") + "\n"
            at = bases[p]
            for r, s in enumerate(steps):
                e = s.edit
                if isinstance(e, PlanMove):
                    row = [p, r, "move", lists[e.list], 2025 + e.year, e.pos, at.best_actions[e.year][e.pos]]
                    tail, at = [2025 + e.to_year, e.to_pos], apply_move(at, e)
                else:
                    row = [p, r, e.kind, lists[e.list], 2025 + e.year, e.pos, "" if e.kind == "delete" else e.action]
                    tail, at = ["", ""], apply_edit(at, e)
                traj += ",".join(map(str, row + [s.variant, s.n_variants, s.n_failed, g17(s.score)] + [g17(v) for v in s.metrics] + (tail if shift else []))) + "\n"
        assert open(os.path.join(outs[shift], "index.csv"), "rb").read() == index.encode(), shift
        assert open(os.path.join(outs[shift], "trajectories.csv"), "rb").read() == traj.encode(), shift
        assert Plan.load(os.path.join(outs[shift], "refined.jsonl")) == [w[0] for w in want[shift]]
        saved = str(tmp_path / f"want{shift}.jsonl")
        Plan.save(saved, [w[0] for w in want[shift]])
        assert open(os.path.join(outs[shift], "refined.jsonl"), "rb").read() == open(saved, "rb").read()
    assert ",move,best_actions," in open(os.path.join(outs[1], "trajectories.csv")).read()
    assert ",move," not in open(os.path.join(outs[0], "trajectories.csv")).read()
