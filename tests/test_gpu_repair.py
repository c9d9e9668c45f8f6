"""GPU: plan repair (include/eirgrid_hip.h eg_repair_plans; csrc/eg_repair.h k_repair_pick_many, csrc/eg_refine.cpp).  Engine.repair_plans
on the short case of tests/test_gpu_plan_constraints.py against tests/test_repair.py repair_restated run over the UNCONSTRAINED engine —
statuses and excess rows from tests/test_plan_constraints.py judge —: steps, stops, violations, plans and the record, byte for byte; one
plan, three in a call, the same three a launch each, with and without moves.  And what the call leaves alone."""
import dataclasses

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.constraints import Constraint
from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanMove
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plan_constraints import NAME, _demoting_loop, constrained, short      # noqa: F401 (short: the module's fixture, reused)
from tests.test_gpu_refine import _assert_same_trajectory
from tests.test_plan_constraints import judge
from tests.test_refine import CASES, SEED, apply_edit, refine_restated, round_edits
from tests.test_repair import repair_restated

pytestmark = pytest.mark.gpu

OK, INFEASIBLE = N.EG_EP_OK, N.EG_EP_INFEASIBLE
LAUNCH = "EIRGRID_REFINE_LAUNCH_VARIANTS"
MODE = 2


def bits(x):
    return np.float64(x).tobytes()


def _judging(eng, pol, constraints):
    """repair_restated's evaluator: a round's variants evaluated WITHOUT constraints, judged by the restatement"""
    def evaluate(plan, edits, moves):
        res = [eng.evaluate_plan_edits(pol, plan, edits, SEED, 0, same_index=True)]
        if moves:
            res.append(eng.evaluate_plan_moves(pol, plan, moves, SEED, 0, same_index=True))
        status = np.concatenate([r.status for r in res]); metrics = np.concatenate([r.metrics for r in res]); yearly = np.concatenate([r.yearly for r in res])
        judged, violated, excess = judge(yearly, status, constraints)
        return judged, metrics.copy(), excess
    return evaluate


@pytest.fixture(scope="module")
def broken(short):
    """(policy, [a plan one delete below the reserve, the feasible base, a plan two deletes below it], the reserve and the generation floor,
    the neighbourhood that holds the two deleted actions)"""
    pol, base, edits, free, cs = short
    bad = apply_edit(base, edits[1])                 # the unconstrained winner of the refinement: it dips under the reserve
    deleted = base.best_actions[edits[1].year][edits[1].pos]
    e2 = round_edits(bad, CASES[NAME]["replace_with"])[3]
    second = bad.best_actions[e2.year][e2.pos]
    worse = apply_edit(bad, e2)
    hood = dict(replace_with=CASES[NAME]["replace_with"], append_with=(deleted, second))
    return pol, [Plan(bad.best_actions, bad.best_deficit_actions, "bad"), Plan(base.best_actions, base.best_deficit_actions, "base"),
                 Plan(worse.best_actions, worse.best_deficit_actions, "worse")], cs, hood


def _assert_is_the_restatement(engine, pol, got, want, cs, what):
    plan, steps, stop, start, final, rec = got
    wplan, wsteps, wstop, wstart, wfinal = want
    assert stop == wstop and len(steps) == len(wsteps), (what, stop, wstop, len(steps), len(wsteps))
    assert (bits(start), bits(final)) == (bits(wstart), bits(wfinal)), (what, start, wstart, final, wfinal)
    for r, (s, w) in enumerate(zip(steps, wsteps)):
        assert type(s.edit) is type(w[0]) and s.edit == w[0], (what, r, s.edit, w[0])
        assert (s.variant, s.n_variants, s.n_failed, s.n_feasible, s.violated) == w[1:6], (what, r, s, w[1:6])
        assert bits(s.violation) == bits(w[6]) and bits(s.score) == bits(w[7]) and s.metrics.tobytes() == w[8].tobytes(), (what, r, s, w)
    assert plan == wplan, what
    # the record: the returned plan's, evaluated alone without constraints, but for the status the judgment gives it
    alone = engine.evaluate_plans(pol, [wplan], SEED, 0)
    status = judge(alone.yearly, alone.status, cs)[0]
    assert rec is not None and rec.status.tolist() == status.tolist(), (what, rec.status, status)
    for name in _ALL_FIELDS:
        assert name == "status" or _used(rec, name).tobytes() == _used(alone, name).tobytes(), (what, "the record", name)
    if steps:
        assert rec.metrics[0].tobytes() == steps[-1].metrics.tobytes(), what


# ---------------------------------------------------------------- 1: the definition
@pytest.mark.parametrize("max_shift", [0, 1])
def test_one_infeasible_plan_is_repaired_as_the_definition_says(engine, broken, max_shift):
    pol, plans, cs, hood = broken
    cs = cs[:1]
    want = repair_restated(_judging(engine, pol, cs), plans[0], MODE, 4, max_shift=max_shift, **hood)
    # the base is truly infeasible and the restated descent ends feasible after at least one step: nothing here passes vacuously
    assert want[2] == "feasible" and len(want[1]) >= 1 and want[3] > 0.0 and want[4] == 0.0, want[1:]
    with constrained(engine, cs):
        got = engine.repair_plans(pol, [plans[0]], SEED, 0, MODE, 4, max_shift=max_shift, **hood)
    assert len(got) == 1 and got[0][0].name == "bad"
    _assert_is_the_restatement(engine, pol, got[0], want, cs, ("one plan", max_shift))
    st, names, ex = engine.plan_feasibility(pol, [got[0][0]], SEED, 0, constraints=cs)      # replayed alone, the repaired plan is legal
    assert st.tolist() == [OK] and names == [[]]


@pytest.mark.parametrize("max_shift, launch, k, weights, rounds", [(0, None, 1, None, 3), (1, None, 1, None, 3), (0, "1", 1, None, 3), (1, "500", 2, (1.0, 0.001), 3),
                                                                   (0, None, 2, (0.5, 3.0), 1)])
def test_three_plans_in_a_call_each_as_if_alone(engine, broken, monkeypatch, max_shift, launch, k, weights, rounds):
    pol, plans, cs, hood = broken
    cs = cs[:k]
    if launch is None:
        monkeypatch.delenv(LAUNCH, raising=False)
    else:      # "1": every plan a launch to itself; "500": no two of the plans with their moves share one
        monkeypatch.setenv(LAUNCH, launch)
    with constrained(engine, cs):
        got = engine.repair_plans(pol, plans, SEED, 0, MODE, rounds, max_shift=max_shift, violation_weights=weights, **hood)
    monkeypatch.delenv(LAUNCH, raising=False)
    assert [g[0].name for g in got] == ["bad", "base", "worse"]
    wants = [repair_restated(_judging(engine, pol, cs), p, MODE, rounds, max_shift=max_shift, weights=weights, **hood) for p in plans]
    for p, (g, w) in enumerate(zip(got, wants)):
        _assert_is_the_restatement(engine, pol, g, w, cs, (max_shift, launch, k, "plan", p))
    # a feasible base: no steps, its own record
    assert wants[1][1:] == ([], "feasible", 0.0, 0.0) and got[1][0] == plans[1]
    if rounds == 3:      # the plan two deletes down needs two steps; with moves allowed the second one is a move
        assert [w[2] for w in wants] == ["feasible"] * 3 and len(wants[0][1]) == 1 and len(wants[2][1]) == 2, [w[1:] for w in wants]
        assert wants[2][3] > wants[2][1][0][6] > wants[2][1][1][6] == 0.0      # V falls strictly
        if k == 1:
            assert isinstance(wants[2][1][1][0], PlanMove) == (max_shift == 1)
        for g in got:      # replayed alone, every repaired plan is legal
            assert engine.plan_feasibility(pol, [g[0]], SEED, 0, constraints=cs)[0].tolist() == [OK]
    else:
        assert wants[2][2] == "max_rounds" and len(wants[2][1]) == 1 and wants[2][4] > 0.0


def test_without_the_repairing_action_the_descent_runs_out_of_rounds(engine, broken):
    pol, plans, cs, hood = broken
    kw = dict(replace_with=hood["replace_with"])
    want = repair_restated(_judging(engine, pol, cs), plans[0], MODE, 3, weights=(0.5, 3.0), **kw)
    assert want[2] == "max_rounds" and len(want[1]) == 3 and want[3] > want[1][0][6] > want[1][1][6] > want[1][2][6] == want[4] > 0.0
    with constrained(engine, cs):
        got = engine.repair_plans(pol, [plans[0]], SEED, 0, MODE, 3, violation_weights=(0.5, 3.0), **kw)
    _assert_is_the_restatement(engine, pol, got[0], want, cs, "max_rounds")
    assert got[0][5].status[0] == INFEASIBLE


# ---------------------------------------------------------------- 2: refinement is what it was
def test_refine_under_constraints_returns_what_it_returned(engine, short):
    pol, base, edits, free, cs = short
    case = CASES[NAME]
    cs = cs[:1]
    second = apply_edit(base, edits[2])
    kw = dict(replace_with=case["replace_with"])
    with constrained(engine, cs):
        one = engine.refine_plan(pol, base, SEED, 0, case["mode"], case["max_rounds"], **kw)
        many = engine.refine_plans(pol, [base, second], SEED, 0, case["mode"], case["max_rounds"], **kw)
        failed = engine.refine_plans(pol, [apply_edit(base, edits[1])], SEED, 0, case["mode"], 2, max_shift=1, **kw)
    for what, got, start in (("refine_plan", one, base), ("refine_plans[0]", many[0], base), ("refine_plans[1]", many[1], second)):
        want = refine_restated(_demoting_loop(engine, pol, cs), start, case["mode"], case["max_rounds"], case["replace_with"])
        _assert_same_trajectory(got, want, what)
    assert failed[0][2] == "base_failed" and failed[0][1] == [] and np.isnan(failed[0][3]) and failed[0][4] is None


# ---------------------------------------------------------------- 3: refusals
def test_the_call_refuses_what_it_cannot_do(engine, world, broken):
    pol, plans, cs, hood = broken
    with pytest.raises(EirgridError, match="eg_repair_plans: no plan constraints are set"):
        engine.repair_plans(pol, plans, SEED, 0, MODE, 2, **hood)
    with constrained(engine, cs):
        for bad in ((1.0, 0.0), (-1.0, 1.0), (np.inf, 1.0), (1.0, np.nan)):
            with pytest.raises(EirgridError, match=r"eg_repair_plans: weights\[[01]\] = .* \(finite and > 0\)"):
                engine.repair_plans(pol, plans, SEED, 0, MODE, 2, violation_weights=bad, **hood)
        with pytest.raises(ValueError, match="3 violation weights for 2 constraints"):
            engine.repair_plans(pol, plans, SEED, 0, MODE, 2, violation_weights=(1.0, 1.0, 1.0), **hood)
        with pytest.raises(EirgridError, match=r"eg_repair_plans: max_shift = 26"):
            engine.repair_plans(pol, plans, SEED, 0, MODE, 2, max_shift=26, **hood)
        with pytest.raises(EirgridError, match=r"eg_repair_plans: mode 3"):
            engine.repair_plans(pol, plans, SEED, 0, 3, 2, **hood)
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        with pytest.raises(EirgridError, match="eg_repair_plans: the context is a rank of an eg_group"):
            g.ranks[0].repair_plans(pol, plans, SEED, 0, MODE, 2, **hood)
    finally:
        g.close()


# ---------------------------------------------------------------- 4: what the call leaves alone
def test_constraints_archive_and_resident_policy_are_untouched(world, broken):
    pol_eval, plans, cs, hood = broken
    eng = Engine(world, device=0)
    try:
        eng.set_constraints(cs)
        eng.track_pareto(16)
        eng.push(ActionWeights())
        eng.device_step(3, 0, 256, 10, 3)
        eng.fold_pareto_last_batch()
        before = eng.fetch_pareto()
        pol_before = ActionWeights(); eng.pull(pol_before)
        got = eng.repair_plans(pol_eval, plans, SEED, 0, MODE, 4, max_shift=1, **hood)
        assert [g[2] for g in got] == ["feasible"] * 3
        after = eng.fetch_pareto()
        pol_after = ActionWeights(); eng.pull(pol_after)
        assert eng.last_batch_constraints() == cs and eng._constraints == cs      # judged under them, and they are still set
        # ... for the next batch as well
        assert eng.evaluate_plans(pol_eval, [plans[0]], SEED, 0).status[0] == INFEASIBLE
        assert before[0].metrics.shape[0] > 0 and before[3] == after[3]
        for f in dataclasses.fields(before[0]):
            assert getattr(before[0], f.name).tobytes() == getattr(after[0], f.name).tobytes(), f.name
        assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
        assert [t.tobytes() for t in pol_before.tables()] == [t.tobytes() for t in pol_after.tables()]
        assert [pol_before.lists(0), pol_before.lists(1)] == [pol_after.lists(0), pol_after.lists(1)]
    finally:
        eng.close()


# ---------------------------------------------------------------- 5: the script
def test_the_script_writes_what_repair_plans_returns(engine, broken, tmp_path):
    import csv
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pol, plans, cs, hood = broken
    ckpt = str(tmp_path / "policy.json")
    pol.save_to_file(ckpt)
    pol = ActionWeights.load_from_file(ckpt)      # (as the tools see it: a checkpoint carries no count table)
    plan_file = str(tmp_path / "broken.jsonl")
    Plan.save(plan_file, plans)
    out_dir = str(tmp_path / "out")
    run = subprocess.run([sys.executable, os.path.join(root, "scripts", "repair_plans.py"), "--world", "synthetic", "--plans", plan_file, "--policy", ckpt, "--seed", str(SEED),
                          "--constraint", str(cs[0]), "--constraint", str(cs[1]), "--weight", "1,0.001", "--rounds", "3", "--replace", ",".join(map(str, hood["replace_with"])),
                          "--append", ",".join(map(str, hood["append_with"])), "--shift", "1", "--cost-only", "--then-refine", "--out", out_dir],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    with constrained(engine, cs):
        want = engine.repair_plans(pol, plans, SEED, 0, MODE, 3, max_shift=1, violation_weights=(1.0, 0.001), **hood)
        legal = [w[0] for w in want if w[2] == "feasible"]
        refined = engine.refine_plans(pol, legal, SEED, 0, MODE, 3, max_shift=1, **hood)
    assert len(legal) == 3 and sum(len(w[1]) for w in want) == 3
    d = os.path.join(out_dir, "repair")
    back = Plan.load(os.path.join(d, "repaired.jsonl"))
    assert back == [w[0] for w in want] and [p.name for p in back] == ["bad", "base", "worse"]
    index = list(csv.DictReader(open(os.path.join(d, "index.csv"))))
    assert list(index[0].keys()) == ("plan,name,stop,steps,start_violation,final_violation,score,net_emissions,public_opinion,total_cost,power_reliability,"
                                     "violated").split(",")
    for p, (row, (plan, steps, stop, start, final, rec)) in enumerate(zip(index, want)):
        assert (row["plan"], row["name"], row["stop"], row["steps"], row["violated"]) == (str(p), plans[p].name, stop, str(len(steps)), ""), row
        assert (row["start_violation"], row["final_violation"]) == ("%.17g" % start, "%.17g" % final), row
        assert [row[k] for k in ("net_emissions", "public_opinion", "total_cost", "power_reliability")] == ["%.17g" % v for v in rec.metrics[0]]
    rows = list(csv.DictReader(open(os.path.join(d, "trajectories.csv"))))
    assert len(rows) == 3 + 3 and [r["round"] for r in rows] == ["start", "0", "start", "start", "0", "1"]
    steps = [s for w in want for s in w[1]]
    assert [(r["variant"], r["n_variants"], r["n_feasible"], r["violation"]) for r in rows if r["round"] != "start"] == \
        [(str(s.variant), str(s.n_variants), str(s.n_feasible), "%.17g" % s.violation) for s in steps]
    assert [r["kind"] for r in rows if r["round"] != "start"] == ["move" if isinstance(s.edit, PlanMove) else s.edit.kind for s in steps]
    assert Plan.load(os.path.join(out_dir, "refine", "refined.jsonl")) == [r[0] for r in refined]
    assert "repaired 3 plans (3 feasible, 0 stuck, 0 out of rounds, 0 failed; 3 steps in all)" in run.stdout, run.stdout
