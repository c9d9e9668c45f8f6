"""GPU: greedy plan refinement (include/eirgrid_hip.h eg_refine_plan; csrc/eg_refine.cpp, csrc/eg_refine_many.h k_refine_pick_many).  The
device picks each round's winner and makes its plan block the next round's base; the trajectory must be the one the definition gives — restated
once as a loop over Engine.evaluate_plan_edits + rank_score (scores and metrics bit for bit) and once over the tabled
oracle (tests/test_refine.py refine_restated)."""
import csv
import json
import os
import re
import subprocess

import numpy as np
import pytest

from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanEdit
from eirgrid_amd.world import World
from tests.helpers import assert_episode_equal
from tests.test_gpu_plan_edits import _long_policy, _sized_plan
from tests.test_gpu_plans import _engine, _run_dir, _same_records
from tests.test_refine import CASES, SEED, OracleEvaluator, apply_edit, oracle_run, refine_restated, round_edits, short_policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def _loop(eng, pol, seed=SEED, index=0):
    """the round's variants as the existing plan-edit path evaluates them (whole records fetched, scored on the host)"""
    def evaluate(plan, edits):
        res = eng.evaluate_plan_edits(pol, plan, edits, seed, index, same_index=True)
        return res.status.copy(), res.metrics.copy()
    return evaluate


def _assert_same_trajectory(got, want, what, bitwise=True):
    plan, steps, stop, start, _rec = got
    wplan, wsteps, wstop, wstart = want[:4]
    assert stop == wstop and len(steps) == len(wsteps), (what, stop, wstop, len(steps), len(wsteps))
    assert np.float64(start).tobytes() == np.float64(wstart).tobytes() or (np.isnan(start) and np.isnan(wstart)), (what, start, wstart)
    for r, (s, w) in enumerate(zip(steps, wsteps)):
        assert (s.edit, s.variant, s.n_variants, s.n_failed) == (w[0], w[1], w[2], w[3]), (what, r, s, w[:4])
        assert np.float64(s.score).tobytes() == np.float64(w[4]).tobytes(), (what, r, s.score, w[4])
        assert s.metrics.tobytes() == np.asarray(w[5], np.float64).tobytes(), (what, r)
    assert plan == wplan, what


@pytest.mark.parametrize("helper", ["0", "all"])
@pytest.mark.parametrize("name", list(CASES))
def test_refinement_is_the_definition(world, helper, name):
    case = CASES[name]
    pol, base, ev, want = oracle_run(world, name)
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        got = eng.refine_plan(pol, base, SEED, 0, case["mode"], case["max_rounds"], replace_with=case["replace_with"])
        loop = refine_restated(_loop(eng, pol), base, case["mode"], case["max_rounds"], case["replace_with"])
        _assert_same_trajectory(got, loop, (name, helper, "loop over evaluate_plan_edits"))
        _assert_same_trajectory(got, want, (name, helper, "tabled oracle"))
        assert all(s.n_failed == 0 for s in got[1])      # no variant skipped as failed: the oracle run showed none
        assert_episode_equal(got[4], 0, ev.record(got[0]), f"{name}: the refined plan's record")
    finally:
        eng.close()


def test_the_device_applied_base_is_the_refined_plans_block(world, engine):
    case = CASES["short, mode 2"]
    pol, base, ev, want = oracle_run(world, "short, mode 2")
    plan, steps, stop, start, rec = engine.refine_plan(pol, base, SEED, 0, case["mode"], case["max_rounds"], replace_with=case["replace_with"])
    assert stop == "local_optimum" and len(steps) == 1
    dev = engine.debug_fetch_plan_block(0)      # variant 0 of the last round: a copy of the base k_refine_pick_many installed
    last = engine.fetch(237)                    # the last round's variants stay behind as the last batch (239 less the deleted entry's delete and replace)
    assert last.metrics[0].tobytes() == rec.metrics[0].tobytes()
    engine.evaluate_plans(pol, [plan], SEED, 0)
    host = engine.debug_fetch_plan_block(0)
    assert dev.tobytes() == host.tobytes(), np.flatnonzero(dev != host)[:8]
    assert dev.tobytes() != _block_of(engine, pol, base).tobytes()


def test_one_plan_gets_a_launch_to_itself_whatever_the_launch_size(engine, monkeypatch):
    """eg_refine_plan is eg_refine_plans' loop over one plan.  A plan never straddles two launches, so the smallest launch size must not
    split its 239 variants: the same plan, steps, stop reason and start score, and the same record in every field, n_chunks included."""
    case = CASES["short, mode 2"]
    pol = case["policy"]()
    base = Plan.from_policy(pol)
    runs = []
    for cap in ("1", None):
        if cap is None:
            monkeypatch.delenv("EIRGRID_REFINE_LAUNCH_VARIANTS", raising=False)
        else:
            monkeypatch.setenv("EIRGRID_REFINE_LAUNCH_VARIANTS", cap)
        runs.append(engine.refine_plan(pol, base, SEED, 0, case["mode"], case["max_rounds"], replace_with=case["replace_with"]))
    (plan, steps, stop, start, rec), unset = runs
    assert stop == "local_optimum" and len(steps) == 1 and steps[0].n_variants == 239
    _assert_same_trajectory(runs[0], (unset[0], [(s.edit, s.variant, s.n_variants, s.n_failed, s.score, s.metrics) for s in unset[1]], unset[2], unset[3]),
                            "a launch size of 1 against the default")
    _same_records(rec, unset[4], "the refined plan's record")


def _block_of(eng, pol, plan):
    eng.evaluate_plans(pol, [plan], SEED, 0)
    return eng.debug_fetch_plan_block(0)


CROSSINGS = [
    # a 97-action base whose best delete takes it to 96 actions: round 0 runs the base on the long-replay route and 97 of its variants on
    # the short one, rounds 1 and 2 are short throughout.  (Under a fresh policy no append improves a 95- or 96-action base of this
    # shape — the tabled oracle picks a delete every time — so the other direction is not reached by a greedy step.)
    dict(n=97, append_with=(14,), max_rounds=2, lengths=[97, 96, 95]),
]


@pytest.mark.parametrize("helper", ["0", "all"])
@pytest.mark.parametrize("case", CROSSINGS, ids=["97 down"])
def test_a_trajectory_crosses_the_short_long_boundary(world, helper, case):
    pol = ActionWeights()
    base = _sized_plan(case["n"])
    ev = OracleEvaluator(world, pol, 19, 64)
    want = refine_restated(ev, base, 1, case["max_rounds"], (), case["append_with"])
    lengths = [len(base)]
    plan = base
    for s in want[1]:
        plan = apply_edit(plan, s[0]); lengths.append(len(plan))
    assert lengths == case["lengths"], lengths      # the crossing happened (picked with the oracle on the CPU)
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        got = eng.refine_plan(pol, base, 19, 64, 1, case["max_rounds"], append_with=case["append_with"])
        _assert_same_trajectory(got, want, (case["n"], helper, "tabled oracle"))
        _assert_same_trajectory(got, refine_restated(_loop(eng, pol, 19, 64), base, 1, case["max_rounds"], (), case["append_with"]), (case["n"], helper, "loop"))
        assert_episode_equal(got[4], 0, ev.record(got[0]), "the refined plan's record")
    finally:
        eng.close()


def _overflow_base():
    """tests/test_gpu_plan_edits.py's shape: a replay of these 2 042 entries fills the 4 096-entry run record to the last one or two;
    one more entry overflows it"""
    run = [[60] * 78 for _ in range(26)]
    run[0] = [15] * 20 + [60] * (2042 - 25 * 78 - 20)
    return Plan(run, [[24] for _ in range(26)])


def test_failed_variants_are_counted_and_never_win(world, engine):
    # cost_only: the score rises with every nuclear plant deleted, so the plan moves — in mode 1 this base is a local optimum, and a run
    # without a step reports no count.  Round 0: each of the 26 appends overflows the run record; round 1, one entry shorter: none does.
    pol = ActionWeights()
    base = _overflow_base()
    got = engine.refine_plan(pol, base, 23, 0, 2, 2, append_with=[60])
    _assert_same_trajectory(got, refine_restated(_loop(engine, pol, 23, 0), base, 2, 2, (), [60]), "beside overflowing variants, loop")
    _assert_same_trajectory(got, refine_restated(OracleEvaluator(world, pol, 23, 0), base, 2, 2, (), [60]), "beside overflowing variants, tabled oracle")
    plan, steps, stop, start, rec = got
    assert stop == "max_rounds" and [s.n_variants for s in steps] == [1 + 2042 + 26 + 26, 2042 + 26 + 26]
    assert [s.n_failed for s in steps] == [26, 0], steps
    assert all(s.edit.kind == "delete" for s in steps) and rec.status[0] == 0
    edits = round_edits(base, (), [60])
    first = engine.evaluate_plan_edits(pol, base, edits, 23, 0, same_index=True)      # round 0 once more: who failed
    failed = np.flatnonzero(first.status != 0)
    assert failed.tolist() == list(range(len(edits) - 26, len(edits))) and (first.status[failed] == -1).all()      # the appends, EG_EP_OVERFLOW
    assert steps[0].variant not in failed


def test_a_failing_base_stops_at_once(world, engine):
    pol = ActionWeights()
    base = apply_edit(_overflow_base(), PlanEdit("insert", 0, 25, 78, 60))
    assert engine.evaluate_plans(pol, [base], 23, 0).status[0] == -1
    plan, steps, stop, start, rec = engine.refine_plan(pol, base, 23, 0, 1, 3)
    assert stop == "base_failed" and steps == [] and plan == base and rec is None and np.isnan(start)


def test_refine_calls_do_not_touch_training(world, tmp_path):
    pol_eval = _long_policy(9)
    base = Plan.from_policy(pol_eval)
    out = []
    for refine in (False, True):
        eng = Engine(world, device=0)
        try:
            eng.push(ActionWeights())
            eng.track_best_result()
            eng.track_top_k(10)
            for step in range(6):
                eng.device_step(3, 1024 * step, 1024, 10, 3 + step)
                if refine and step < 5:
                    r = eng.refine_plan(pol_eval, base, 9, 0, 1 + step % 2, 2, replace_with=[12] if step % 2 else None)
                    assert len(r[1]) >= 1
            batch = eng.fetch(1024)
            pol = ActionWeights(); eng.pull(pol)
            path = tmp_path / f"policy_{refine}.json"
            pol.save_to_file(path)
            text = re.sub(r'"timestamp": "[^"]*"', '"timestamp": ""', path.read_text())      # (the host's clock at the pull)
            idx, best = eng.fetch_best_result()
            rows, scores, index = eng.fetch_top_k()
            out.append((text, batch, idx, best, rows, scores.tobytes(), index.tobytes()))
        finally:
            eng.close()
    (pa, la, ia, ba, ra, sa, xa), (pb, lb, ib, bb, rb, sb, xb) = out
    assert pa == pb and ia == ib and sa == sb and xa == xb
    _same_records(la, lb, "last batch")
    _same_records(ba, bb, "best_result")
    _same_records(ra, rb, "top-k")


def test_a_rank_of_a_group_is_refused(world):
    from eirgrid_amd._native import EirgridError
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        with pytest.raises(EirgridError, match="rank of an eg_group"):
            g.ranks[0].refine_plan(ActionWeights(), _sized_plan(30), 1)
    finally:
        g.close()


def test_cli_writes_the_trajectory_and_the_refined_plan(built, tmp_path):
    wd = World.from_json_dict(json.load(open(WORLD)))
    pol = short_policy()
    base = Plan.from_policy(pol, "short")
    ckpt = str(tmp_path / "policy.json")
    pol.save_to_file(ckpt)
    pol = ActionWeights.load_from_file(ckpt)      # (as the CLI sees it: a checkpoint carries no count table)
    plan_file = str(tmp_path / "base.jsonl")
    Plan.save(plan_file, [base])
    rd = str(tmp_path / "refine")
    args = [CLI, "--world", WORLD, "--evaluate-policy", ckpt, "--seed", str(SEED), "--refine", plan_file, "--refine-rounds", "3", "--refine-replace", "12",
            "--refine-append", "14", "-c", rd]
    out = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    d = os.path.join(_run_dir(rd), "refine")
    lines = open(os.path.join(d, "trajectory.csv")).read().splitlines()
    eng = Engine(wd, device=0)
    try:
        plan, steps, stop, start, rec = eng.refine_plan(pol, base, SEED, 0, 1, 3, replace_with=[12], append_with=[14])
    finally:
        eng.close()
    assert lines[-1] == f"# stop: {stop} after {len(steps)} steps" and len(steps) >= 1
    rows = list(csv.DictReader(lines[:-1]))
    assert list(rows[0].keys()) == "round,kind,list,year,pos,action,variant,n_variants,n_failed,score,net_emissions,public_opinion,total_cost,power_reliability".split(",")
    assert rows[0]["round"] == "start" and rows[0]["score"] == "%.17g" % start and len(rows) == 1 + len(steps)
    for r, (row, s) in enumerate(zip(rows[1:], steps)):
        e = s.edit
        assert (row["round"], row["kind"], row["list"], row["year"], row["pos"]) == (str(r), e.kind, ("best_actions", "best_deficit_actions")[e.list], str(2025 + e.year), str(e.pos))
        assert row["action"] == ("" if e.kind == "delete" else str(e.action))
        assert (int(row["variant"]), int(row["n_variants"]), int(row["n_failed"])) == (s.variant, s.n_variants, s.n_failed)
        assert row["score"] == "%.17g" % s.score
        assert [row[k] for k in ("net_emissions", "public_opinion", "total_cost", "power_reliability")] == ["%.17g" % v for v in s.metrics]
    refined = os.path.join(d, "refined.jsonl")
    assert Plan.load(refined) == [plan]
    ev = str(tmp_path / "evaluate")
    out = subprocess.run([CLI, "--world", WORLD, "--evaluate-policy", ckpt, "--seed", str(SEED), "--evaluate", refined, "-c", ev], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    index = list(csv.DictReader(open(os.path.join(_run_dir(ev), "plans", "index.csv"))))
    assert len(index) == 1 and index[0]["status"] == "0" and index[0]["score"] == rows[-1]["score"]
