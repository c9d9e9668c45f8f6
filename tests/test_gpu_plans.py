"""GPU: plan evaluation (include/eirgrid_hip.h eg_evaluate_plans; csrc/eg_plans.cpp launch_plans; the per-episode list base of the
replay kernels).  Plan j under policy P is the replay episode at global index first + j under a snapshot equal to P with has_best = 1
and the plan as its best lists.  Bar: every record bit-identical to the tabled oracle and to the replay batches the library already
runs; an evaluation leaves the training state of its context untouched."""
import csv
import json
import os
import re
import subprocess

import numpy as np
import pytest

from eirgrid_amd.engine import ActionWeights, BatchResult, Engine, HostTables, Plan, rank_score
from eirgrid_amd.world import World
from oracle import api as O
from oracle import csv_export as OC
from tests.helpers import assert_episode_equal, oracle_weights_like
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_replay_hoist import _full_script, _seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def _engine(world, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine(world, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _oracle_plan(pol, plan):
    ow = oracle_weights_like(pol)
    ow.set("has_best", 1); ow.set("has_best_actions", 1); ow.set("has_best_deficit_actions", 1)
    for y in range(26):
        ow.set_list(0, y, plan.best_actions[y]); ow.set_list(1, y, plan.best_deficit_actions[y])
    return ow


def _same_records(a, b, what, rows_a=None, rows_b=None):
    for name in _ALL_FIELDS + ("n_chunks",):
        ua, ub = _used(a, name), _used(b, name)
        if rows_a is not None:
            ua, ub = ua[rows_a], ub[rows_b]
        assert ua.tobytes() == ub.tobytes(), (what, name)


def _mixed_plans(engine, rng):
    """~256 distinct plans in shuffled order: sampled episodes' lists (short), the same lists cut short (the year lists run out:
    seeded fallbacks), with empty years, long scripts of ~230 generators, and one plan at the 4 096-entry capacity."""
    res = engine.rollout_batch(ActionWeights(), 4711, 96)
    plans = []
    for e in range(96):
        p = Plan.from_result(res, e, f"sampled {e}")
        if e % 3 == 1:
            p = Plan([l[:len(l) // 2] for l in p.best_actions], [l[:1] for l in p.best_deficit_actions], f"cut {e}")
        if e % 3 == 2:
            p = Plan([[] if y % 4 == e % 4 else l for y, l in enumerate(p.best_actions)],
                     [[] if y % 5 == 0 else l for y, l in enumerate(p.best_deficit_actions)], f"gaps {e}")
        plans.append(p)
    for k in range(96):
        pol = _full_script(rng, int(rng.integers(8, 10)), [0, 4, 12, 7, 5, 1, 13, 2], offsets_per_year=int(rng.integers(0, 2)))
        p = Plan.from_policy(pol, f"long {k}")
        if k % 4 == 3:      # a long list whose later years are empty: the fallbacks run with a long list in place
            p = Plan([l if y < 20 else [] for y, l in enumerate(p.best_actions)], p.best_deficit_actions, f"long cut {k}")
        plans.append(p)
    for k in range(63):
        pol = _full_script(rng, int(rng.integers(1, 3)), [0, 4, 12, 7])
        plans.append(Plan.from_policy(pol, f"script {k}"))
    cap = [[60] * 157 for _ in range(26)]
    cap[0] += [60] * (4096 - 26 * 157)
    plans.append(Plan(cap, [[24] for _ in range(26)], "capacity"))
    assert sum(len(l) for l in cap) == 4096
    order = rng.permutation(len(plans))
    plans = [plans[i] for i in order]
    assert len({(json.dumps(p.best_actions), json.dumps(p.best_deficit_actions)) for p in plans}) == len(plans)
    return plans


def test_every_plan_is_the_oracles_replay(world, engine):
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    rng = np.random.default_rng(2030)
    plans = _mixed_plans(engine, rng)
    lengths = np.array([len(p) for p in plans])
    assert (lengths <= 96).sum() >= 32 and (lengths > 200).sum() >= 32
    classic = _engine(world, EIRGRID_REPLAY_SOLO="0", EIRGRID_HELPER_WAVES="0")
    solo = _engine(world, EIRGRID_HELPER_WAVES="0")
    try:
        for pi, pol in enumerate([ActionWeights(), _seeded(engine)]):
            seed, first = 900 + pi, 10_000 * (pi + 1)
            a = solo.evaluate_plans(pol, plans, seed, first)
            b = classic.evaluate_plans(pol, plans, seed, first)
            c = engine.evaluate_plans(pol, plans, seed, first)      # (256 plans: the small-batch kernel)
            ok = a.status == 0
            assert ok.mean() > 0.9 and (a.status[~ok] == -1).all()      # (the capacity plan overflows: EG_EP_OVERFLOW)
            # An episode that failed writes the per-year counts and rows of the years it ran only: the rest of its record is what an
            # earlier batch of that engine left there (the three engines have different histories).  Of a failed episode: what it writes
            # at its end.
            for name in ("status", "metrics", "n_gens", "n_offsets", "n_draws"):
                assert getattr(a, name).tobytes() == getattr(b, name).tobytes() == getattr(c, name).tobytes(), (pi, name)
            _same_records(a, b, f"policy {pi}: solo vs classic", ok, ok)
            for name in _ALL_FIELDS:
                assert _used(a, name)[ok].tobytes() == _used(c, name)[ok].tobytes(), (pi, name)
            assert (a.n_draws[lengths <= 96] > 0).any()
            for j, p in enumerate(plans):
                st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, p), seed + first + j, replay=True)
                if ok[j]:
                    assert_episode_equal(a, j, ref, f"policy {pi}, plan {j} ({p.name})")
                else:
                    assert st == a.status[j], (pi, j, p.name)
    finally:
        classic.close(); solo.close()


@pytest.mark.parametrize("helper", ["0", "all"])
def test_copies_of_a_plan_are_the_replay_batch(world, engine, helper):
    rng = np.random.default_rng(77)
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        for pol in (_seeded(engine), _full_script(rng, 9, [0, 4, 12, 7, 5, 1, 13, 2], offsets_per_year=1)):
            plan = Plan.from_policy(pol)
            for n in (64, 1500):
                a = eng.evaluate_plans(pol, [plan] * n, 31, 500)
                b = eng.rollout_batch(pol, 31, n, first_episode_index=500, replay_mask=np.ones(n, np.uint8))
                _same_records(a, b, (helper, len(plan), n))
    finally:
        eng.close()


def test_round_trip_with_training(world):
    eng = Engine(world, device=0)
    try:
        eng.push(ActionWeights())
        n, period, seed, first = 256, 4, 61, 0
        pol = ActionWeights()
        for step in range(40):
            eng.device_step(seed, first, n, period, seed + first)
            first += n
            eng.pull(pol)
            if pol.get("has_best_actions") == 1 and step >= 2:
                break
        assert pol.get("has_best_actions") == 1
        eng.device_step(seed, first, n, period, seed + first)
        batch = eng.fetch(n)
        plan = Plan.from_policy(pol)
        for i in (first, first + period * 7):
            assert i % period == 0
            got = eng.evaluate_plans(pol, [plan], seed, i)
            _same_records(got, batch, i, [0], [i - first])
    finally:
        eng.close()


def test_evaluation_does_not_touch_training(world, engine, tmp_path):
    res = engine.rollout_batch(ActionWeights(), 5, 500)
    plans = [Plan.from_result(res, e % 500, str(e)) if e < 500 else Plan([l[::-1] for l in Plan.from_result(res, e % 500).best_actions],
                                                                         res.lists(e % 500, "def")) for e in range(1000)]
    out = []
    for evaluate in (False, True):
        eng = Engine(world, device=0)
        try:
            eng.push(ActionWeights())
            eng.track_best_result()
            eng.track_top_k(10)
            for step in range(20):
                eng.device_step(3, 1024 * step, 1024, 10, 3 + step)
                if evaluate and step == 9:      # (under a policy of its own: a pull is part of the training loop's host state)
                    r = eng.evaluate_plans(ActionWeights(), plans, 9, 0)
                    assert (r.status == 0).mean() > 0.9
            pol = ActionWeights(); eng.pull(pol)
            path = tmp_path / f"policy_{evaluate}.json"
            pol.save_to_file(path)
            text = re.sub(r'"timestamp": "[^"]*"', '"timestamp": ""', path.read_text())      # (the host's clock at the pull)
            idx, best = eng.fetch_best_result()
            rows, scores, index = eng.fetch_top_k()
            out.append((text, idx, best, rows, scores.tobytes(), index.tobytes()))
        finally:
            eng.close()
    (pa, ia, ba, ra, sa, xa), (pb, ib, bb, rb, sb, xb) = out
    assert pa == pb and ia == ib and sa == sb and xa == xb
    _same_records(ba, bb, "best_result")
    _same_records(ra, rb, "top-k")


def _run_dir(ck):
    runs = os.listdir(ck)
    assert len(runs) == 1, runs
    return os.path.join(ck, runs[0])


def test_cli_evaluates_plans(built, tmp_path):
    wd = World.from_json_dict(json.load(open(WORLD)))
    tb = O.OracleTables(HostTables(wd), len(wd.existing_x))
    ck = str(tmp_path / "train")
    out = subprocess.run([CLI, "--world", WORLD, "-n", "96", "--batch", "32", "--seed", "7", "-c", ck, "-i", "40", "-r", "1000"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rd = _run_dir(ck)
    latest = os.path.join(rd, "latest_weights.json")
    pol = ActionWeights.load_from_file(latest)
    eng = Engine(wd, device=0)
    try:
        res = eng.rollout_batch(pol, 99, 8)
    finally:
        eng.close()
    plans = [Plan.from_result(res, e, f"episode {e}") for e in range(5)]
    lines = [json.dumps({"name": p.name, **_schema(p)}) for p in plans]
    lines.insert(2, json.dumps({"name": "broken", "best_actions": {}}))
    jl = tmp_path / "plans.jsonl"
    jl.write_text("\n".join(lines) + "\n")
    args = ["--world", WORLD, "--evaluate-policy", latest, "--seed", "11", "--top-k", "3", "--batch", "2"]
    out = subprocess.run([CLI, *args, "--evaluate", str(jl), "-c", str(tmp_path / "bad")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 1 and 'line 3: missing "best_deficit_actions"' in out.stderr, out.stdout + out.stderr
    assert not (tmp_path / "bad").exists()
    del lines[2]
    jl.write_text("\n".join(lines) + "\n")
    for name, path, want in (("jsonl", str(jl), plans), ("ckpt", os.path.join(rd, "best_weights.json"), None)):
        ev = str(tmp_path / name)
        out = subprocess.run([CLI, *args, "--evaluate", path, "-c", ev], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Evaluated %d plans in" % (len(want) if want else 1) in out.stdout
        plans_dir = os.path.join(_run_dir(ev), "plans")
        want = want or Plan.load(path)
        rows = list(csv.DictReader(open(os.path.join(plans_dir, "index.csv"))))
        assert [r["plan"] for r in rows] == [str(j) for j in range(len(want))]
        refs = []
        for j, (p, r) in enumerate(zip(want, rows)):
            st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, p), 11 + j, replay=True)
            refs.append(ref)
            assert r["name"] == p.name and int(r["status"]) == st and int(r["n_generators"]) == ref.n_gens
            m = list(ref.metrics)
            assert [r[k] for k in ("final_net_emissions", "average_public_opinion", "total_cost", "power_reliability")] == ["%.17g" % v for v in m]
            assert r["score"] == "%.17g" % rank_score(m)
        order = sorted(range(len(want)), key=lambda j: (-rank_score(list(refs[j].metrics)), j))[:3]
        for rank, j in enumerate(order):
            f = os.path.join(plans_dir, "top_k", "%02d" % (rank + 1), "simulation_summary.csv")
            text = open(f).read()
            stamp = text.split("\n")[1].split(",", 1)[1]
            ref = refs[j]
            rec = BatchResult.alloc(1)
            rec.metrics[0] = list(ref.metrics); rec.yearly[0] = np.array([list(row) for row in ref.yearly]); rec.n_act[0] = list(ref.n_act)
            k = int(sum(ref.n_act)); rec.act_log[0, :k] = list(ref.act_log)[:k]
            assert text == OC.summary_csv_text(rec.metrics[0], rec.yearly[0], rec.n_act[0], rec.act_log[0], stamp), (name, rank)


def _schema(p):
    """A plan in the checkpoint schema, written the way eg_policy_save_json writes best lists."""
    from tests.test_plans import _action
    return {"best_actions": {str(2025 + y): [_action(a) for a in l] for y, l in enumerate(p.best_actions)},
            "best_deficit_actions": {str(2025 + y): [_action(a) for a in l] for y, l in enumerate(p.best_deficit_actions)}}
