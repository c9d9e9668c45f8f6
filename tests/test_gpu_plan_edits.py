"""GPU: plan edits (include/eirgrid_hip.h eg_evaluate_plan_edits; csrc/eg_plan_edits.h k_plan_edits; eg_plans.cpp).  Variant j of a
plan-edit batch is the base plan with edit j applied, evaluated exactly as eg_evaluate_plans evaluates the edited plan: the plan blocks
the device writes must give, record for record and byte for byte, what the blocks the host builds give — and what the tabled oracle
computes for the edited plan."""
import csv
import os
import re
import subprocess

import numpy as np
import pytest

from eirgrid_amd.engine import ActionWeights, Engine, HostTables, Plan, PlanEdit, rank_score, sensitivity_edits
from eirgrid_amd.world import World
from oracle import api as O
from tests.helpers import assert_episode_equal
from tests.test_gpu_plans import _engine, _oracle_plan, _run_dir, _same_records
from tests.test_gpu_replay_hoist import _full_script, _seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def _apply(plan, e):
    """Edit e applied to a copy of `plan`, written out here once more (not PlanEdit.apply: the test's own restatement)."""
    run = [list(l) for l in plan.best_actions]; dfc = [list(l) for l in plan.best_deficit_actions]
    l = (run, dfc)[e.list][e.year]
    if e.kind == "delete":
        l.pop(e.pos)
    elif e.kind == "replace":
        l[e.pos] = e.action
    elif e.kind == "insert":
        l[e.pos:e.pos] = [e.action]
    else:
        assert e.kind == "none"
    return Plan(run, dfc)


def _edit_set(plan, rng, extra=0):
    """`none`, then every kind at the first, a middle and the last position of a list, in the first and the last non-empty year, on both
    lists (an insert also behind the last entry; a list without entries: inserts into its first and last year), then `extra` random
    edits.  Deficit lists take what the repair loop can use: a generator at 100 % or DoNothing."""
    actions = ([3, 12, 14, 36, 45, 56, 57, 59, 60, 1], [24, 21, 36, 0, 60])
    edits = [PlanEdit()]
    for which, lists in enumerate((plan.best_actions, plan.best_deficit_actions)):
        years = [y for y, l in enumerate(lists) if l]
        for y in ([years[0], years[-1]] if years else [0, 25]):
            n = len(lists[y])
            for pos in sorted({0, n // 2, max(n - 1, 0)}):
                if n:
                    edits.append(PlanEdit("delete", which, y, pos))
                    edits.append(PlanEdit("replace", which, y, pos, int(rng.choice(actions[which]))))
                edits.append(PlanEdit("insert", which, y, pos, int(rng.choice(actions[which]))))
            edits.append(PlanEdit("insert", which, y, n, int(rng.choice(actions[which]))))
    for _ in range(extra):
        which = int(rng.integers(0, 2))
        lists = (plan.best_actions, plan.best_deficit_actions)[which]
        y = int(rng.integers(0, 26))
        n = len(lists[y])
        kind = str(rng.choice(["delete", "replace", "insert"])) if n else "insert"
        pos = int(rng.integers(0, n + 1 if kind == "insert" else n))
        edits.append(PlanEdit(kind, which, y, pos, int(rng.choice(actions[which]))))
    return edits


def _long_policy(seed=5):
    return _full_script(np.random.default_rng(seed), 9, [0, 4, 12, 7, 5, 1, 13, 2], offsets_per_year=1)


def _bases(engine):
    short, long_ = _seeded(engine), _long_policy()
    assert len(Plan.from_policy(short)) == 28 and len(Plan.from_policy(long_)) >= 200
    return [("short", short), ("long", long_)]


def _junk_plan():
    """Both lists full of CloseGenerator: a plan batch of these leaves no zero byte in the pool's lists, and masks and offsets of its own"""
    full = [[59] * 157 for _ in range(26)]
    full[0] += [59] * (4096 - 26 * 157)
    return Plan(full, full)


def _check_blocks(eng, pol, base, edits, what):
    """The plan blocks k_plan_edits writes against the blocks the host's write_lists builds for the edited plans, all 8 832 bytes of
    each (eg_debug_fetch_plan_block) — with the pool overwritten in between, so that nothing is left over from the host's blocks."""
    n = len(edits)
    eng.evaluate_plans(pol, [_apply(base, e) for e in edits], 1, 0)
    host = [eng.debug_fetch_plan_block(j) for j in range(n)]
    eng.evaluate_plans(pol, [_junk_plan()] * n, 1, 0)
    assert eng.debug_fetch_plan_block(n - 1)[640:].min() == 59
    eng.evaluate_plan_edits(pol, base, edits, 1, 0)
    for j in range(n):
        dev = eng.debug_fetch_plan_block(j)
        if dev.tobytes() != host[j].tobytes():
            bad = np.flatnonzero(dev != host[j])
            raise AssertionError(f"{what}: block {j} ({edits[j]}) differs at bytes {bad[:8].tolist()} ({len(bad)} in all)")


def _check_against_host_path(eng, pol, base, edits, seed, first, what):
    """(b): same_index = False against evaluate_plans of the edited plans; same_index = True against one-plan calls at `first`"""
    edited = [_apply(base, e) for e in edits]
    _check_blocks(eng, pol, base, edits, what)
    want = eng.evaluate_plans(pol, edited, seed, first)
    got = eng.evaluate_plan_edits(pol, base, edits, seed, first, same_index=False)
    _same_records(got, want, (what, "index + j"))
    got = eng.evaluate_plan_edits(pol, base, edits, seed, first, same_index=True)
    for j, p in enumerate(edited):
        one = eng.evaluate_plans(pol, [p], seed, first)
        _same_records(got, one, (what, "same index", j, edits[j]), [j], [0])
    return want


def test_an_edit_list_of_none_is_the_base_plan(world, engine):
    for name, pol in _bases(engine):
        base = Plan.from_policy(pol)
        for n in (1, 5, 300):
            want = engine.evaluate_plans(pol, [base] * n, 41, 700)
            for same in (False, True):
                got = engine.evaluate_plan_edits(pol, base, [PlanEdit()] * n, 41, 700, same_index=same)
                if same:      # every variant at index 700: plan 0 of the plan batch
                    _same_records(got, want, (name, n, same), list(range(n)), [0] * n)
                else:
                    _same_records(got, want, (name, n, same))
        cut = Plan([l[:len(l) // 2] for l in base.best_actions], [l[:1] for l in base.best_deficit_actions])      # (lists that run out: seeded draws)
        for pol2 in (pol, ActionWeights()):
            want = engine.evaluate_plans(pol2, [cut] * 3, 41, 700)
            got = engine.evaluate_plan_edits(pol2, cut, [PlanEdit()] * 3, 41, 700, same_index=False)
            _same_records(got, want, (name, "cut"))
            assert (want.n_draws > 0).all()
            got = engine.evaluate_plan_edits(pol2, cut, [PlanEdit()] * 3, 41, 701, same_index=True)
            for j in range(3):
                _same_records(got, want, (name, "cut, same index", j), [j], [1])


def test_blocks_are_write_lists_byte_for_byte(world, engine):
    """The edges no episode record shows: lists at and next to the 4 096-entry capacity (the byte shifted in behind a full list, the
    byte shifted out of one), years longer than a wave, an action that leaves or enters a year's masks, empty lists."""
    pol = ActionWeights()
    rng = np.random.default_rng(3)

    def lists(total, first_year):
        l = [[int(a) for a in rng.integers(0, 61, 150)] for _ in range(26)]
        l[first_year] += [int(a) for a in rng.integers(0, 61, total - 26 * 150)]
        return l
    full = Plan(lists(4096, 3), lists(4096, 25))
    edits = [PlanEdit()]
    for which in (0, 1):
        ly = (3, 25)[which]      # the year that holds the list's extra entries
        last = len((full.best_actions, full.best_deficit_actions)[which][ly]) - 1
        for y, pos in ((0, 0), (ly, 149), (ly, 150), (ly, last), (12, 64), (24, 0), (25, 149 if which == 0 else last)):
            edits += [PlanEdit("delete", which, y, pos), PlanEdit("replace", which, y, pos, int(rng.integers(0, 61)))]
    _check_blocks(engine, pol, full, edits, "full lists")
    almost = Plan(lists(4095, 0), lists(4095, 13))
    edits = [PlanEdit("insert", which, y, pos, a) for which in (0, 1) for y, pos, a in ((0, 0, 60), (25, 150, 0), (25, 0, 33), (13, 75, 7), (7, 64, 59))]
    _check_blocks(engine, pol, almost, edits, "one entry below the capacity")
    # masks: the only occurrence of an action deleted or replaced away, one of two occurrences deleted, a new action inserted, the same
    # action in the other list of the year (the first mask keeps it), an empty plan
    run = [[] for _ in range(26)]; dfc = [[] for _ in range(26)]
    run[4] = [5, 9, 5, 33]; dfc[4] = [9, 24]; run[25] = [60]
    small = Plan(run, dfc)
    edits = [PlanEdit("delete", 0, 4, 3), PlanEdit("delete", 0, 4, 0), PlanEdit("delete", 0, 4, 1), PlanEdit("replace", 0, 4, 3, 5), PlanEdit("insert", 0, 4, 2, 44),
             PlanEdit("delete", 1, 4, 0), PlanEdit("delete", 1, 4, 1), PlanEdit("replace", 1, 4, 1, 9), PlanEdit("insert", 1, 4, 2, 63 - 3), PlanEdit("delete", 0, 25, 0),
             PlanEdit("insert", 1, 0, 0, 24), PlanEdit("insert", 0, 24, 0, 0), PlanEdit()]
    _check_blocks(engine, pol, small, edits, "masks")
    empty = Plan([[] for _ in range(26)], [[] for _ in range(26)])
    _check_blocks(engine, pol, empty, [PlanEdit(), PlanEdit("insert", 0, 0, 0, 1), PlanEdit("insert", 1, 25, 0, 24)], "empty base")


@pytest.mark.parametrize("helper", ["0", "all"])
def test_edits_are_the_host_built_plans(world, engine, helper):
    rng = np.random.default_rng(11)
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        for name, pol in _bases(engine):
            base = Plan.from_policy(pol)
            edits = _edit_set(base, rng)
            kinds = {(e.kind, e.list) for e in edits}
            assert kinds >= {(k, w) for k in ("delete", "replace", "insert") for w in (0, 1)}, kinds
            for pol2 in (pol, ActionWeights()):      # (under a fresh policy the fallback draws come from other tables)
                res = _check_against_host_path(eng, pol2, base, edits, 77, 3000, (helper, name))
                assert (res.status == 0).all()
            assert len({res.metrics[j].tobytes() for j in range(len(edits))}) > 3      # (the edits matter)
    finally:
        eng.close()


def test_every_variant_is_the_oracles_replay_of_the_edited_plan(world, engine):
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    rng = np.random.default_rng(2031)
    eng = _engine(world, EIRGRID_HELPER_WAVES="0")
    try:
        for name, pol in _bases(engine):
            base = Plan.from_policy(pol)
            edits = _edit_set(base, rng, extra=40)[:80]
            assert len(edits) >= 64
            seed, first = 1234, 90_000
            for same in (True, False):      # (every edit at the shared index; the first 16 once more at an index of their own)
                got = eng.evaluate_plan_edits(pol, base, edits, seed, first, same_index=same)
                small = engine.evaluate_plan_edits(pol, base, edits, seed, first, same_index=same)      # (the small-batch kernel)
                for j, e in enumerate(edits if same else edits[:16]):
                    st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, _apply(base, e)), seed + first + (0 if same else j), replay=True)
                    assert st == 0, (name, j, e)      # no case skipped: every variant of these bases finishes
                    assert_episode_equal(got, j, ref, f"{name}, same_index {same}, edit {j} {e}")
                    assert_episode_equal(small, j, ref, f"{name} (small-batch kernel), same_index {same}, edit {j} {e}")
    finally:
        eng.close()


def _sized_plan(n):
    """n best_actions entries over the 26 years (generators of four types), four deficit actions a year"""
    rng = np.random.default_rng(n)
    per = [n // 26 + (1 if y < n % 26 else 0) for y in range(26)]
    run = [[int(3 * rng.choice([0, 4, 12, 7]) + rng.integers(0, 3)) for _ in range(k)] for k in per]
    return Plan(run, [[24, 36, 21, 24] for _ in range(26)])


@pytest.mark.parametrize("helper", ["0", "all"])
def test_variants_cross_the_short_long_boundary(world, helper):
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        pol = ActionWeights()
        for n, kind in ((97, "delete"), (96, "insert")):
            base = _sized_plan(n)
            assert len(base) == n
            edits = [PlanEdit()]
            for y in (0, 12, 25):
                k = len(base.best_actions[y])
                edits += [PlanEdit(kind, 0, y, p, 13) for p in (0, k // 2, k - 1)]
                edits += [PlanEdit("replace", 0, y, 0, 13), PlanEdit(kind, 1, y, 1, 24)]      # (these keep the base's length: the other route)
            lengths = {len(_apply(base, e)) for e in edits}
            assert lengths == {96, 97}, lengths
            res = _check_against_host_path(eng, pol, base, edits, 19, 64, (helper, n, kind))
            assert (res.status == 0).all()
    finally:
        eng.close()


def test_an_overflowing_variant_reports_it_and_leaves_the_others_alone(world, engine):
    # A replay records every action twice, the repair loop's actions included: 2 042 entries — twenty nuclear plants in 2025,
    # DoNothing otherwise — and the year's deficit actions fill the 4 096 entries of the run record to the last one or two (the tabled
    # oracle: 4 095 or 4 096 recorded for seeds 23..29); one more entry overflows it.
    run = [[60] * 78 for _ in range(26)]
    run[0] = [15] * 20 + [60] * (2042 - 25 * 78 - 20)
    base = Plan(run, [[24] for _ in range(26)])
    assert len(base) == 2042
    edits = [PlanEdit(), PlanEdit("insert", 0, 25, 78, 60), PlanEdit("delete", 0, 0, 5), PlanEdit("replace", 0, 13, 7, 3), PlanEdit("insert", 0, 0, 0, 60),
             PlanEdit("delete", 1, 4, 0), PlanEdit()]
    pol = ActionWeights()
    want = engine.evaluate_plans(pol, [_apply(base, e) for e in edits], 23, 0)
    got = engine.evaluate_plan_edits(pol, base, edits, 23, 0, same_index=False)
    assert got.status.tolist() == want.status.tolist()
    assert got.status[1] == -1 and got.status[4] == -1, got.status      # EG_EP_OVERFLOW in the variant's own status
    ok = got.status == 0
    assert ok.tolist() == [True, False, True, True, False, True, True], got.status
    for name in ("status", "metrics", "n_gens", "n_offsets", "n_draws"):
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
    _same_records(got, want, "beside overflowing variants", ok, ok)


def test_edit_evaluations_do_not_touch_training(world, engine, tmp_path):
    pol_eval = _long_policy(9)
    base = Plan.from_policy(pol_eval)
    edits = sensitivity_edits(base, replace_with=[12])
    out = []
    for evaluate in (False, True):
        eng = Engine(world, device=0)
        try:
            eng.push(ActionWeights())
            eng.track_best_result()
            eng.track_top_k(10)
            for step in range(6):
                eng.device_step(3, 1024 * step, 1024, 10, 3 + step)
                if evaluate and step < 5:
                    r = eng.evaluate_plan_edits(pol_eval, base, edits, 9, 0, same_index=bool(step % 2))
                    assert (r.status == 0).all()
            batch = eng.fetch(1024)
            pol = ActionWeights(); eng.pull(pol)
            path = tmp_path / f"policy_{evaluate}.json"
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
    from eirgrid_amd.engine import Group
    from eirgrid_amd._native import EirgridError
    g = Group(world, devices=(0, 0))
    try:
        with pytest.raises(EirgridError, match="rank of an eg_group"):
            g.ranks[0].evaluate_plan_edits(ActionWeights(), _sized_plan(30), [PlanEdit()], 1)
    finally:
        g.close()


def test_cli_writes_the_sensitivity_table(built, tmp_path):
    import json
    wd = World.from_json_dict(json.load(open(WORLD)))
    ck = str(tmp_path / "train")
    out = subprocess.run([CLI, "--world", WORLD, "-n", "512", "--batch", "64", "--seed", "7", "-c", ck, "-i", "40", "-r", "1000", "--stop-after", "128"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    rd = _run_dir(ck)
    latest = os.path.join(rd, "latest_weights.json")      # (what an interrupted run leaves behind)
    best = latest
    base = Plan.load(best)[0]
    n_entries = sum(len(l) for l in base.best_actions) + sum(len(l) for l in base.best_deficit_actions)
    assert n_entries > 0
    pol = ActionWeights.load_from_file(latest)
    out = subprocess.run([CLI, "--world", WORLD, "--gpus", "2", "--sensitivity", best], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--sensitivity runs on one device" in out.stderr
    eng = Engine(wd, device=0)
    try:
        for replace in (None, [12, 60]):
            sv = str(tmp_path / ("sens_%d" % len(replace or [])))
            args = [CLI, "--world", WORLD, "--evaluate-policy", latest, "--seed", "11", "--batch", "50", "--sensitivity", best, "-c", sv]
            if replace:
                args += ["--sensitivity-replace", ",".join(map(str, replace))]
            out = subprocess.run(args, capture_output=True, text=True, timeout=600)
            assert out.returncode == 0, out.stdout + out.stderr
            rows = list(csv.DictReader(open(os.path.join(_run_dir(sv), "sensitivity", "index.csv"))))
            want = eng.plan_sensitivity(pol, base, 11, replace_with=replace)
            assert len(rows) == 1 + n_entries + len(replace or []) * len(base) == len(want.edits)
            assert list(rows[0].keys()) == ("edit,kind,list,year,pos,action_before,action_after,status,net_emissions,public_opinion,total_cost,"
                                            "power_reliability,score,d_net_emissions,d_public_opinion,d_total_cost,d_score").split(",")
            assert rows[0]["kind"] == "none" and [rows[0][k] for k in ("d_net_emissions", "d_public_opinion", "d_total_cost", "d_score")] == ["0"] * 4
            for j, (r, e) in enumerate(zip(rows, want.edits)):
                assert int(r["edit"]) == j and r["kind"] == e.kind and int(r["status"]) == want.status[j]
                if e.kind != "none":
                    lists = (base.best_actions, base.best_deficit_actions)[e.list]
                    assert (r["list"], int(r["year"]), int(r["pos"])) == (("best_actions", "best_deficit_actions")[e.list], 2025 + e.year, e.pos)
                    assert int(r["action_before"]) == lists[e.year][e.pos]
                    assert r["action_after"] == ("" if e.kind == "delete" else str(e.action))
                m = want.metrics[j]
                assert [r[k] for k in ("net_emissions", "public_opinion", "total_cost", "power_reliability")] == ["%.17g" % v for v in m]
                assert r["score"] == "%.17g" % want.score[j] == ("%.17g" % rank_score(m) if want.status[j] == 0 else "nan")
                # (NaN where the base or the variant failed, in both interfaces)
                assert [r[k] for k in ("d_net_emissions", "d_public_opinion", "d_total_cost")] == ["%.17g" % v for v in want.d_metrics[j][:3]]
                assert r["d_score"] == "%.17g" % want.d_score[j]
    finally:
        eng.close()
