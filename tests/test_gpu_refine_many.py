"""GPU: many plans refined in one call (include/eirgrid_hip.h eg_refine_plans; csrc/eg_refine.cpp, csrc/eg_refine_many.h).  The
specification exists already: per plan the result is eg_refine_plan's for that plan alone, bit for bit — so every test compares with
Engine.refine_plan on the same engine (the same loop over that plan alone: a launch of another shape, of its variants only) and with the
definition restated over the tabled oracle (tests/test_refine.py refine_restated), never with the call itself.  The two kernels are held on their own as well: the blocks
k_plan_edits_many writes against the host's, and k_refine_pick_many on crafted batches cut into segments.

(The bases' trajectories do not depend on the policy's weights — no variant of them draws a fallback — so one call under one policy is
compared with the oracle runs tests/test_refine.py caches per base.)"""
import csv
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, BatchResult, Engine, Plan, PlanEdit, PlanSet, _refine_opts
from eirgrid_amd.world import World
from tests.helpers import assert_episode_equal
from tests.test_crafted_folds import FAILED, level_metrics, refine_block, refine_pick
from tests.test_gpu_plan_edits import _long_policy, _sized_plan
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plans import _engine, _run_dir, _same_records
from tests.test_gpu_refine import _assert_same_trajectory, _overflow_base
from tests.test_refine import SEED, OracleEvaluator, apply_edit, oracle_run, refine_restated, round_edits, short_policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
LAUNCH = "EIRGRID_REFINE_LAUNCH_VARIANTS"
REPLACE = (12,)

_restated = {}


def _bases(world):
    """(the policy the calls run under, the short base, the long base, their cached oracle evaluators)"""
    pol_s, short, ev_s, _ = oracle_run(world, "short, mode 2")
    pol_l, long_, ev_l, _ = oracle_run(world, "long, mode 2")
    assert (len(short), len(long_)) == (67, 272)
    return pol_l, short, long_, ev_s, ev_l


def _oracle(world, which, mode, max_rounds):
    """refine_restated over the base's cached OracleEvaluator with the tests' options (REPLACE), once per session"""
    key = (which, mode, max_rounds)
    if key not in _restated:
        pol, short, long_, ev_s, ev_l = _bases(world)
        _restated[key] = refine_restated(ev_s if which == "short" else ev_l, short if which == "short" else long_, mode, max_rounds, REPLACE)
    return _restated[key]


def _failing_base():
    return apply_edit(_overflow_base(), PlanEdit("insert", 0, 25, 78, 60))


def bits(x):
    return np.float64(x).tobytes()


def _assert_same_as_alone(got, alone, what, same_shape=True):
    """one tuple of refine_plans against refine_plan's for the plan alone: _assert_same_trajectory's comparison, and the record — every
    used byte of it.  n_chunks, the traffic counter of the search that really ran (include/eirgrid_hip.h), is compared only where both
    sides ran in the same launch shape (EIRGRID_HELPER_WAVES forced): the small-batch and the throughput kernels request different chunks
    for the same placements, and which of them a launch runs depends on its size."""
    plan, steps, stop, start, rec = got
    aplan, asteps, astop, astart, arec = alone
    assert stop == astop and len(steps) == len(asteps), (what, stop, astop, len(steps), len(asteps))
    assert bits(start) == bits(astart) or (np.isnan(start) and np.isnan(astart)), (what, start, astart)
    for r, (s, a) in enumerate(zip(steps, asteps)):
        assert (s.edit, s.variant, s.n_variants, s.n_failed) == (a.edit, a.variant, a.n_variants, a.n_failed), (what, r, s, a)
        assert bits(s.score) == bits(a.score) and s.metrics.tobytes() == a.metrics.tobytes(), (what, r, s, a)
    assert plan == aplan and plan.name == aplan.name, what
    assert (rec is None) == (arec is None), what
    if rec is not None:
        for name in _ALL_FIELDS + (("n_chunks",) if same_shape else ()):
            assert _used(rec, name).tobytes() == _used(arec, name).tobytes(), (what, "the refined plan's record", name)


def _alone(eng, pol, plans, seed, index, mode, max_rounds, **kw):
    return [eng.refine_plan(pol, p, seed, index, mode, max_rounds, **kw) for p in plans]


# ---------------------------------------------------------------- 1, 2: the definition
@pytest.mark.parametrize("helper", ["0", "all"])
def test_every_plan_is_refined_as_if_alone(world, helper):
    pol, short, long_, ev_s, ev_l = _bases(world)
    plans = [Plan(short.best_actions, short.best_deficit_actions, "short"), Plan(long_.best_actions, long_.best_deficit_actions, "long"),
             Plan(short.best_actions, short.best_deficit_actions, "short again"), _failing_base()]
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        got = eng.refine_plans(pol, plans, SEED, 0, 2, 4, replace_with=REPLACE)
        alone = _alone(eng, pol, plans, SEED, 0, 2, 4, replace_with=REPLACE)
        assert len(got) == 4
        for p in range(4):
            _assert_same_as_alone(got[p], alone[p], (helper, "plan", p))
        for p, which, ev in ((0, "short", ev_s), (1, "long", ev_l), (2, "short", ev_s)):
            _assert_same_trajectory(got[p], _oracle(world, which, 2, 4), (helper, which, "tabled oracle"))
            assert_episode_equal(got[p][4], 0, ev.record(got[p][0]), f"{which}: the refined plan's record")
        # what the CPU cases establish: the short base takes one step and stops at the optimum, the long one takes its four deletes
        assert (got[0][2], len(got[0][1])) == ("local_optimum", 1) and (got[1][2], [s.variant for s in got[1][1]]) == ("max_rounds", [18, 77, 102, 105])
        assert [s.n_variants for s in got[0][1]] == [239] and [s.n_variants for s in got[1][1]] == [649, 647, 645, 643]      # (272 replaces beside the 377)
        assert all(s.edit.kind == "delete" and s.edit.list == 0 for s in got[1][1])
        # the duplicate gives the duplicate result, under its own name
        _assert_same_as_alone(got[2], (Plan(got[0][0].best_actions, got[0][0].best_deficit_actions, "short again"),) + got[0][1:], "the duplicate")
        assert [g[0].name for g in got] == ["short", "long", "short again", ""]
        # the failing base: no steps, a NaN start, the plan as given; and the plans stopped in three different rounds (0, 1 and 3)
        assert got[3][2] == "base_failed" and got[3][1] == [] and np.isnan(got[3][3]) and got[3][0] == plans[3] and got[3][4] is None
        assert sorted(len(g[1]) + (g[2] == "local_optimum") for g in got[:3]) == [2, 2, 4]
        # ... and its row of `out` is left as the caller passed it
        res = _raw_out(eng, pol, [plans[0], plans[3]], SEED, 0, 2, 4, 0x5A)
        for f in ("metrics", "yearly", "status", "run_log", "n_draws"):
            assert (getattr(res, f)[1:2].view(np.uint8) == 0x5A).all(), f
        assert res.metrics[0].tobytes() == got[0][4].metrics[0].tobytes() and res.status[0] == 0
    finally:
        eng.close()


def _raw_out(eng, pol, plans, seed, index, mode, max_rounds, fill):
    """eg_refine_plans once more, its `out` rows prefilled with the byte `fill`"""
    ps = PlanSet(plans)
    n = len(plans)
    ro, keep = _refine_opts(mode, max_rounds, REPLACE, None)
    steps = (N.EgRefineStep * (n * max_rounds))()
    n_steps = np.zeros(n, np.int32); stop = np.zeros(n, np.int32); start = np.zeros(n)
    res = BatchResult.alloc(n)
    for f in ("metrics", "yearly", "status", "n_run", "n_def", "n_act", "run_log", "def_log", "act_log", "n_gens", "gen_cell", "gen_pack", "n_offsets", "off_pack",
              "n_draws", "bytes_moved", "n_chunks"):
        getattr(res, f).view(np.uint8)[...] = fill
    snap = pol.snapshot(); opts = eng._opts(True, False, True); out = res.struct()
    refined = C.POINTER(N.EgPlanSet)()
    L = N.lib()
    N.check(L.eg_refine_plans(eng.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.byref(ro), C.c_uint64(seed), C.c_uint64(index), C.byref(refined), steps,
                              n_steps.ctypes.data_as(C.POINTER(C.c_int32)), stop.ctypes.data_as(C.POINTER(C.c_int32)), start.ctypes.data_as(C.POINTER(C.c_double)),
                              C.byref(out)), "eg_refine_plans")
    L.eg_plans_free(refined)
    assert stop[n - 1] == N.REFINE_BASE_FAILED
    return res


def test_mode_1_both_plans_run_out_of_rounds(world, engine):
    pol, short, long_, ev_s, ev_l = _bases(world)
    plans = [short, long_]
    got = engine.refine_plans(pol, plans, SEED, 0, 1, 4, replace_with=REPLACE)
    alone = _alone(engine, pol, plans, SEED, 0, 1, 4, replace_with=REPLACE)
    for p, (which, ev) in enumerate((("short", ev_s), ("long", ev_l))):
        _assert_same_as_alone(got[p], alone[p], ("mode 1", which), same_shape=False)      # (the session's engine picks the kernel by launch size)
        _assert_same_trajectory(got[p], _oracle(world, which, 1, 4), ("mode 1", which, "tabled oracle"))
        assert_episode_equal(got[p][4], 0, ev.record(got[p][0]), f"{which}: the refined plan's record")
        assert got[p][2] == "max_rounds" and len(got[p][1]) == 4


# ---------------------------------------------------------------- 3: packing
def test_the_packing_into_launches_does_not_matter(world, engine, monkeypatch):
    pol, short, long_, ev_s, ev_l = _bases(world)
    plans = [short, long_, short]      # 239, 649, 239 variants in round 0
    runs = {}
    for cap in ("300", "700", "900", None):      # every plan alone; again (239 + 649 > 700); short + long, then short; all three in one launch
        if cap is None:
            monkeypatch.delenv(LAUNCH, raising=False)
        else:
            monkeypatch.setenv(LAUNCH, cap)
        runs[cap] = engine.refine_plans(pol, plans, SEED, 0, 2, 4, replace_with=REPLACE)
    for cap in ("300", "700", "900"):
        for p in range(3):
            _assert_same_as_alone(runs[cap][p], runs[None][p], ("launches of", cap, "plan", p), same_shape=False)
    for p, which in enumerate(("short", "long", "short")):
        _assert_same_trajectory(runs["300"][p], _oracle(world, which, 2, 4), (which, "tabled oracle"))
    # what stays behind is the last launch's variants: the long plan's last round alone (it outlives the short ones)
    assert N.lib().eg_last_batch_size(engine.h) == 643


# ---------------------------------------------------------------- 4: the routing boundary inside a shared launch
@pytest.mark.parametrize("helper", ["0", "all"])
def test_a_plan_crosses_the_short_long_boundary_beside_another(world, helper):
    pol = ActionWeights()
    _, short, _, _, _ = _bases(world)
    base = _sized_plan(97)
    key = ("97 down",)
    if key not in _restated:
        ev = OracleEvaluator(world, pol, 19, 64)
        _restated[key] = (ev, refine_restated(ev, base, 1, 2, (), (14,)))
    ev, want = _restated[key]
    lengths, plan = [len(base)], base
    for s in want[1]:
        plan = apply_edit(plan, s[0]); lengths.append(len(plan))
    assert lengths == [97, 96, 95], lengths      # the crossing happened (picked with the oracle on the CPU)
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        plans = [base, short]
        got = eng.refine_plans(pol, plans, 19, 64, 1, 2, append_with=(14,))
        alone = _alone(eng, pol, plans, 19, 64, 1, 2, append_with=(14,))
        for p in range(2):
            _assert_same_as_alone(got[p], alone[p], (helper, "plan", p))
        _assert_same_trajectory(got[0], want, (helper, "the 97-action plan, tabled oracle"))
        assert_episode_equal(got[0][4], 0, ev.record(got[0][0]), "the refined plan's record")
    finally:
        eng.close()


# ---------------------------------------------------------------- 5: the blocks k_plan_edits_many writes
def test_the_variants_blocks_are_the_hosts(world, engine):
    pol, short, long_, ev_s, ev_l = _bases(world)
    plans = [short, _sized_plan(97), long_]
    engine.refine_plans(pol, plans, SEED, 0, 1, 1, replace_with=REPLACE)      # one round: its variants stay behind, a segment per plan
    picks, first = [], 0
    for plan in plans:
        edits = round_edits(plan, REPLACE)
        len0, len1 = len(plan), sum(len(l) for l in plan.best_deficit_actions)
        assert len(edits) == 1 + 2 * len0 + len1
        for j in (0, len(edits) - 1, 1 + len0 + len1 // 2, 1 + len0 + len1 + len0 // 3):      # the base, the last replace, a list-1 delete, a replace
            picks.append((first + j, plan, edits[j]))
        assert (edits[1 + len0 + len1 // 2].kind, edits[1 + len0 + len1 // 2].list) == ("delete", 1) and edits[1 + len0 + len1 + len0 // 3].kind == "replace"
        first += len(edits)
    assert N.lib().eg_last_batch_size(engine.h) == first == 239 + 299 + 649
    dev = [engine.debug_fetch_plan_block(j).copy() for j, _, _ in picks]
    for (j, plan, edit), d in zip(picks, dev):
        engine.evaluate_plans(pol, [apply_edit(plan, edit)], SEED, 0)
        host = engine.debug_fetch_plan_block(0)
        assert d.tobytes() == host.tobytes(), (j, edit, np.flatnonzero(d != host)[:8])


# ---------------------------------------------------------------- 6: k_refine_pick_many on crafted batches
SEGMENTS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def _base_words(s):
    w = np.arange(N.PLAN_BLOCK_BYTES // 4, dtype=np.uint64)
    b = (0xBA5E0000 + (s << 8) + w) & np.uint64(0xFFFFFFFF)
    b[130], b[158] = 7, 5
    return b.astype("<u4").view(np.uint8)


def _crafted():
    """5 314 records in eight segments (SEGMENTS), by segment:
      0  the base alone
      1  random levels and failures; its LAST record far above everything in segment 2
      2  levels up to 50 only, between a larger score just before it and one just after it
      3  its maximum tied at its first and its last variant: the base stays, the block is untouched
      4  a failed base (winner -1) in front of segment 5, whose base is fine; its last record scores far above segment 5
      5  NaN metrics, statuses other than 0 and a candidate that scores -inf (mode 1)
      6  the winner in the one-record last trip
      7  the winner in the last stride trip, failures in that trip"""
    rng = np.random.default_rng(2049)
    first = np.concatenate([[0], np.cumsum(SEGMENTS)[:-1]]).astype(np.uint32)
    n = int(np.sum(SEGMENTS))
    level = rng.integers(0, 50, n).astype(np.float64)
    status = np.where(rng.uniform(size=n) < 0.2, FAILED, 0).astype(np.int32)
    status[first] = 0
    f = [int(x) for x in first]
    status[f[2]:f[4]] = 0
    level[f[2] - 1] = 5000.0; status[f[2] - 1] = 0
    level[f[3]] = 100.0; level[f[4] - 1] = 100.0
    status[f[4]] = FAILED; level[f[5] - 1] = 9000.0; status[f[5] - 1] = 0
    level[f[6] + 1024] = 7000.0; status[f[6] + 1024] = 0
    level[f[7] + 2048] = 7000.0; status[f[7] + 2048] = 0; status[f[7] + 2040:f[7] + 2048] = FAILED; level[f[7] + 2047] = 8000.0
    m = level_metrics(level)
    m[f[5] + 3:f[6]:7, :2] = (-1.0, np.nan)                # a NaN score in mode 1
    m[f[5] + 10] = (-5.0, -np.inf, 1e10, 1.0)              # -inf in mode 1: a candidate all the same
    status[f[5] + 10] = 0
    return first, np.array(SEGMENTS, np.uint32), status, m


@pytest.mark.parametrize("mode", (1, 2))
def test_crafted_segments_are_picked_one_by_one(engine, mode):
    first, count, status, m = _crafted()
    engine._debug_load_batch(m, status, 0)
    entries, bases = engine._debug_refine_pick_many(first, count, mode)
    winners = []
    for s, (f, n) in enumerate(zip(first.tolist(), count.tolist())):
        e = entries[s]
        winner, n_failed, score, base_ok, base_score = refine_pick(status[f:f + n], m[f:f + n], mode)
        assert n_failed == int(((status[f:f + n] != 0) | np.isnan([_score(r, mode) for r in m[f:f + n]])).sum())
        assert (e.winner, e.n_failed, e.base_ok, e.n) == (winner, n_failed, base_ok, n), (s, e.winner, e.n_failed, e.base_ok, e.n, winner, n_failed, base_ok)
        w = f + max(winner, 0)
        assert list(e.edit) == [w, ~w & 0xFFFFFFFF], (s, list(e.edit))
        assert bits(e.score) == bits(score), (s, e.score, score)
        assert bytes(e.metrics) == np.ascontiguousarray(m[w]).tobytes() and bytes(e.base_metrics) == np.ascontiguousarray(m[f]).tobytes(), s
        assert (e.off26, e.offd26) == (w % 4097, (w // 3) % 4097), (s, e.off26, e.offd26)
        assert (np.isnan(e.base_score) and np.isnan(base_score)) or bits(e.base_score) == bits(base_score), (s, e.base_score, base_score)
        want = refine_block(w) if winner > 0 else _base_words(s)
        assert bases[s].tobytes() == want.tobytes(), (s, "the base block")
        winners.append(winner)
    assert winners[0] == 0 and winners[1] == 62 and winners[3] == 0 and winners[4] == -1 and winners[6] == 1024 and winners[7] == 2048, winners
    assert 0 <= winners[2] < 64 and 0 <= winners[5] < 1024 and m[int(first[2]) + winners[2], 0] >= 500000.0 - 50.0      # no neighbour's score won them
    if mode == 1:
        assert np.isneginf(_score(m[int(first[5]) + 10], 1)) and status[int(first[5]) + 10] == 0


def _score(row, mode):
    from eirgrid_amd.engine import rank_score
    return rank_score(np.ascontiguousarray(row), mode == 2)


def test_the_pick_hook_checks_its_segments(engine):
    first, count, status, m = _crafted()
    engine._debug_load_batch(m, status, 0)
    with pytest.raises(N.EirgridError, match="tiling"):
        engine._debug_refine_pick_many(first[::-1].copy(), count, 1)
    with pytest.raises(N.EirgridError, match="cover"):
        engine._debug_refine_pick_many(first[:-1], count[:-1], 1)


# ---------------------------------------------------------------- 7, 8: not training; no group form
def test_refine_plans_calls_do_not_touch_training(world, tmp_path):
    pol_eval = _long_policy(9)
    bases = [Plan.from_policy(pol_eval), _sized_plan(40)]
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
                    r = eng.refine_plans(pol_eval, bases, 9, 0, 1 + step % 2, 2, replace_with=[12] if step % 2 else None)
                    assert len(r) == 2 and len(r[0][1]) >= 1
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
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        with pytest.raises(N.EirgridError, match="rank of an eg_group"):
            g.ranks[0].refine_plans(ActionWeights(), [_sized_plan(30), _sized_plan(31)], 1)
        L = N.lib()
        buf = np.zeros(N.PLAN_BLOCK_BYTES, np.uint8); seg = np.array([0, 1], np.uint32)
        rc = L.eg_debug_refine_pick_many(g.ranks[0].h, 1, seg.ctypes.data_as(C.POINTER(C.c_uint32)), seg[1:].ctypes.data_as(C.POINTER(C.c_uint32)), 1,
                                         buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == N.EG_ERR_BAD_ARG and "eg_group" in L.eg_last_error().decode()
    finally:
        g.close()


# ---------------------------------------------------------------- 9: the script
def test_the_front_script_writes_what_refine_plans_returns(built, tmp_path):
    wd = World.from_json_dict(json.load(open(WORLD)))
    pol = short_policy()
    bases = [Plan.from_policy(pol, "short"), Plan.from_policy(_script_policy(), "second")]
    ckpt = str(tmp_path / "policy.json")
    pol.save_to_file(ckpt)
    pol = ActionWeights.load_from_file(ckpt)      # (as the tools see it: a checkpoint carries no count table)
    plan_file = str(tmp_path / "bases.jsonl")
    Plan.save(plan_file, bases)
    out_dir = str(tmp_path / "front")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "refine_front.py"), "--world", WORLD, "--plans", plan_file, "--policy", ckpt, "--seed", str(SEED),
                          "--rounds", "3", "--replace", "12", "--append", "14", "--out", out_dir], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    eng = Engine(wd, device=0)
    try:
        want = eng.refine_plans(pol, bases, SEED, 0, 1, 3, replace_with=[12], append_with=[14])
    finally:
        eng.close()
    d = os.path.join(out_dir, "refine")
    refined = os.path.join(d, "refined.jsonl")
    back = Plan.load(refined)
    assert back == [w[0] for w in want] and [p.name for p in back] == [b.name for b in bases]
    index = list(csv.DictReader(open(os.path.join(d, "index.csv"))))
    assert list(index[0].keys()) == "plan,name,stop,steps,start_score,final_score,net_emissions,public_opinion,total_cost,power_reliability".split(",")
    assert len(index) == 2 and sum(len(w[1]) for w in want) >= 2
    for p, (row, (plan, steps, stop, start, rec)) in enumerate(zip(index, want)):
        assert (row["plan"], row["name"], row["stop"], row["steps"]) == (str(p), bases[p].name, stop, str(len(steps)))
        assert row["start_score"] == "%.17g" % start and row["final_score"] == "%.17g" % (steps[-1].score if steps else start)
        assert [row[k] for k in ("net_emissions", "public_opinion", "total_cost", "power_reliability")] == ["%.17g" % v for v in rec.metrics[0]]
    rows = list(csv.DictReader(open(os.path.join(d, "trajectories.csv"))))
    assert list(rows[0].keys()) == ("plan,round,kind,list,year,pos,action,variant,n_variants,n_failed,score,net_emissions,public_opinion,total_cost,"
                                    "power_reliability").split(",")
    expect = []
    for p, (plan, steps, stop, start, rec) in enumerate(want):
        expect.append([str(p), "start", "none", "", "", "", "", "0", "", "", "%.17g" % start, "", "", "", ""])
        for r, s in enumerate(steps):
            e = s.edit
            expect.append([str(p), str(r), e.kind, ("best_actions", "best_deficit_actions")[e.list], str(2025 + e.year), str(e.pos), "" if e.kind == "delete" else str(e.action),
                           str(s.variant), str(s.n_variants), str(s.n_failed), "%.17g" % s.score] + ["%.17g" % v for v in s.metrics])
    assert [list(r.values()) for r in rows] == expect
    ev = str(tmp_path / "evaluate")
    run = subprocess.run([CLI, "--world", WORLD, "--evaluate-policy", ckpt, "--seed", str(SEED), "--evaluate", refined, "-c", ev], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    scored = list(csv.DictReader(open(os.path.join(_run_dir(ev), "plans", "index.csv"))))
    assert [(r["status"], r["score"]) for r in scored] == [("0", row["final_score"]) for row in index]


def _script_policy():
    """a second full script (tests/test_gpu_replay_hoist.py _full_script): its replay draws no fallback, so the plan scores the same at every
    global index — `--evaluate` scores plan j at index j, the refinement every plan at index 0"""
    from tests.test_gpu_replay_hoist import _full_script
    return _full_script(np.random.default_rng(11), 2, [0, 4, 12, 7], offsets_per_year=1)
