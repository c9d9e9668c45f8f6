"""GPU: the Pareto archive under the capacity rule "keep spread" (include/eirgrid_hip.h EG_PARETO_KEEP_SPREAD; csrc/eg_pareto.h
k_pareto_spread) against its restatement, tests/test_pareto_spread.py SpreadFront — crafted fronts through eg_debug_pareto_fold (lines
beyond the capacity, a surface folded in three batches, lattices full of ties, degenerate coordinates, a whole batch), real episodes,
the breed and explore searches against their host loops, the refusals and the user script.  Indices, metrics bytes, score bytes and
n_dropped are compared exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_pareto import RECORD_FIELDS, _antichain, _lattice, _names, _ok, _score, _train, check, same
from tests.test_pareto import oriented, split7
from tests.test_pareto_spread import KEEP_SPREAD, SpreadFront, preference, spread_select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
ALL = ("emissions", "opinion", "cost", "reliability")
CUTS = (5, 13, 20)
SEED, INDEX = 91, 7
SAMPLE = 1      # the sampling seed of the four plans the searches start from (tests/test_gpu_breed.py SAMPLE_CAP, tests/test_gpu_explore.py likewise)
pytestmark = pytest.mark.gpu


@pytest.fixture
def engine(engine):
    """The session's engine, with tracking off again for whoever uses it next."""
    yield engine
    engine.track_pareto(0)


@pytest.fixture(scope="module")
def eng(built):
    from eirgrid_amd.engine import Engine
    from eirgrid_amd.world import World
    e = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sampled(eng):
    from eirgrid_amd.engine import ActionWeights, Plan
    pol = ActionWeights()
    res = eng.rollout_batch(pol, SAMPLE, 4)
    return pol, [Plan.from_result(res, e, f"sampled {e}") for e in range(4)]


# ---------------------------------------------------------------- 1: lines beyond the capacity
@pytest.mark.parametrize("n,cap", [(257, 256), (300, 256), (3000, 8), (3000, 1)])
def test_line_antichains(engine, n, cap):
    """(257, 256) drops exactly one; (3000, 8) has more alive entries than the workgroup has threads; no n is a multiple of 64.  The
    points are evenly spaced, so many distances tie and the order of preference decides."""
    m = _antichain(n, n + cap)
    engine.track_pareto(cap, ("emissions", "cost"), keep="spread")
    ref = SpreadFront(cap, 5, _score()).fold(m, _ok(n), 0)
    engine._debug_pareto_fold(m, _ok(n), 0)
    _, index, scores, dropped = check(engine, ref, (n, cap))
    assert dropped == n - cap and len(index) == cap
    best = int(np.argmax([_score()(r) for r in m]))
    assert best in index.tolist()      # (s_0)
    if cap == 1:
        assert index.tolist() == [best]


# ---------------------------------------------------------------- 2: a surface, three uneven batches
def _surface(n, seed):
    """Points whose oriented coordinates are an affine image of v with v >= 0 and sum(v) = 1: none dominates another."""
    w = np.random.default_rng(seed).random((n, 4)) + 0.05
    v = w / w.sum(1, keepdims=True)
    return np.stack([1000.0 + 5000.0 * v[:, 0], 0.9 - 0.8 * v[:, 1], 1e9 + 4e9 * v[:, 2], 1.0 - 0.5 * v[:, 3]], axis=1)


def test_a_surface_in_three_batches(engine):
    """The second and third folds select among held u new; held entries that survive keep their record slots (the tags show)."""
    m, cap = _surface(2000, 21), 32
    engine.track_pareto(cap, ALL, keep="spread")
    ref = SpreadFront(cap, 15, _score())
    before, stayed, entered = None, 0, 0
    for a, b in ((0, 700), (700, 1800), (1800, 2000)):
        engine._debug_pareto_fold(m[a:b], _ok(b - a), a)
        _, index, _, dropped = check(engine, ref.fold(m[a:b], _ok(b - a), a), (a, b))
        assert len(index) == cap and dropped > 0
        if before is not None:
            stayed += len(set(before) & set(index.tolist()))
            entered += len(set(index.tolist()) - set(before))
        before = index.tolist()
    assert ref.n_dropped > 1900 and stayed > 0 and entered > 0, (ref.n_dropped, stayed, entered)


# ---------------------------------------------------------------- 3: ties
@pytest.mark.parametrize("cost_only", [False, True])
def test_a_lattice_full_of_ties(engine, cost_only):
    """Small integers: many equal distances.  Under the cost-only score every point of this lattice scores 2.0, so the global index
    decides s_0 and every tie after it."""
    m = _lattice()
    score = _score(cost_only)
    if cost_only:
        assert len({score(r) for r in m[:50]}) == 1
    engine.track_pareto(16, ALL, cost_only=cost_only, keep="spread")
    ref = SpreadFront(16, 15, score)
    for a, b in split7(len(m)):
        engine._debug_pareto_fold(m[a:b], _ok(b - a), a)
        check(engine, ref.fold(m[a:b], _ok(b - a), a), (cost_only, a, b))
    assert ref.n_dropped > 0 and len(ref.index) == 16


# ---------------------------------------------------------------- 4: degenerate coordinates
def test_degenerate_coordinates(engine):
    n, cap = 300, 16
    line = _antichain(n, 5)
    # an active metric that is constant over the front: its range is 0, the coordinate is ignored
    engine.track_pareto(cap, ("emissions", "opinion", "cost"), keep="spread")
    ref = SpreadFront(cap, 7, _score()).fold(line, _ok(n), 0)
    engine._debug_pareto_fold(line, _ok(n), 0)
    check(engine, ref, "constant opinion")
    assert ref.n_dropped == n - cap
    # a valid point of +inf cost, non-dominated through its emissions: the cost range is not finite, emissions alone spread the front
    m = np.concatenate([line, [[900.0, 0.5, np.inf, 1.0]]])
    engine.track_pareto(cap, ("emissions", "cost"), keep="spread")
    ref = SpreadFront(cap, 5, _score()).fold(m, _ok(n + 1), 0)
    engine._debug_pareto_fold(m, _ok(n + 1), 0)
    check(engine, ref, "+inf cost")
    assert ref.n_dropped == n + 1 - cap
    by_emissions = spread_select(np.stack([m[:, 0], np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)], axis=1), [_score()(r) for r in m], np.arange(n + 1), cap)
    assert sorted(by_emissions.tolist()) == ref.index.tolist()
    # the key of a NaN score is -inf.  No valid metrics give a NaN rank score, so the entry that stands last here scores -inf itself (an
    # inactive opinion of -inf): it is the one point that is never s_0, whatever its index
    assert preference(np.array([np.nan, 1.0, -np.inf]), np.arange(3)).tolist() == [1, 0, 2]
    m = line.copy()
    m[:, 0] -= 100000.0      # (net-negative emissions: the score is the cost's and the opinion's)
    first = int(SpreadFront(1, 5, _score()).fold(m, _ok(n), 0).index[0])
    m[first, 1] = -np.inf
    assert _score()(m[first]) == -np.inf
    engine.track_pareto(1, ("emissions", "cost"), keep="spread")
    ref = SpreadFront(1, 5, _score()).fold(m, _ok(n), 0)
    engine._debug_pareto_fold(m, _ok(n), 0)
    _, index, _, _ = check(engine, ref, "-inf score")
    assert index.tolist() != [first] and len(index) == 1


# ---------------------------------------------------------------- 5: one whole batch
def test_antichain_of_a_whole_batch(engine):
    """16 384 mutually non-dominated points into an empty archive, cap 256: the expected rows from the selection itself (256 rounds over
    16 384 rows), not from the O(n^2) front — an antichain by construction."""
    n, cap = 16384, 256
    m = _antichain(n, 3)
    score = _score()
    s = np.array([score(r) for r in m])
    keep = np.sort(spread_select(oriented(m, 5), s, np.arange(n), cap))
    assert len(set(keep.tolist())) == cap
    engine.track_pareto(cap, ("emissions", "cost"), keep="spread")
    engine._debug_pareto_fold(m, _ok(n), 0)
    rows, index, scores, dropped = engine.fetch_pareto()
    assert index.tolist() == keep.tolist() and dropped == n - cap
    assert scores.tobytes() == s[keep].tobytes() and rows.metrics.tobytes() == m[keep].tobytes()
    assert rows.n_draws.tolist() == keep.tolist()


# ---------------------------------------------------------------- 6: within the capacity the rules agree
def test_within_the_capacity_the_archive_is_the_score_rule_s(engine):
    m = _lattice()
    line = _antichain(256, 8)
    got = {}
    for keep in ("score", "spread"):
        engine.track_pareto(256, ALL, keep=keep)
        for a, b in split7(len(m)):
            engine._debug_pareto_fold(m[a:b], _ok(b - a), a)
        got[keep] = engine.fetch_pareto()
        engine.track_pareto(256, ("emissions", "cost"), keep=keep)      # a front of exactly cap points
        engine._debug_pareto_fold(line, _ok(256), 0)
        got[keep + " line"] = engine.fetch_pareto()
    assert 100 < len(got["score"][1]) < 256 and got["score"][3] == 0
    same(got["spread"], got["score"], "lattice")
    assert len(got["score line"][1]) == 256 and got["score line"][3] == 0
    same(got["spread line"], got["score line"], "line of 256")


# ---------------------------------------------------------------- 7: real episodes
@pytest.mark.parametrize("mask", [15, 5])
def test_real_episodes(mask):
    """Three training batches of 4 096 on the golden world, cap 8: after each the archive is SpreadFront over the fetched metrics, and
    every archived record is byte for byte what eg_fetch_record returned when its episode ran."""
    from eirgrid_amd.engine import ActionWeights, Engine
    from eirgrid_amd.world import World
    eng = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    try:
        eng.push(ActionWeights())
        eng.track_pareto(8, _names(mask), keep="spread")
        ref, records = SpreadFront(8, mask, _score()), {}

        def on_batch(b, first):
            res = eng.fetch(4096)
            ref.fold(res.metrics, res.status, first)
            for i in ref.index:
                if first <= i < first + 4096 and int(i) not in records:
                    records[int(i)] = eng.fetch_record(int(i) - first)
            rows, index, _, _ = check(eng, ref, (mask, b), tags=False)
            for r, i in enumerate(index):
                for f in RECORD_FIELDS:
                    assert getattr(rows, f)[r].tobytes() == getattr(records[int(i)], f)[0].tobytes(), (mask, b, int(i), f)
        _train(eng, 3, on_batch=on_batch)
        print(f"mask {mask}: held {len(ref.index)}, dropped {ref.n_dropped}")
        assert ref.n_dropped > 0 and len(ref.index) == 8      # (the restatement alone: the front outgrew the cap)
    finally:
        eng.close()


# ---------------------------------------------------------------- 8: breed and explore
def test_breed_front_is_the_host_loop(eng, sampled, monkeypatch):
    from tests import test_gpu_breed as B
    monkeypatch.setattr(B, "Front", SpreadFront)      # the host loop of tests/test_gpu_breed.py, folding with the spread rule
    pol, parents = sampled
    ref = B.breed_restated(eng, pol, parents, SEED, INDEX, ALL, False, CUTS, 3, 4, 40)
    print("breed rows", ref["rows"], ref["stop"])
    assert any(r[6] > 0 for r in ref["rows"]), ref["rows"]      # (the reference alone: room ran out)
    front = eng.breed_front(pol, parents, SEED, INDEX, objectives=ALL, cuts=CUTS, generations=3, cap=4, max_variants=40, keep="spread")
    B._assert_is(front, ref, "breed, cap 4, spread")
    assert any(r.n_dropped > 0 for r in front.generations)
    assert front.plans == front.lineage(parents)[-1] == ref["pops"][-1]


def test_explore_front_is_the_host_loop(eng, sampled, monkeypatch):
    from tests import test_gpu_explore as X
    monkeypatch.setattr(X, "Front", SpreadFront)
    pol, starts = sampled
    ref = X.explore_restated(eng, pol, starts, SEED, INDEX, ALL, False, 3, 4, 37, X.DELETES)
    assert ref["rows"][-1][5] > 0, ref["rows"]      # (the reference alone: room ran out)
    front = eng.explore_front(pol, starts, SEED, INDEX, objectives=ALL, generations=3, cap=4, launch=37, keep="spread", **X.DELETES)
    X._assert_is(front, ref, "explore, cap 4, spread")
    assert front.generations[-1].n_dropped > 0


# ---------------------------------------------------------------- 9: refusals
def test_refusals(world, sampled):
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import ActionWeights, Engine, Group
    L = N.lib()
    e = Engine(world, device=0)
    g = Group(world, devices=(0, 0))
    try:
        for mode in (0, 3, KEEP_SPREAD, KEEP_SPREAD | 3, 0x201, 0x1101, -1):
            assert L.eg_pareto_track(e.h, 8, 15, mode) == N.EG_ERR_BAD_ARG, mode
            assert "eg_pareto_track: mode " + str(mode) in L.eg_last_error().decode(), (mode, L.eg_last_error())
            assert L.eg_debug_breed_begin(e.h, 8, 15, mode) == N.EG_ERR_BAD_ARG, mode
            assert "eg_debug_breed_begin: mode " + str(mode) in L.eg_last_error().decode(), (mode, L.eg_last_error())
        for mode in (KEEP_SPREAD | 1, KEEP_SPREAD | 2):
            assert L.eg_pareto_track(e.h, 8, 15, mode) == N.EG_OK, (mode, L.eg_last_error())
            assert L.eg_debug_breed_begin(e.h, 8, 15, mode) == N.EG_OK, (mode, L.eg_last_error())
            state = e._debug_breed_fetch()["state"].view(np.int32)      # cap, n_held, objectives, mode | i64 n_dropped, the rule
            assert state[:4].tolist() == [8, 0, 15, mode & 3] and state[4:8].view(np.int64).tolist() == [0, 1]
        assert L.eg_pareto_track(g.ranks[0].h, 8, 15, KEEP_SPREAD | 1) == N.EG_ERR_BAD_ARG and "eg_group" in L.eg_last_error().decode()
        pol, plans = sampled
        with pytest.raises(N.EirgridError, match="eg_breed_plans: the context is a rank of an eg_group"):
            g.ranks[0].breed_front(pol, plans[:2], 1, keep="spread")
        with pytest.raises(ValueError, match="keep = 'nonsense'"):
            e.track_pareto(8, keep="nonsense")
        with pytest.raises(ValueError, match="keep = 'nonsense'"):
            e.breed_front(ActionWeights(), plans, 1, keep="nonsense")
        with pytest.raises(ValueError, match="keep = 'nonsense'"):
            e.explore_front(ActionWeights(), plans, 1, keep="nonsense")
    finally:
        g.close(); e.close()


# ---------------------------------------------------------------- 10: the script
def test_the_breed_script_keeps_spread(eng, sampled, tmp_path):
    from eirgrid_amd.engine import ActionWeights, Plan
    pol, parents = sampled
    ckpt, plan_file, out_dir = str(tmp_path / "policy.json"), str(tmp_path / "parents.jsonl"), str(tmp_path / "run")
    pol.save_to_file(ckpt)
    Plan.save(plan_file, parents)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "breed_front.py"), "--world", WORLD, "--plans", plan_file, "--policy", ckpt, "--seed", str(SEED),
                          "--generations", "2", "--cap", "4", "--cuts", "2030,2038,2045", "--keep", "spread", "--out", out_dir], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    kw = dict(cuts=CUTS, generations=2, cap=4)
    want = eng.breed_front(ActionWeights.load_from_file(ckpt), Plan.load(plan_file), SEED, 0, keep="spread", **kw)
    assert any(g.n_dropped > 0 for g in want.generations)
    back = Plan.load(os.path.join(out_dir, "breed", "plans.jsonl"))
    assert back == want.plans and [p.name for p in back] == [p.name for p in want.plans]
    other = eng.breed_front(ActionWeights.load_from_file(ckpt), Plan.load(plan_file), SEED, 0, **kw)
    print("spread", [p.name for p in want.plans], "score", [p.name for p in other.plans])
