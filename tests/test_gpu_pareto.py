"""GPU: the Pareto archive (include/eirgrid_hip.h eg_pareto_track; csrc/eg_pareto.h) against the restatement of its definition in
tests/test_pareto.py — crafted metric sets through eg_debug_pareto_fold (ties, chains, antichains beyond the capacity, equal points,
infinities and NaN, evictions, split invariance, the streaming truncation), then real episodes, the replay hoist, the three folds side
by side, plan batches, the refusals and the user script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_pareto import SCRIPT, Front, front, split7, valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
RECORD_FIELDS = ("metrics", "yearly", "status", "n_run", "n_def", "n_act", "run_log", "def_log", "act_log", "n_gens", "gen_cell",
                 "gen_pack", "n_offsets", "off_pack", "n_draws", "bytes_moved", "n_chunks")
CHUNK = 256      # csrc/eg_pareto.h: episodes per workgroup of the filter = entries per tile of the pairwise kernels
pytestmark = pytest.mark.gpu


@pytest.fixture
def engine(engine):
    """The session's engine, with tracking off again for whoever uses it next."""
    yield engine
    engine.track_pareto(0)


def _score(cost_only=False):
    from eirgrid_amd.engine import rank_score
    return lambda row: rank_score(np.ascontiguousarray(row), cost_only)


def _ok(n):
    return np.zeros(n, np.int32)


def check(eng, ref, what, tags=True):
    """n_held, indices, score bits, n_dropped and every row's metrics equal the restatement's; with `tags` (synthetic records) n_draws of
    every row is its global index: a record in the wrong slot shows."""
    rows, index, scores, dropped = eng.fetch_pareto()
    assert index.tolist() == ref.index.tolist(), (what, index.tolist(), ref.index.tolist())
    assert dropped == ref.n_dropped, (what, dropped, ref.n_dropped)
    assert scores.tobytes() == ref.scores().tobytes(), what
    assert rows.metrics.tobytes() == ref.m.tobytes(), what
    assert (rows.status == 0).all(), what
    if tags:
        assert rows.n_draws.tolist() == index.tolist(), (what, rows.n_draws.tolist())
    return rows, index, scores, dropped


def same(a, b, what, fields=RECORD_FIELDS):
    assert a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3], (what, a[1], b[1])
    for f in fields:
        assert getattr(a[0], f).tobytes() == getattr(b[0], f).tobytes(), (what, f)


SIZES = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1)


@pytest.mark.parametrize("mask", [15, 5, 1, 8, 10])
def test_small_integer_points_at_every_size(engine, mask):
    """Random points of [0, 6]^4 — ties and equal points everywhere — one below, at and one above the wave and the chunk / tile size,
    three chunks plus one; then a second batch of the same size on top of the held entries."""
    rng = np.random.default_rng(100 + mask)
    for n in SIZES:
        engine.track_pareto(256, _names(mask))
        ref = Front(256, mask, _score())
        first = 10
        for b in range(2):
            m = rng.integers(0, 7, (n, 4)).astype(np.float64)
            engine._debug_pareto_fold(m, _ok(n), first)
            if b == 0:      # the hook leaves a batch of n tagged records behind
                assert engine.fetch(n).n_draws.tolist() == list(range(first, first + n))
            check(engine, ref.fold(m, _ok(n), first), (mask, n, b))
            if mask in (1, 8):      # one objective: the optimum, at its lowest index
                assert len(ref.index) == 1
            first += n + 5


def _names(mask):
    from eirgrid_amd.engine import PARETO_OBJECTIVES
    return tuple(n for i, n in enumerate(PARETO_OBJECTIVES) if mask >> i & 1)


def test_a_chain_leaves_its_head(engine):
    n = 2000
    i = np.arange(n, dtype=np.float64)
    chain = np.stack([i, 5000.0 - i, 7.0 + i, 5000.0 - i], axis=1)      # every point dominates the next
    for name, m, head in (("forward", chain, 0), ("reversed", chain[::-1].copy(), n - 1)):
        engine.track_pareto(256)
        ref = Front(256, 15, _score()).fold(m, _ok(n), 0)
        engine._debug_pareto_fold(m, _ok(n), 0)
        rows, index, _, _ = check(engine, ref, name)
        assert index.tolist() == [head] and rows.metrics[0].tolist() == chain[0].tolist()


def _antichain(n, seed):
    """x ascending against y descending under mask 5, in shuffled index order; emissions above net zero, so the rank score falls with x."""
    r = np.random.default_rng(seed).permutation(n).astype(np.float64)
    return np.stack([1000.0 + 50.0 * r, np.full(n, 0.5), 1e9 * (n - r), np.ones(n)], axis=1)


@pytest.mark.parametrize("n,cap", [(300, 256), (3000, 256), (3000, 8)])
def test_antichain_beyond_the_capacity(engine, n, cap):
    m = _antichain(n, n + cap)
    engine.track_pareto(cap, ("emissions", "cost"))
    ref = Front(cap, 5, _score()).fold(m, _ok(n), 0)
    engine._debug_pareto_fold(m, _ok(n), 0)
    _, index, _, dropped = check(engine, ref, (n, cap))
    assert dropped == n - cap and len(index) == cap
    if (n, cap) == (300, 256):
        assert dropped == 44


def test_antichain_of_a_whole_batch(engine):
    """16 384 mutually non-dominated points into an empty archive: every one survives the filter and the pairwise pass, and the one
    truncation keeps the 256 of the largest rank score.  (Expected without the O(n^2) restatement: an antichain by construction.)"""
    n, cap = 16384, 256
    m = _antichain(n, 3)
    assert len(np.unique(m[:, 0])) == n and (np.diff(m[np.argsort(m[:, 0]), 2]) < 0).all()
    score = _score()
    s = np.array([score(r) for r in m])
    keep = np.array(sorted(sorted(range(n), key=lambda e: (-s[e], e))[:cap]))
    engine.track_pareto(cap, ("emissions", "cost"))
    engine._debug_pareto_fold(m, _ok(n), 0)
    rows, index, scores, dropped = engine.fetch_pareto()
    assert index.tolist() == keep.tolist() and dropped == n - cap
    assert scores.tobytes() == s[keep].tobytes() and rows.metrics.tobytes() == m[keep].tobytes()
    assert rows.n_draws.tolist() == keep.tolist()


def test_equal_points_are_held_once_at_the_lowest_index(engine):
    rng = np.random.default_rng(9)
    n = 3 * CHUNK
    m = np.repeat(_antichain(n // 4, 4), 4, axis=0)      # 192 antichain points at every fourth index, each followed by three it dominates
    level = np.tile(np.arange(4.0), n // 4)
    m[:, 0] += level; m[:, 2] += 1e3 * level
    m[200] = m[4]; m[2 * CHUNK + 8] = m[CHUNK + 4]      # equal points inside one chunk, and in two chunks
    m[CHUNK + 100, [1, 3]] = [0.1, 0.2]; m[CHUNK + 100, [0, 2]] = m[40, [0, 2]]      # equal but for the inactive metrics
    engine.track_pareto(256, ("emissions", "cost"))
    ref = Front(256, 5, _score())
    engine._debug_pareto_fold(m, _ok(n), 5000)
    _, index, _, _ = check(engine, ref.fold(m, _ok(n), 5000), "one batch")
    assert not {5200, 5000 + 2 * CHUNK + 8, 5000 + CHUNK + 100} & set(index.tolist()) and {5004, 5000 + CHUNK + 4, 5040} <= set(index.tolist())
    before = engine.fetch_pareto()
    engine._debug_pareto_fold(m, _ok(n), 5000)      # the same batch again: the held entries stay
    same(engine.fetch_pareto(), before, "folded twice")
    check(engine, ref.fold(m, _ok(n), 5000), "folded twice")
    held = ref.index.copy()
    pick = rng.choice(len(held), 40, replace=False)      # equal points at lower indices arrive later: representative and record move
    late = ref.m[pick]
    engine._debug_pareto_fold(late, _ok(40), 100)
    rows, index, _, _ = check(engine, ref.fold(late, _ok(40), 100), "lower index later")
    assert set(range(100, 140)) <= set(index.tolist()) and len(index) == len(held)


def test_zeros_infinities_nan_and_failed_episodes(engine):
    inf, nan = np.inf, np.nan
    m = np.array([[+0.0, 0.5, 3e9, 1.0],      # 0
                  [-0.0, 0.5, 3e9, 1.0],      # 1: -0.0 == +0.0, the same point as 0
                  [5.0, 0.5, inf, 1.0],       # 2: +inf cost, dominated
                  [-inf, 0.1, 9e9, 0.2],      # 3: -inf emissions, on the front
                  [nan, 0.9, 1.0, 1.0],       # 4: NaN in an active metric
                  [-5.0, nan, 1.0, 1.0],      # 5: NaN in an inactive metric (mask 5): skipped as well
                  [-9.0, 0.9, 1.0, 1.0],      # 6: would dominate everything, but failed
                  [7.0, 0.5, 2e9, 1.0],       # 7
                  [-0.0, 0.5, 2e9, 1.0]])     # 8: dominates 0 and 1
    st = np.array([0, 0, 0, 0, 0, 0, -2, 0, 0], np.int32)
    for mask in (5, 15, 1):
        engine.track_pareto(256, _names(mask))
        ref = Front(256, mask, _score()).fold(m, st, 0)
        engine._debug_pareto_fold(m, st, 0)
        rows, index, _, _ = check(engine, ref, mask)
        assert not {4, 5, 6} & set(index.tolist()) and 3 in index.tolist()
    engine.track_pareto(256, ("emissions", "cost"))
    engine._debug_pareto_fold(m[:2][::-1].copy(), _ok(2), 0)      # -0.0 first: the entry keeps the lower index's bits
    rows, index, _, _ = engine.fetch_pareto()
    assert index.tolist() == [0] and np.signbit(rows.metrics[0, 0])


def test_eviction_frees_slots_for_the_same_fold(engine):
    """cap 32.  Batch 1: an antichain of 20.  Batch 2: three points that dominate all of them.  Batch 3: 29 more beside those three —
    32 entries in 32 slots only if the 20 evicted slots came back."""
    def anti(k, x0, y0):
        i = np.arange(k, dtype=np.float64)
        return np.stack([x0 + i, np.full(k, 0.5), y0 - i, np.ones(k)], axis=1)
    engine.track_pareto(32, ("emissions", "cost"))
    ref = Front(32, 5, _score())
    for b, (m, first) in enumerate(((anti(20, 100.0, 1e6), 0), (anti(3, 50.0, 900.0), 100), (anti(29, 10.0, 2000.0), 200))):
        engine._debug_pareto_fold(m, _ok(len(m)), first)
        _, index, _, dropped = check(engine, ref.fold(m, _ok(len(m)), first), b)
        assert len(index) == (20, 3, 32)[b] and dropped == 0


def _lattice(n=5000, hi=8, t=10):
    """Points of [0, hi]^4 away from the ideal corner (oriented coordinate sum >= t): a front of 162 points among 3 341 distinct ones."""
    u = np.random.default_rng(77).integers(0, hi + 1, (6 * n, 4))
    u = u[u.sum(1) >= t][:n].astype(np.float64)
    u[:, 1] = hi - u[:, 1]; u[:, 3] = hi - u[:, 3]
    assert len(u) == n
    return u


@pytest.fixture(scope="module")
def lattice():
    m = _lattice()
    m.setflags(write=False)
    return m, Front(256, 15, _score()).fold(m, _ok(len(m)), 0)


def test_split_invariance_while_nothing_is_dropped(engine, lattice):
    m, ref = lattice
    assert 100 < len(ref.index) < 256 and ref.n_dropped == 0
    parts = split7(len(m))
    got = []
    for name, order in (("one batch", [(0, len(m))]), ("seven batches", parts), ("seven batches, reversed", parts[::-1])):
        engine.track_pareto(256)
        for a, b in order:
            engine._debug_pareto_fold(m[a:b], _ok(b - a), a)
        check(engine, ref, name)
        got.append(engine.fetch_pareto())
    same(got[0], got[1], "one batch / seven"); same(got[0], got[2], "one batch / seven reversed")


def test_truncation_is_the_streaming_rule(engine, lattice):
    m, _ = lattice
    engine.track_pareto(16)
    ref = Front(16, 15, _score())
    for a, b in split7(len(m)):
        engine._debug_pareto_fold(m[a:b], _ok(b - a), a)
        check(engine, ref.fold(m[a:b], _ok(b - a), a), (a, b))
    assert ref.n_dropped > 0 and len(ref.index) == 16


def _train(eng, batches, n=4096, seed=9001, on_batch=None):
    first = 0
    for b in range(batches):
        eng.device_step(seed, first, n, 10, seed + first)
        if on_batch:
            on_batch(b, first)
        first += n


@pytest.mark.parametrize("mask", [15, 5])
def test_real_episodes(world, mask):
    """Three batches of 4 096 through device_step, every 10th a replay: after each the archive is the restatement over the fetched
    metrics, and every archived record is byte for byte what eg_fetch_record returned when its episode ran."""
    from eirgrid_amd.engine import ActionWeights, Engine
    eng = Engine(world, device=0)
    try:
        eng.push(ActionWeights())
        eng.track_pareto(256, _names(mask))
        ref, records = Front(256, mask, _score()), {}

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
        assert len(ref.index) > 1 and ref.n_dropped == 0
    finally:
        eng.close()


def test_replay_hoist_gives_the_same_archive(world):
    from eirgrid_amd.engine import ActionWeights, Engine
    a, b = Engine(world, device=0), Engine(world, device=0)
    try:
        b.replay_hoist(True)
        for e in (a, b):
            e.push(ActionWeights())
            e.track_pareto(256)
        first = 0
        for n, period in ((4096, 0), (4096, 10), (4096, 3), (2048, 1)):
            for e in (a, b):
                e.device_step(31, first, n, period, 31 + first)
            first += n
            same(a.fetch_pareto(), b.fetch_pareto(), (n, period), RECORD_FIELDS[:-1])      # (n_chunks counts the search that really ran)
        armed, _ = b.replay_hoist_stats()
        assert armed >= 3, armed
    finally:
        a.close(); b.close()


def _policy_bytes(eng):
    from eirgrid_amd.engine import ActionWeights
    pol = ActionWeights()
    eng.pull(pol)
    return b"".join(np.ascontiguousarray(t).tobytes() for t in pol.tables()) + repr((pol.lists(0), pol.lists(1), pol.get("best_cost"))).encode()


def test_the_three_folds_side_by_side(world):
    """Pareto, top-K (k = 10) and best_result on in one run, each alone in runs of their own, and a run with none: every archive and the
    pulled policy are identical."""
    from eirgrid_amd.engine import ActionWeights, Engine
    got = {}
    for name in ("all", "pareto", "topk", "best", "none"):
        eng = Engine(world, device=0)
        try:
            eng.push(ActionWeights())
            if name in ("all", "pareto"):
                eng.track_pareto(256)
            if name in ("all", "topk"):
                eng.track_top_k(10)
            if name in ("all", "best"):
                eng.track_best_result()
            _train(eng, 2)
            got[name] = {"policy": _policy_bytes(eng),
                         "pareto": eng.fetch_pareto() if name in ("all", "pareto") else None,
                         "topk": eng.fetch_top_k() if name in ("all", "topk") else None,
                         "best": eng.fetch_best_result() if name in ("all", "best") else None}
        finally:
            eng.close()
    same(got["all"]["pareto"], got["pareto"]["pareto"], "pareto")
    assert len(got["all"]["pareto"][1]) > 1
    (ra, sa, ia), (rb, sb, ib) = got["all"]["topk"], got["topk"]["topk"]
    assert ia.tolist() == ib.tolist() and sa.tobytes() == sb.tobytes() and len(ia) == 10
    assert got["all"]["best"][0] == got["best"]["best"][0] is not None
    for f in RECORD_FIELDS:
        assert getattr(ra, f).tobytes() == getattr(rb, f).tobytes(), f
        assert getattr(got["all"]["best"][1], f).tobytes() == getattr(got["best"]["best"][1], f).tobytes(), f
    for name in ("pareto", "topk", "best", "none"):
        assert got[name]["policy"] == got["all"]["policy"], name


def test_plan_batches_are_folded_on_request_only(world):
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    eng = Engine(world, device=0)
    try:
        w = ActionWeights()
        res = eng.rollout_batch(w, 4711, 40)
        plans = [Plan.from_result(res, e, f"p{e}") for e in range(40)]
        eng.track_pareto(256)
        out = eng.evaluate_plans(w, plans, 99, 7000)
        assert eng.fetch_pareto()[1].tolist() == []      # an evaluation is not training
        ref = Front(256, 15, _score()).fold(out.metrics, out.status, 7000)
        eng.fold_pareto_last_batch()
        rows, index, _, _ = check(eng, ref, "plans", tags=False)
        assert len(index) >= 1 and all(7000 <= i < 7040 for i in index)
        for r, i in enumerate(index):
            for f in RECORD_FIELDS:
                assert getattr(rows, f)[r].tobytes() == getattr(eng.fetch_record(int(i) - 7000), f)[0].tobytes(), (int(i), f)
        before = eng.fetch_pareto()
        eng.fold_pareto_last_batch()
        same(eng.fetch_pareto(), before, "folded twice")
    finally:
        eng.close()


def test_refusals_name_the_field(world):
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import ActionWeights, Engine, Group
    L = N.lib()
    eng = Engine(world, device=0)
    g = Group(world, devices=(0, 0))
    try:
        for args, word in (((-1, 15, 1), "cap"), ((257, 15, 1), "cap"), ((8, 0, 1), "objectives"), ((8, 16, 1), "objectives"),
                           ((8, 15, 0), "mode"), ((8, 15, 3), "mode")):
            assert L.eg_pareto_track(eng.h, *args) == N.EG_ERR_BAD_ARG, args
            assert word in L.eg_last_error().decode(), (args, L.eg_last_error())
        assert L.eg_pareto_track(g.ranks[0].h, 8, 15, 1) == N.EG_ERR_BAD_ARG and "eg_group" in L.eg_last_error().decode()
        assert L.eg_pareto_fold_last_batch(eng.h) == N.EG_ERR_BAD_ARG and "tracking" in L.eg_last_error().decode()
        held = N.C.c_int32(0)
        assert L.eg_fetch_pareto(eng.h, None, N.C.byref(held), None, None, None) == N.EG_ERR_BAD_ARG      # never tracked
        eng.track_pareto(8)
        assert L.eg_pareto_fold_last_batch(eng.h) == N.EG_ERR_BAD_ARG and "batch" in L.eg_last_error().decode()
        eng.push(ActionWeights())
        eng.device_step(3, 0, 512, 10, 3)
        before = eng.fetch_pareto()
        assert len(before[1]) >= 1
        eng.track_pareto(0)      # stops the folding, the archive stays fetchable
        eng.device_step(3, 512, 512, 10, 4)
        same(eng.fetch_pareto(), before, "cap 0")
        assert L.eg_pareto_fold_last_batch(eng.h) == N.EG_ERR_BAD_ARG
    finally:
        g.close(); eng.close()


def test_pareto_front_script(tmp_path):
    """The user script in a fresh child process: index.csv is Engine.fetch_pareto() of the same run made here, and eg_plans_load reads
    plans.jsonl back with as many plans."""
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    out = subprocess.run([sys.executable, SCRIPT, "--world", WORLD, "-n", "8192", "--batch", "4096", "--seed", "9001", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    eng = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    try:
        eng.push(ActionWeights())
        eng.track_pareto(256)
        _train(eng, 2)
        rows, index, scores, dropped = eng.fetch_pareto()
    finally:
        eng.close()
    lines = open(tmp_path / "pareto" / "index.csv").read().strip().split("\n")
    assert lines[0] == "global_index,final_net_emissions,average_public_opinion,total_cost,power_reliability,rank_score"
    want = [",".join([str(int(index[r]))] + ["%.17g" % x for x in rows.metrics[r]] + ["%.17g" % scores[r]]) for r in range(len(index))]
    assert lines[1:] == want and len(want) > 1
    plans = Plan.load(tmp_path / "pareto" / "plans.jsonl")
    assert len(plans) == len(index)
    assert plans[0] == Plan.from_result(rows, 0)
