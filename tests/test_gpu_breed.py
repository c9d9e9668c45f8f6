"""GPU: generations of plan crosses with Pareto selection on the device (include/eirgrid_hip.h eg_breed_plans; csrc/eg_breed.h
k_breed_gather, k_breed_turnover; csrc/eg_breed.cpp) against a restatement written out here: a Python generation loop that enumerates
the variants as the header does, evaluates each chunk with the existing Engine.evaluate_plan_crosses(..., same_index=True) over the
host-built population, and folds chunk by chunk with the O(n^2) restatement of the archive's streaming rule (tests/test_pareto.py Front,
capacity included).  Everything runs on tests/golden/world_v1.json."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanCross, cross_pairs, rank_score
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plan_crosses import SHORT_MAX, _full_plan, _record_parents
from tests.test_gpu_plans import _same_records
from tests.test_pareto import Front, valid
from tests.test_plan_crosses import apply_cross

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
CUTS = (5, 13, 20)
ALL = ("emissions", "opinion", "cost", "reliability")
SEED, INDEX = 91, 7
# test 3 (cap 6, chunks of 40): the plans of this file replay to the end without a fallback draw, so the evaluation seed does not move
# them; what a seed moves is which four episodes are sampled as parents.  SAMPLE_CAP is the sampling seed at which the RESTATEMENT alone
# drops for want of room in some generation and, in some generation, keeps a child while a parent leaves — looked for with the
# restatement only (sampling seeds 1, 2, 3, ... in order; the first that does both)
SAMPLE_CAP = 1


def _mask(objectives):
    return sum(1 << ALL.index(o) for o in objectives)


def _len(plan, which):
    return sum(len(l) for l in (plan.best_actions, plan.best_deficit_actions)[which])


def _fits(pop, x):
    child = apply_cross(pop, x)
    return _len(child, 0) <= 4096 and _len(child, 1) <= 4096


def breed_restated(eng, pol, parents, seed, index, objectives, cost_only, cuts, generations, cap, launch):
    """The header's generation loop, on the host: {rows: a tuple per generation in eg_breed_generation's field order, members: per
    generation [(PlanCross, variant, score bytes, metrics bytes)], stop, pops: every population from P_0 on}."""
    mask = _mask(objectives)
    pops, rows, members, stop = [list(parents)], [], [], "max_generations"
    for g in range(generations):
        pop = pops[-1]
        n = len(pop)
        every = cross_pairs(n, cuts)
        crosses = [x for x in every if x.a == x.b or _fits(pop, x)]
        arch = Front(cap, mask, lambda m: rank_score(m, cost_only))
        n_valid = 0
        for first in range(0, len(crosses), launch):
            chunk = crosses[first:first + launch]
            res = eng.evaluate_plan_crosses(pol, pop, chunk, seed, index, same_index=True)
            n_valid += int(valid(res.metrics[:len(chunk)], res.status[:len(chunk)]).sum())
            arch.fold(res.metrics[:len(chunk)], res.status[:len(chunk)], first)
        kept = [int(k) for k in arch.index]
        rows.append((n, len(every) - len(crosses), len(kept), sum(k >= n for k in kept), len(crosses), n_valid, arch.n_dropped))
        members.append([(crosses[k], k, np.float64(rank_score(m, cost_only)).tobytes(), np.ascontiguousarray(m).tobytes()) for k, m in zip(kept, arch.m)])
        if not kept:
            stop = "empty"
            break
        pops.append([apply_cross(pop, crosses[k]) for k in kept])
        if len(kept) == n and all(k < n for k in kept):
            stop = "converged"
            break
    return {"rows": rows, "members": members, "stop": stop, "pops": pops}


def _rows(front):
    return [(r.n_parents, r.n_skipped, r.n_kept, r.n_children_kept, r.n_variants, r.n_valid, r.n_dropped) for r in front.generations]


def _members(front):
    return [[(m.cross, m.variant, np.float64(m.score).tobytes(), np.array(m.metrics, np.float64).tobytes()) for m in kept] for kept in front.members]


def _assert_is(front, ref, what):
    assert front.stop_reason == ref["stop"], (what, front.stop_reason, ref["stop"])
    assert _rows(front) == ref["rows"], (what, _rows(front), ref["rows"])
    got = _members(front)
    assert len(got) == len(ref["members"]), what
    for g, (a, b) in enumerate(zip(got, ref["members"])):
        assert a == b, (what, "generation", g, [m[:2] for m in a], [m[:2] for m in b])


@pytest.fixture(scope="module")
def eng(built):
    from eirgrid_amd.world import World
    e = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sets(eng):
    """{name: (policy, parents, objectives, cost_only)} — four sampled episodes under all four objectives; a short, a long and four
    crafted plans whose children cross kShortReplayMax both ways, under emissions and cost"""
    pol = ActionWeights()
    res = eng.rollout_batch(pol, 4711, 4)
    sampled = [Plan.from_result(res, e, f"sampled {e}") for e in range(4)]
    cpol, crafted, _ = _record_parents(eng, np.random.default_rng(17))
    lens = [len(p) for p in crafted]
    assert min(lens) <= SHORT_MAX < max(lens)
    res = eng.rollout_batch(pol, SAMPLE_CAP, 4)
    sampled6 = [Plan.from_result(res, e, f"sampled {e}") for e in range(4)]
    return {"sampled": (pol, sampled, ALL, False), "crafted": (cpol, crafted, ("emissions", "cost"), True), "sampled6": (pol, sampled6, ALL, False)}


_CACHE = {}


def _ref(eng, sets, name, cap, launch, seed=SEED, generations=3):
    key = ("ref", name, cap, launch, seed, generations)
    if key not in _CACHE:
        pol, parents, objectives, cost_only = sets[name]
        _CACHE[key] = breed_restated(eng, pol, parents, seed, INDEX, objectives, cost_only, CUTS, generations, cap, launch)
    return _CACHE[key]


def _front(eng, sets, name, cap, launch, seed=SEED, generations=3):
    key = ("front", name, cap, launch, seed, generations)
    if key not in _CACHE:
        pol, parents, objectives, cost_only = sets[name]
        _CACHE[key] = eng.breed_front(pol, parents, seed, INDEX, objectives=objectives, cost_only=cost_only, cuts=CUTS, generations=generations, cap=cap,
                                      max_variants=launch)
    return _CACHE[key]


# ---------------------------------------------------------------- 1: one generation is cross_front
def test_one_generation_is_cross_front(eng, sets):
    pol, parents, _, _ = sets["sampled"]
    for kw in ({}, {"objectives": ("emissions", "cost"), "cost_only": True}):
        want = eng.cross_front(pol, parents, SEED, INDEX, **kw)
        got = eng.breed_front(pol, parents, SEED, INDEX, generations=1, **kw)
        row, kept = got.generations[0], got.members[0]
        print("cross_front", kw, "kept", want.variant.tolist(), "of", want.n_variants, "valid", want.n_valid)
        assert len(got.generations) == 1 and len(got.members) == 1
        assert [m.variant for m in kept] == want.variant.tolist() and len(kept) >= 1
        assert [m.cross for m in kept] == want.crosses
        assert np.array([m.metrics for m in kept]).tobytes() == want.metrics.tobytes() == got.metrics.tobytes()
        assert np.array([m.score for m in kept]).tobytes() == want.score.tobytes() == got.score.tobytes()
        assert (row.n_parents, row.n_skipped, row.n_variants, row.n_valid, row.n_dropped) == (4, 0, want.n_variants, want.n_valid, 0)
        assert (row.n_kept, row.n_children_kept) == (len(want.variant), int((~want.is_parent).sum()))
        only_parents = len(want.variant) == 4 and bool(want.is_parent.all())
        assert got.stop_reason == ("converged" if only_parents else "max_generations")
        assert N.lib().eg_last_batch_size(eng.h) == want.n_variants      # (one chunk)


# ---------------------------------------------------------------- 2: three generations, one chunk and chunks of 40
@pytest.mark.parametrize("name", ["sampled", "crafted"])
def test_three_generations_are_the_restatement_whatever_the_chunks(eng, sets, name):
    ref = _ref(eng, sets, name, 256, 16384)
    print(name, "rows", ref["rows"], ref["stop"])
    whole, chunked = _front(eng, sets, name, 256, 16384), _front(eng, sets, name, 256, 40)
    _assert_is(whole, ref, (name, "one chunk"))
    _assert_is(chunked, ref, (name, "chunks of 40"))
    assert _rows(whole) == _rows(chunked) and _members(whole) == _members(chunked)
    assert all(r.n_dropped == 0 for r in whole.generations)
    assert sum(r.n_children_kept for r in whole.generations) > 0 and max(r.n_variants for r in whole.generations) > 40      # (children bred, several chunks)
    if name == "crafted":      # the population crosses kShortReplayMax both ways
        lens = [len(p) for pop in ref["pops"] for p in pop]
        assert min(lens) <= SHORT_MAX < max(lens)


# ---------------------------------------------------------------- 3: capacity
@pytest.mark.parametrize("name", ["sampled6", "crafted"])
def test_a_small_cap_drops_by_the_streaming_rule(eng, sets, name):
    ref = _ref(eng, sets, name, 6, 40)
    rows = ref["rows"]
    print(name, "rows", rows, ref["stop"])
    # (the reference alone:) room ran out, and a generation kept a child while a parent left
    assert any(r[6] > 0 for r in rows), rows
    assert any(r[3] > 0 and r[2] - r[3] < r[0] for r in rows), rows
    front = _front(eng, sets, name, 6, 40)
    _assert_is(front, ref, (name, "cap 6"))
    assert any(r.n_dropped > 0 for r in front.generations)
    assert any(r.n_children_kept > 0 and r.n_kept - r.n_children_kept < r.n_parents for r in front.generations)


# ---------------------------------------------------------------- 4: the blocks and the records
def _same_records_but_n_chunks(a, b, what, rows_a, rows_b):
    """tests/test_gpu_plans.py _same_records, n_chunks excepted (include/eirgrid_hip.h: it counts what the search that really ran requested,
    and a chunk of many variants runs another kernel than a plan alone)"""
    for name in _ALL_FIELDS:
        assert _used(a, name)[rows_a].tobytes() == _used(b, name)[rows_b].tobytes(), (what, name)


@pytest.mark.parametrize("name,cap,launch", [("sampled", 256, 40), ("crafted", 256, 16384), ("crafted", 6, 40)])
def test_the_population_is_the_lineage_and_its_records_are_the_plans(eng, sets, name, cap, launch, seed=SEED):
    pol, parents, _, _ = sets[name]
    front = _front(eng, sets, name, cap, launch)
    ref = _ref(eng, sets, name, cap, launch if cap == 6 else 16384)
    line = front.lineage(parents)
    assert len(line) == len(ref["pops"])
    for g, (a, b) in enumerate(zip(line, ref["pops"])):
        assert a == b, (name, "population", g)      # (PlanCross.apply against the tests' apply_cross)
    assert len(front.plans) == len(line[-1]) >= 1
    for r, (got, want) in enumerate(zip(front.plans, line[-1])):
        assert got.best_actions == want.best_actions and got.best_deficit_actions == want.best_deficit_actions, (name, "plan", r)
        assert got.name == want.name, (name, r, got.name, want.name)
    assert any(">" in p.name and "@20" in p.name for p in front.plans), [p.name for p in front.plans]      # (a child is named A>B@year)
    assert front.records is not None and len(front.records.status) == len(front.plans)
    for r, p in enumerate(front.plans):
        one = eng.evaluate_plans(pol, [p], seed, INDEX)
        _same_records_but_n_chunks(front.records, one, (name, "record", r), [r], [0])
        assert front.records.metrics[r].tobytes() == front.metrics[r].tobytes()


# ---------------------------------------------------------------- 5: edges
def test_edges(eng, sets):
    pol, parents, _, _ = sets["sampled"]
    # one parent converges in generation 0 with itself
    one = eng.breed_front(pol, parents[:1], SEED, INDEX, cuts=CUTS, generations=4)
    assert one.stop_reason == "converged" and _rows(one) == [(1, 0, 1, 0, 1, 1, 0)]
    assert one.members[0][0].cross == PlanCross(0, 0, 0, 0) and one.plans == parents[:1] and one.plans[0].name == parents[0].name
    # two identical parents keep one: every variant is the same plan, one point, held at the lowest number
    twin = Plan(parents[1].best_actions, parents[1].best_deficit_actions, "twin")
    two = eng.breed_front(pol, [parents[1], twin], SEED, INDEX, cuts=CUTS, generations=4)
    assert two.stop_reason == "converged" and _rows(two) == [(2, 0, 1, 0, 8, 8, 0), (1, 0, 1, 0, 1, 1, 0)]
    assert [m.variant for m in two.members[0]] == [0] and two.plans == [parents[1]] and two.plans[0].name == parents[1].name
    # max_generations = 1 stops there (the four sampled plans breed children: test 1)
    first = _front(eng, sets, "sampled", 256, 16384, SEED, 1)
    assert first.stop_reason == "max_generations" and len(first.generations) == 1 and first.generations[0].n_children_kept > 0


def test_full_parents_skip_the_children_that_outgrow_a_list(eng):
    rng = np.random.default_rng(3)
    f1, f2 = _full_plan(rng, 3, 13, 25, 1), _full_plan(rng, 20, 10, 18, 22)
    every = cross_pairs(2, CUTS)
    fit = [x for x in every if x.a == x.b or _fits([f1, f2], x)]
    assert 2 <= len(fit) < len(every)
    front = eng.breed_front(ActionWeights(), [f1, f2], 1, 0, cuts=CUTS, generations=1)
    row = front.generations[0]
    assert (row.n_parents, row.n_skipped, row.n_variants) == (2, len(every) - len(fit), len(fit)) and row.n_skipped > 0
    assert front.stop_reason in ("max_generations", "converged", "empty")
    assert [m.cross for m in front.members[0]] == [fit[m.variant] for m in front.members[0]]
    assert front.plans == front.lineage([f1, f2])[-1]


def test_a_generation_without_a_valid_variant_returns_its_population(eng):
    from tests.test_gpu_refine_many import _failing_base
    pol, bad = ActionWeights(), _failing_base()
    bad.name = "overflows"
    assert eng.evaluate_plans(pol, [bad], SEED, INDEX).status[0] != N.EG_EP_OK      # (the run record overflows)
    front = eng.breed_front(pol, [bad, bad], SEED, INDEX, cuts=CUTS, generations=3)
    assert front.stop_reason == "empty" and _rows(front) == [(2, 0, 0, 0, 8, 0, 0)] and front.members == [[]]
    assert front.plans == [bad, bad] and [p.name for p in front.plans] == ["overflows", "overflows"]
    assert front.records is None and front.metrics.shape == (0, 4) and front.lineage([bad, bad]) == [[bad, bad]]


def test_a_run_to_convergence_and_one_more_call(eng, sets):
    pol, parents, _, _ = sets["sampled"]
    kw = dict(objectives=("emissions", "cost"), cost_only=True, cuts=CUTS, generations=12, cap=4)
    front = eng.breed_front(pol, parents, SEED, INDEX, **kw)
    print("convergence", _rows(front), front.stop_reason)
    assert front.stop_reason == "converged" and 2 <= len(front.generations) <= 12
    last = front.generations[-1]
    assert last.n_kept == last.n_parents and last.n_children_kept == 0
    again = eng.breed_front(pol, front.plans, SEED, INDEX, **kw)
    assert again.stop_reason == "converged" and len(again.generations) == 1
    assert again.plans == front.plans and [p.name for p in again.plans] == [p.name for p in front.plans]
    assert again.metrics.tobytes() == front.metrics.tobytes() and again.score.tobytes() == front.score.tobytes()


# ---------------------------------------------------------------- 6: side effects
def test_breeding_touches_nothing_else(eng, sets, tmp_path):
    import re
    from eirgrid_amd.world import World
    pol_eval, parents, _, _ = sets["sampled"]
    world = World.from_json_dict(json.load(open(WORLD)))
    kw = dict(cuts=CUTS, generations=2, cap=8, max_variants=30)
    want = eng.breed_front(pol_eval, parents, SEED, INDEX, **kw)
    out = []
    for breed in (False, True):
        e = Engine(world, device=0)
        try:
            e.push(ActionWeights())
            e.track_best_result()
            e.track_top_k(10)
            e.track_pareto(16)
            for step in range(3):
                e.device_step(3, 256 * step, 256, 10, 3 + step)
                if breed and step < 2:
                    f = e.breed_front(pol_eval, parents, SEED, INDEX, **kw)
                    # (a context that has never held a plan batch, and whose plan pool grows from generation to generation)
                    assert _rows(f) == _rows(want) and _members(f) == _members(want) and f.plans == want.plans and f.stop_reason == want.stop_reason
                    last = f.generations[-1].n_variants
                    assert N.lib().eg_last_batch_size(e.h) == (last % 30 or 30)      # the last chunk stays behind
            batch = e.fetch(256)
            pol = ActionWeights(); e.pull(pol)
            path = tmp_path / f"policy_{breed}.json"
            pol.save_to_file(path)
            text = re.sub(r'"timestamp": "[^"]*"', '"timestamp": ""', path.read_text())
            idx, best = e.fetch_best_result()
            rows, scores, index = e.fetch_top_k()
            par = e.fetch_pareto()
            out.append((text, batch, idx, best, rows, scores.tobytes(), index.tobytes(), par))
        finally:
            e.close()
    (pa, la, ia, ba, ra, sa, xa, fa), (pb, lb, ib, bb, rb, sb, xb, fb) = out
    assert pa == pb and ia == ib and sa == sb and xa == xb
    _same_records(la, lb, "last batch")
    _same_records(ba, bb, "best_result")
    _same_records(ra, rb, "top-k")
    # the context's own Pareto archive: index, metrics, n_dropped
    assert len(fa[1]) >= 1 and fa[1].tolist() == fb[1].tolist() and fa[2].tobytes() == fb[2].tobytes() and fa[3] == fb[3]
    assert fa[0].metrics.tobytes() == fb[0].metrics.tobytes()


def test_refusals_launch_nothing(eng, sets):
    pol, parents, _, _ = sets["sampled"]
    prev = eng.evaluate_plans(pol, parents[:2], 9, 40)
    with pytest.raises(EirgridError, match=r"eg_breed_validate: cap 0 is outside 1\.\.EG_PARETO_MAX \(256\)"):
        eng.breed_front(pol, parents, SEED, INDEX, cap=0)
    with pytest.raises(EirgridError, match=r"eg_breed_validate: cuts\[1\] = 26 \(a year index 1\.\.25\)"):
        eng.breed_front(pol, parents, SEED, INDEX, cuts=(5, 26))
    assert N.lib().eg_last_batch_size(eng.h) == 2
    got = eng.fetch()
    for name in _ALL_FIELDS + ("n_chunks",):
        assert _used(got, name).tobytes() == _used(prev, name).tobytes(), name


def test_a_rank_of_a_group_is_refused():
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import Group
    g = Group(synthetic_world(), devices=(0, 0))
    try:
        base = Plan([[3, 12]] + [[] for _ in range(25)], [[] for _ in range(26)])
        with pytest.raises(EirgridError, match="eg_breed_plans: the context is a rank of an eg_group"):
            g.ranks[0].breed_front(ActionWeights(), [base, base], 1)
    finally:
        g.close()


# ---------------------------------------------------------------- 7: the script
def test_the_script_writes_the_population(eng, sets, tmp_path):
    pol, parents, _, _ = sets["sampled"]
    ckpt, plan_file, out_dir = str(tmp_path / "policy.json"), str(tmp_path / "parents.jsonl"), str(tmp_path / "run")
    pol.save_to_file(ckpt)
    Plan.save(plan_file, parents)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "breed_front.py"), "--world", WORLD, "--plans", plan_file, "--policy", ckpt, "--seed", str(SEED),
                          "--generations", "2", "--cap", "8", "--cuts", "2030,2038,2045", "--out", out_dir], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    want = eng.breed_front(ActionWeights.load_from_file(ckpt), Plan.load(plan_file), SEED, 0, cuts=CUTS, generations=2, cap=8)
    d = os.path.join(out_dir, "breed")
    assert sorted(os.listdir(d)) == ["generations.csv", "index.csv", "plans.jsonl"]
    back = Plan.load(os.path.join(d, "plans.jsonl"))
    assert back == want.plans and [p.name for p in back] == [p.name for p in want.plans]
    index = list(csv.DictReader(open(os.path.join(d, "index.csv"))))
    assert [r["name"] for r in index] == [p.name for p in want.plans]
    assert [r["score"] for r in index] == ["%.17g" % s for s in want.score]
    gens = list(csv.DictReader(open(os.path.join(d, "generations.csv"))))
    assert [(int(r["n_parents"]), int(r["n_variants"]), int(r["n_kept"]), int(r["n_children_kept"])) for r in gens] == \
           [(g.n_parents, g.n_variants, g.n_kept, g.n_children_kept) for g in want.generations]
