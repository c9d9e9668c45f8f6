"""GPU: a Pareto local search over one-entry edits and moves with the archive and its frontier on the device (include/eirgrid_hip.h
eg_explore_plans; csrc/eg_explore.h k_explore_turnover; csrc/eg_explore.cpp) against a restatement written out here: a Python generation
loop that enumerates the neighbourhoods as the header does (refine_edits / refine_moves), evaluates every base's variants with the
existing Engine.evaluate_plan_edits / evaluate_plan_moves(..., same_index=True) over the host-built plan, and folds chunk by chunk,
with running numbers, into ONE O(n^2) restatement of the archive's streaming rule (tests/test_pareto.py Front, capacity included) that
lives through the call.  Scores and metrics are compared as bytes.  Everything runs on tests/golden/world_v1.json."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanEdit, PlanMove, rank_score, refine_edits, refine_moves
from tests.test_gpu_breed import _same_records_but_n_chunks
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plan_crosses import SHORT_MAX, _record_parents
from tests.test_gpu_plans import _same_records
from tests.test_pareto import Front, valid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
ALL = ("emissions", "opinion", "cost", "reliability")
SEED, INDEX = 91, 7
DELETES = dict(replace_with=None, append_with=None, max_shift=0)
EDITS = dict(replace_with=(12,), append_with=(9, 60), max_shift=0)
MOVES = dict(replace_with=None, append_with=None, max_shift=2)
# test 3 (cap 4, chunks of 37, deletes only): the plans of this file replay to the end without a fallback draw, so the evaluation seed
# does not move them; what a seed moves is which four episodes are sampled as start plans.  SAMPLE_CAP is the sampling seed at which the
# RESTATEMENT alone drops for want of room and, after some generation, holds a neighbour while a start plan has left — looked for with
# the restatement only (sampling seeds 1, 2, 3, ... in order; the first that does both)
SAMPLE_CAP = 1


def _mask(objectives):
    return sum(1 << ALL.index(o) for o in objectives)


def _apply(plan, edit):
    """an edit or a move applied by hand (not PlanEdit.apply / PlanMove.apply, which lineage uses)"""
    lists = ([list(l) for l in plan.best_actions], [list(l) for l in plan.best_deficit_actions])
    if isinstance(edit, PlanMove):
        a = lists[edit.list][edit.year][edit.pos]
        lists[edit.list][edit.year] = lists[edit.list][edit.year][:edit.pos] + lists[edit.list][edit.year][edit.pos + 1:]
        to = lists[edit.list][edit.to_year]
        lists[edit.list][edit.to_year] = to[:edit.to_pos] + [a] + to[edit.to_pos:]
    else:
        l = lists[edit.list][edit.year]
        if edit.kind == "delete":
            lists[edit.list][edit.year] = l[:edit.pos] + l[edit.pos + 1:]
        elif edit.kind == "replace":
            lists[edit.list][edit.year] = l[:edit.pos] + [edit.action] + l[edit.pos + 1:]
        elif edit.kind == "insert":
            lists[edit.list][edit.year] = l[:edit.pos] + [edit.action] + l[edit.pos:]
    return Plan(lists[0], lists[1])


def _hood(plan, kw):
    return refine_edits(plan, kw["replace_with"], kw["append_with"])[1:], refine_moves(plan, kw["max_shift"])


def explore_restated(eng, pol, starts, seed, index, objectives, cost_only, generations, cap, launch, kw, max_variants=0):
    """The header's loop, on the host: {rows: a tuple per generation in ExploreGeneration's field order, members: [row][(parent, edit,
    number, score bytes, metrics bytes)], stop, plans: {number: Plan} of everything that ever was a member or a start plan, numbers:
    the archive's at the end, routes: the set of (base is long, variant is long) seen}."""
    score = lambda m: rank_score(m, cost_only)
    arch = Front(cap, _mask(objectives), score)
    n = len(starts)
    plans = {p: starts[p] for p in range(n)}
    frontier, number, rows, members, stop, routes, all_held = list(range(n)), 0, [], [], "max_generations", set(), []
    for g in range(generations):
        gen_first = number
        variants = [(-1, PlanEdit())] * n if g == 0 else []      # (parent number, edit) by position in the generation
        metrics, status = [], []
        nones = []
        per_base = []
        for k in frontier:
            edits, moves = _hood(plans[k], kw)
            m, s = np.zeros((0, 4)), np.zeros(0, np.int32)
            if g == 0 or edits:      # (generation 0: the start plan itself rides in front of its edits)
                res = eng.evaluate_plan_edits(pol, plans[k], ([PlanEdit()] if g == 0 else []) + edits, seed, index, same_index=True)
                cnt = len(edits) + (g == 0)
                m, s = res.metrics[:cnt], res.status[:cnt]
                if g == 0:
                    nones.append((m[0], s[0]))
                    m, s = m[1:], s[1:]
            if moves:
                res = eng.evaluate_plan_moves(pol, plans[k], moves, seed, index, same_index=True)
                m, s = np.concatenate([m, res.metrics[:len(moves)]]), np.concatenate([s, res.status[:len(moves)]])
            per_base.append((m, s))
            variants += [(k, e) for e in edits + moves]
            deltas = {((e.kind == "insert") - (e.kind == "delete")) * (e.list == 0) for e in edits} | ({0} if moves else set())
            routes |= {(len(plans[k]) > SHORT_MAX, len(plans[k]) + d > SHORT_MAX) for d in deltas}
        metrics = np.concatenate([np.array([m for m, _ in nones]).reshape(-1, 4)] + [m for m, _ in per_base]).reshape(-1, 4)
        status = np.concatenate([np.array([s for _, s in nones], np.int32)] + [s for _, s in per_base])
        V = len(variants)
        assert len(metrics) == V == len(status)
        for first in range(0, V, launch):
            arch.fold(metrics[first:first + launch], status[first:first + launch], gen_first + first)
        number += V
        m_first = gen_first + (n if g == 0 else 0)
        held = [int(k) for k in arch.index]
        new = [k for k in held if k >= m_first]
        entry = {int(k): (np.float64(score(m)).tobytes(), np.ascontiguousarray(m).tobytes()) for k, m in zip(arch.index, arch.m)}
        rows.append((len(frontier), len(held), len(new), V, int(valid(metrics, status).sum()), arch.n_dropped))
        all_held.append(held)
        if not held:
            stop = "empty"
            break
        if g == 0:
            members.append([(-1, PlanEdit(), k) + entry[k] for k in held if k < n])
        members.append([variants[k - gen_first] + (k,) + entry[k] for k in new])
        for k in new:
            parent, edit = variants[k - gen_first]
            plans[k] = _apply(plans[parent], edit)
        frontier = new
        if not new:
            stop = "explored"
            break
        want = sum(len(e) + len(m) for e, m in (_hood(plans[k], kw) for k in new))
        if max_variants and number + want > max_variants:
            stop = "budget"
            break
    return {"rows": rows, "members": members, "stop": stop, "plans": plans, "numbers": [int(k) for k in arch.index], "routes": routes, "held": all_held}


def _rows(front):
    return [(r.n_frontier, r.n_held, r.n_new, r.n_variants, r.n_valid, r.n_dropped) for r in front.generations]


def _members(front):
    return [[(m.parent, m.edit, m.number, np.float64(m.score).tobytes(), np.array(m.metrics, np.float64).tobytes()) for m in row] for row in front.members]


def _assert_is(front, ref, what):
    print(what, "rows", ref["rows"], ref["stop"])
    assert front.stop_reason == ref["stop"], (what, front.stop_reason, ref["stop"])
    assert _rows(front) == ref["rows"], (what, _rows(front), ref["rows"])
    got = _members(front)
    assert len(got) == len(ref["members"]), what
    for g, (a, b) in enumerate(zip(got, ref["members"])):
        assert a == b, (what, "members row", g, [m[:3] for m in a], [m[:3] for m in b])
    assert front.numbers.tolist() == ref["numbers"], what
    assert front.plans == [ref["plans"][k] for k in ref["numbers"]], what


@pytest.fixture(scope="module")
def eng(built):
    from eirgrid_amd.world import World
    e = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    yield e
    e.close()


def _sampled(eng, pol, seed):
    res = eng.rollout_batch(pol, seed, 4)
    return [Plan.from_result(res, e, f"sampled {e}") for e in range(4)]


@pytest.fixture(scope="module")
def sets(eng):
    """{name: (policy, start plans, objectives, cost_only)} — four sampled episodes under all four objectives; a short, a long and four
    crafted plans (tests/test_gpu_plan_crosses.py _record_parents) under emissions and cost; four episodes sampled at SAMPLE_CAP"""
    pol = ActionWeights()
    cpol, crafted, _ = _record_parents(eng, np.random.default_rng(17))
    lens = [len(p) for p in crafted]
    assert min(lens) <= SHORT_MAX < max(lens)
    return {"sampled": (pol, _sampled(eng, pol, 4711), ALL, False), "crafted": (cpol, crafted, ("emissions", "cost"), True),
            "sampled4": (pol, _sampled(eng, pol, SAMPLE_CAP), ALL, False)}


_CACHE = {}


def _key(kw):
    return tuple(sorted((k, tuple(v) if v is not None and k != "max_shift" else v) for k, v in kw.items()))


def _ref(eng, sets, name, cap, launch, kw, generations=3, max_variants=0):
    key = ("ref", name, cap, launch, _key(kw), generations, max_variants)
    if key not in _CACHE:
        pol, starts, objectives, cost_only = sets[name]
        _CACHE[key] = explore_restated(eng, pol, starts, SEED, INDEX, objectives, cost_only, generations, cap, launch, kw, max_variants)
    return _CACHE[key]


def _front(eng, sets, name, cap, launch, kw, generations=3, max_variants=0):
    key = ("front", name, cap, launch, _key(kw), generations, max_variants)
    if key not in _CACHE:
        pol, starts, objectives, cost_only = sets[name]
        _CACHE[key] = eng.explore_front(pol, starts, SEED, INDEX, objectives=objectives, cost_only=cost_only, generations=generations, cap=cap, launch=launch,
                                        max_variants=max_variants, **kw)
    return _CACHE[key]


# ---------------------------------------------------------------- 1: one generation is the host fold of the neighbourhoods
@pytest.mark.parametrize("name", ["sampled", "crafted"])
def test_one_generation_is_the_host_fold_of_the_neighbourhoods(eng, sets, name):
    ref = _ref(eng, sets, name, 256, 16384, MOVES, generations=1)
    front = _front(eng, sets, name, 256, 16384, MOVES, generations=1)
    _assert_is(front, ref, (name, "one generation"))
    starts = sets[name][1]
    row = front.generations[0]
    assert len(front.generations) == 1 and len(front.members) == 2
    assert row.n_frontier == len(starts) and row.n_variants == len(starts) + sum(len(e) + len(m) for e, m in (_hood(p, MOVES) for p in starts))
    assert row.n_dropped == 0 and row.n_held == len(front.plans) >= 1 and row.n_new == len(front.members[1])
    assert front.stop_reason == ("max_generations" if row.n_new else "explored")
    assert all(m.parent == -1 and m.edit == PlanEdit() and m.number < len(starts) for m in front.members[0])
    assert all(0 <= m.parent < len(starts) and m.number >= len(starts) for m in front.members[1])
    if row.n_variants <= 16384:
        assert N.lib().eg_last_batch_size(eng.h) == row.n_variants      # (one chunk)


# ---------------------------------------------------------------- 2: three generations, one chunk and chunks of 37
@pytest.mark.parametrize("kind", ["deletes", "edits", "moves"])
@pytest.mark.parametrize("name", ["sampled", "crafted"])
def test_three_generations_are_the_restatement_whatever_the_chunks(eng, sets, name, kind):
    kw = {"deletes": DELETES, "edits": EDITS, "moves": MOVES}[kind]
    ref = _ref(eng, sets, name, 256, 16384, kw)
    whole, chunked = _front(eng, sets, name, 256, 16384, kw), _front(eng, sets, name, 256, 37, kw)
    _assert_is(whole, ref, (name, kind, "chunks of 16 384"))
    _assert_is(chunked, ref, (name, kind, "chunks of 37"))
    assert _rows(whole) == _rows(chunked) and _members(whole) == _members(chunked) and whole.plans == chunked.plans
    assert whole.numbers.tolist() == chunked.numbers.tolist() and whole.metrics.tobytes() == chunked.metrics.tobytes()
    assert all(r.n_dropped == 0 for r in whole.generations)
    assert sum(r.n_new for r in whole.generations) > 0 and min(r.n_variants for r in whole.generations if r.n_variants) > 37      # (neighbours entered, several chunks)
    if kind == "moves":      # a cut at 37 leaves a chunk with moves only: a start plan has more than 2 * 37 moves in a row
        assert any(len(_hood(p, kw)[1]) > 74 for p in sets[name][1])
    if name == "crafted":      # the members cross kShortReplayMax both ways
        lens = [len(p) for p in ref["plans"].values()]
        assert min(lens) <= SHORT_MAX < max(lens)
    # a later generation holds nothing but the neighbourhoods of the members that entered in the one before
    for g in range(1, len(whole.generations)):
        assert whole.generations[g].n_frontier == whole.generations[g - 1].n_new == len(whole.members[g])
        assert {m.parent for m in whole.members[g + 1]} <= {m.number for m in whole.members[g]}


# ---------------------------------------------------------------- 3: capacity
def test_a_small_cap_drops_by_the_streaming_rule(eng, sets):
    ref = _ref(eng, sets, "sampled4", 4, 37, DELETES)
    rows = ref["rows"]
    # (the reference alone:) room ran out, and after a generation the archive held a neighbour while a start plan had left
    assert any(r[5] > 0 for r in rows), rows
    assert any(any(k >= 4 for k in held) and sum(k < 4 for k in held) < 4 for held in ref["held"]), ref["held"]
    front = _front(eng, sets, "sampled4", 4, 37, DELETES)
    _assert_is(front, ref, "cap 4")
    assert any(r.n_dropped > 0 for r in front.generations) and all(r.n_held <= 4 for r in front.generations)


# ---------------------------------------------------------------- 4: the replay routes
def _truncated(plan, n_entries, name):
    """the first n_entries best_actions entries of a plan, in year order"""
    run, left = [], n_entries
    for l in plan.best_actions:
        run.append(list(l[:left])); left -= len(run[-1])
    assert left == 0
    return Plan(run, plan.best_deficit_actions, name)


def test_variants_change_the_replay_route_of_their_base(eng, sets):
    pol, crafted, objectives, cost_only = sets["crafted"]
    long_ = max(crafted, key=len)
    starts = [_truncated(long_, SHORT_MAX, "96"), _truncated(long_, SHORT_MAX + 1, "97")]
    assert [len(p) for p in starts] == [SHORT_MAX, SHORT_MAX + 1]
    kw = dict(replace_with=None, append_with=(9,), max_shift=1)
    ref = explore_restated(eng, pol, starts, SEED, INDEX, ALL, False, 2, 256, 37, kw)
    # the appends of the first take the long route, the deletes of the second the short one; and both stay where they are with a move
    assert ref["routes"] >= {(False, False), (False, True), (True, True), (True, False)}, ref["routes"]
    front = eng.explore_front(pol, starts, SEED, INDEX, generations=2, launch=37, **kw)
    _assert_is(front, ref, "routes")
    assert front.generations[0].n_new > 0 and any(k >= 2 for k in front.numbers.tolist())
    line = front.lineage(starts)[-1]
    for r, k in enumerate(front.numbers.tolist()):
        assert front.plans[r] == line[k] == ref["plans"][k]
        one = eng.evaluate_plans(pol, [ref["plans"][k]], SEED, INDEX)
        _same_records_but_n_chunks(front.records, one, ("routes", "record", r), [r], [0])


# ---------------------------------------------------------------- 5: population, lineage, records
@pytest.mark.parametrize("name,cap,launch,kind", [("sampled", 256, 37, "moves"), ("crafted", 256, 16384, "edits"), ("sampled4", 4, 37, "deletes")])
def test_the_population_is_the_lineage_and_its_records_are_the_plans(eng, sets, name, cap, launch, kind):
    kw = {"deletes": DELETES, "edits": EDITS, "moves": MOVES}[kind]
    pol, starts, _, _ = sets[name]
    front = _front(eng, sets, name, cap, launch, kw)
    ref = _ref(eng, sets, name, cap, launch if cap == 4 else 16384, kw)
    line = front.lineage(starts)
    assert len(line) == len(front.members) == len(ref["members"])
    for row, known in zip(front.members, line):      # (PlanEdit.apply / PlanMove.apply against the tests' _apply)
        assert all(known[m.number] == ref["plans"][m.number] for m in row)
    want = [line[-1][k] for k in front.numbers.tolist()]
    assert len(front.plans) == len(want) >= 1
    for r, (got, w) in enumerate(zip(front.plans, want)):
        assert got.best_actions == w.best_actions and got.best_deficit_actions == w.best_deficit_actions, (name, "plan", r)
        assert got.name == w.name, (name, r, got.name, w.name)
    assert any(k >= len(starts) for k in front.numbers.tolist())      # (a neighbour is held)
    assert front.records is not None and len(front.records.status) == len(front.plans)
    step = max(1, len(front.plans) // 12)      # (a dozen of them, the first and the last among them)
    for r in sorted(set(range(0, len(front.plans), step)) | {len(front.plans) - 1}):
        one = eng.evaluate_plans(pol, [front.plans[r]], SEED, INDEX)
        _same_records_but_n_chunks(front.records, one, (name, "record", r), [r], [0])
    assert front.records.metrics.tobytes() == front.metrics.tobytes()


# ---------------------------------------------------------------- 6: running to the end
def test_a_run_to_the_end_and_one_more_call(eng, sets):
    pol, starts, _, _ = sets["sampled"]
    # (a delete can only lower the cost, and a generation moves the one held point by one entry: at most one generation per entry of the
    # largest start plan, 40 + 13, and one more)
    kw = dict(objectives=("cost",), cost_only=True, generations=64, cap=8)
    front = eng.explore_front(pol, starts, SEED, INDEX, **kw)
    print("to the end", _rows(front), front.stop_reason)
    assert max(len(p) + sum(len(l) for l in p.best_deficit_actions) for p in starts) < 63
    assert front.stop_reason == "explored" and 2 <= len(front.generations) <= 64
    assert front.generations[-1].n_new == 0 and front.members[-1] == [] and all(r.n_dropped == 0 for r in front.generations)
    assert len(front.plans) == 1      # (one objective: one point)
    again = eng.explore_front(pol, front.plans, SEED, INDEX, **kw)
    assert again.stop_reason == "explored" and len(again.generations) == 1 and again.generations[0].n_new == 0
    assert again.plans == front.plans and [p.name for p in again.plans] == [p.name for p in front.plans]
    assert again.metrics.tobytes() == front.metrics.tobytes() and again.score.tobytes() == front.score.tobytes()


# ---------------------------------------------------------------- 7: the budget
def test_a_budget_one_short_of_the_second_generation_stops_after_the_first(eng, sets):
    pol, starts, objectives, cost_only = sets["sampled"]
    two = _front(eng, sets, "sampled", 256, 16384, DELETES, generations=2)
    one = _front(eng, sets, "sampled", 256, 16384, DELETES, generations=1)
    assert len(two.generations) == 2
    need = two.generations[0].n_variants + two.generations[1].n_variants
    short = eng.explore_front(pol, starts, SEED, INDEX, generations=3, max_variants=need - 1, **DELETES)
    assert short.stop_reason == "budget" and one.stop_reason == "max_generations"
    assert _rows(short) == _rows(one) and _members(short) == _members(one) and short.plans == one.plans and short.numbers.tolist() == one.numbers.tolist()
    assert short.records.metrics.tobytes() == one.records.metrics.tobytes()
    # with exactly the need the second generation runs; the budget is looked at before the generation cap, and a third would not fit
    enough = eng.explore_front(pol, starts, SEED, INDEX, generations=2, max_variants=need, **DELETES)
    assert two.stop_reason == "max_generations" and two.generations[1].n_new > 0
    assert enough.stop_reason == "budget" and _rows(enough) == _rows(two) and _members(enough) == _members(two) and enough.plans == two.plans


# ---------------------------------------------------------------- 8: a full list
def test_a_full_list_gets_no_appends(eng):
    rng = np.random.default_rng(3)
    run = [[int(a) for a in rng.integers(0, 61, 150)] for _ in range(26)]
    run[13] = []
    run[3] += [int(a) for a in rng.integers(0, 61, 4096 - 25 * 150)]
    empty = [[] for _ in range(26)]
    full = Plan(run, [[24]] + empty[1:], "full")
    small = Plan([[3, 12]] + empty[1:], empty, "small")
    assert len(full) == 4096
    pol = ActionWeights()
    kw = dict(replace_with=None, append_with=(9,), max_shift=0)
    ref = explore_restated(eng, pol, [full, small], 1, 0, ALL, False, 1, 256, 16384, kw)
    front = eng.explore_front(pol, [full, small], 1, 0, generations=1, **kw)
    _assert_is(front, ref, "a full list")
    assert front.generations[0].n_variants == 2 + (4096 + 1) + (2 + 26)
    assert all(len(p) <= 4096 for p in front.plans)
    assert not any(m.parent == 0 and m.edit.kind == "insert" for m in front.members[1])


# ---------------------------------------------------------------- 9: nothing valid
def test_a_call_without_a_valid_variant_returns_the_start_plans(eng):
    from tests.test_gpu_refine import _overflow_base
    pol, base = ActionWeights(), _overflow_base()
    bad = Plan(base.best_actions[:25] + [base.best_actions[25] + [60] * 40], base.best_deficit_actions, "overflows")
    ref = explore_restated(eng, pol, [bad, bad], SEED, INDEX, ALL, False, 3, 256, 16384, DELETES)
    assert ref["stop"] == "empty" and ref["rows"][0][4] == 0, ref["rows"]      # (the run record overflows, with an entry less as well)
    front = eng.explore_front(pol, [bad, bad], SEED, INDEX, generations=3, **DELETES)
    assert front.stop_reason == "empty" and _rows(front) == ref["rows"] and front.members == []
    assert _rows(front)[0][:3] == (2, 0, 0)
    assert front.plans == [bad, bad] and [p.name for p in front.plans] == ["overflows", "overflows"]
    assert front.records is None and front.metrics.shape == (0, 4) and len(front.numbers) == 0 and front.lineage([bad, bad]) == []


# ---------------------------------------------------------------- 10: side effects
def test_exploring_touches_nothing_else(eng, sets, tmp_path):
    import re
    from eirgrid_amd.world import World
    pol_eval, starts, _, _ = sets["sampled"]
    world = World.from_json_dict(json.load(open(WORLD)))
    kw = dict(generations=2, cap=8, launch=300, max_shift=1)
    want = eng.explore_front(pol_eval, starts, SEED, INDEX, **kw)
    out = []
    for explore in (False, True):
        e = Engine(world, device=0)
        try:
            e.push(ActionWeights())
            e.track_best_result()
            e.track_top_k(10)
            e.track_pareto(16)
            for step in range(3):
                e.device_step(3, 256 * step, 256, 10, 3 + step)
                if explore and step < 2:
                    f = e.explore_front(pol_eval, starts, SEED, INDEX, **kw)
                    # (a context that has never held a plan batch, and whose plan pool grows from generation to generation)
                    assert _rows(f) == _rows(want) and _members(f) == _members(want) and f.plans == want.plans and f.stop_reason == want.stop_reason
                    last = f.generations[-1].n_variants
                    assert N.lib().eg_last_batch_size(e.h) == (last % 300 or 300)      # the last chunk stays behind
            batch = e.fetch(256)
            pol = ActionWeights(); e.pull(pol)
            path = tmp_path / f"policy_{explore}.json"
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


# ---------------------------------------------------------------- 11: refusals and the script
def test_refusals_launch_nothing(eng, sets):
    pol, starts, _, _ = sets["sampled"]
    prev = eng.evaluate_plans(pol, starts[:2], 9, 40)
    with pytest.raises(EirgridError, match=r"eg_explore_validate: cap 0 is outside 1\.\.EG_PARETO_MAX \(256\)"):
        eng.explore_front(pol, starts, SEED, INDEX, cap=0)
    with pytest.raises(EirgridError, match=r"eg_explore_validate: append_with\[1\]: action 61 >= 61"):
        eng.explore_front(pol, starts, SEED, INDEX, append_with=(5, 61))
    with pytest.raises(EirgridError, match=r"eg_explore_validate: max_shift = 26 \(0\.\.25 years; 0: no moves\)"):
        eng.explore_front(pol, starts, SEED, INDEX, max_shift=26)
    with pytest.raises(EirgridError, match=r"eg_explore_validate: max_variants = -1 \(0: no budget\)"):
        eng.explore_front(pol, starts, SEED, INDEX, max_variants=-1)
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
        with pytest.raises(EirgridError, match="eg_explore_plans: the context is a rank of an eg_group"):
            g.ranks[0].explore_front(ActionWeights(), [base, base], 1)
    finally:
        g.close()


def test_the_script_writes_the_population(eng, sets, tmp_path):
    pol, starts, _, _ = sets["sampled"]
    ckpt, plan_file, out_dir = str(tmp_path / "policy.json"), str(tmp_path / "starts.jsonl"), str(tmp_path / "run")
    pol.save_to_file(ckpt)
    Plan.save(plan_file, starts)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "explore_front.py"), "--world", WORLD, "--plans", plan_file, "--policy", ckpt, "--seed", str(SEED),
                          "--generations", "2", "--cap", "8", "--append", "9", "--shift", "1", "--out", out_dir], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    want = eng.explore_front(ActionWeights.load_from_file(ckpt), Plan.load(plan_file), SEED, 0, generations=2, cap=8, append_with=(9,), max_shift=1)
    d = os.path.join(out_dir, "explore")
    assert sorted(os.listdir(d)) == ["generations.csv", "index.csv", "plans.jsonl"]
    back = Plan.load(os.path.join(d, "plans.jsonl"))
    assert back == want.plans and [p.name for p in back] == [p.name for p in want.plans]
    index = list(csv.DictReader(open(os.path.join(d, "index.csv"))))
    assert [r["name"] for r in index] == [p.name for p in want.plans] and [int(r["number"]) for r in index] == want.numbers.tolist()
    assert [r["score"] for r in index] == ["%.17g" % s for s in want.score]
    gens = list(csv.DictReader(open(os.path.join(d, "generations.csv"))))
    assert [(int(r["n_frontier"]), int(r["n_variants"]), int(r["n_held"]), int(r["n_new"])) for r in gens] == \
           [(g.n_frontier, g.n_variants, g.n_held, g.n_new) for g in want.generations]
    assert gens[-1]["stop"] == want.stop_reason
