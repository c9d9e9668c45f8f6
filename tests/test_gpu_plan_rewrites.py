"""GPU: plan rewrites (include/eirgrid_hip.h eg_evaluate_plan_rewrites; csrc/eg_plan_rewrites.h k_plan_rewrites; eg_plans.cpp).  Variant j of
a plan-rewrite batch is a plan with an action map applied to every entry of a window of years of the selected lists, evaluated exactly as
eg_evaluate_plans evaluates the host-built child: the plan blocks the device writes must equal, byte for byte, the blocks the host
builds for the children, the records must be those of the host-built children and the tabled oracle's, and Engine.technology_report must
return the rows of a host loop over the children without touching the context's archive."""
import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.engine import ActionMap, ActionWeights, HostTables, Plan, PlanRewrite, rank_score, technology_rewrites
from oracle import api as O
from tests.helpers import assert_episode_equal
from tests.test_gpu_plan_crosses import _counted, _full_plan, _lists, _offsets
from tests.test_gpu_plan_edits import _junk_plan, _long_policy
from tests.test_gpu_plans import _engine, _oracle_plan, _same_records
from tests.test_gpu_replay_hoist import _seeded
from tests.test_plan_rewrites import apply_rewrite

pytestmark = pytest.mark.gpu

SHORT_MAX = 96      # kShortReplayMax (csrc/eg_internal.h): the best_actions length up to which a plan takes the short replay route
DROP = 0xFF


def _labels(plans, maps, rw, which):
    """what rewrite rw exercises on list `which` of the kernel's window compaction and of what it writes around it, by name"""
    out = {f"lists {rw.lists}"}
    if rw.map > 0:
        out.add("map index above 0")
    if rw.plan > 0:
        out.add("plan index above 0")
    f, t = rw.from_year, rw.to_year
    if f == t:
        out.add("empty window")
    if not rw.lists >> which & 1:
        return out
    plan, to = plans[rw.plan], maps[rw.map].to
    o = _offsets(plan, which)
    flat = [a for l in _lists(plan, which) for a in l]
    s0, s1, total = int(o[f]), int(o[t]), int(o[26])
    window = flat[s0:s1]
    kept = [to[e] != DROP for e in window]
    K = sum(kept)
    child = total - (len(window) - K)
    if f == 0:
        out.add("from = 0")
    if t == 26:
        out.add("to = 26")
    if f == 0 and t == 26:
        out.add("whole plan")
    if f < t and 0 in (len(_lists(plan, which)[f]), len(_lists(plan, which)[t - 1])):
        out.add("empty year at a window edge")
    if total == 0:
        out.add("empty plan")
    if window:
        out.add(f"start {s0 % 8} kept {K % 8}")
        if K == 0:
            out.add("window wholly dropped")
        if K == len(window) and [to[e] for e in window] != window:
            out.add("nothing dropped but values changed")
        if K == len(window) and [to[e] for e in window] == window and any(v == DROP for v in to):
            out.add("a dropping map that drops nothing it meets")
        if 0 < K < len(window):
            out.add("some dropped")
        # runs of dropped entries, by their source positions: across an 8-byte word, across a 512-byte step of the wave (the steps start
        # at the word that holds the window's start)
        base = 8 * (s0 // 8)
        i = 0
        while i < len(window):
            if kept[i]:
                i += 1
                continue
            j = i
            while j + 1 < len(window) and not kept[j + 1]:
                j += 1
            if (s0 + i) // 8 != (s0 + j) // 8:
                out.add("dropped run across a word boundary")
            if (s0 + i - base) // 512 != (s0 + j - base) // 512:
                out.add("dropped run across a 512-byte step boundary")
            i = j + 1
        if any(len(l) > 512 for l in _lists(plan, which)[f:t]):
            out.add("window year of more than 512 entries")
        if any(len(l) > 64 for l in _lists(plan, which)[f:t]):
            out.add("window year of more than 64 entries")
    if child <= total - 512:
        out.add("child much shorter than its parent")
    if total == 4096 and child == 0:
        out.add("child of 0 entries from a full plan")
    if total == 4096 and child == 4096 and [to[e] for e in window] != window:
        out.add("full plan, values changed, nothing dropped")
    if which == 0 and total > SHORT_MAX and child <= SHORT_MAX:
        out.add("long parent, short child")
    return out


def _residue_cover(labels):
    """{residue of the window's start: the residues of the kept length it met}"""
    cover = {r: set() for r in range(8)}
    for l in labels:
        if l.startswith("start "):
            cover[int(l.split()[1])].add(int(l.split()[3]))
    return cover


def _check_blocks(eng, pol, plans, maps, rewrites, what):
    """The plan blocks k_plan_rewrites writes against the blocks the host's write_lists builds for the children, all 8 832 bytes of each
    (eg_debug_fetch_plan_block) — with the pool overwritten in between, so that nothing is left over from the host's blocks."""
    n = len(rewrites)
    children = [apply_rewrite(plans, maps, rw) for rw in rewrites]
    assert all(rw.apply(plans, maps) == c for rw, c in zip(rewrites, children))
    eng.evaluate_plans(pol, children, 1, 0)
    host = [eng.debug_fetch_plan_block(j) for j in range(n)]
    eng.evaluate_plans(pol, [_junk_plan()] * n, 1, 0)
    assert eng.debug_fetch_plan_block(n - 1)[640:].min() == 59
    eng.evaluate_plan_rewrites(pol, plans, maps, rewrites, 1, 0)
    for j in range(n):
        dev = eng.debug_fetch_plan_block(j)
        if dev.tobytes() != host[j].tobytes():
            bad = np.flatnonzero(dev != host[j])
            raise AssertionError(f"{what}: block {j} ({rewrites[j]}) differs at bytes {bad[:8].tolist()} ({len(bad)} in all)")


def _small_plans(rng):
    """four plans of 0..4 entries a year, the two lists counted apart (the windows' starts fall on every residue mod 8), actions 0..59
    so that 60 does not occur; a plan whose years 2..4 hold runs of one action (a dropped run across a word); an empty plan; L1, L2
    of 110 entries, long with a short child"""
    few = lambda c: [[int(a) for a in rng.integers(0, 60, k)] for k in c]
    out = [Plan(few(rng.integers(0, 5, 26)), few(rng.integers(0, 5, 26)), f"R{k}") for k in range(4)]
    runs = [[7, 8], [9], [12] * 11, [12, 12, 30], [12] * 5 + [31]] + [[int(a)] for a in rng.integers(0, 60, 21)]
    out.append(Plan(runs, [list(l) for l in runs], "runs"))
    out.append(Plan([[] for _ in range(26)], [[] for _ in range(26)], "empty"))
    early = lambda a, b: [a] * 10 + [0] * 3 + [b] * 10 + [0] * 3
    out += [_counted(rng, early(1, 10), early(2, 2), "L1"), _counted(rng, early(10, 1), early(2, 2), "L2")]
    assert [len(p) for p in out[-2:]] == [110, 110]
    return out


def _small_maps(plans):
    """identity, drop-all, drop one action that occurs (R0's first), drop one that does not (60), a substitution, cost_tier(0), every
    second action index dropped, and the action of the `runs` plan's runs dropped"""
    occurs = next(a for l in plans[0].best_actions for a in l)
    return [ActionMap.identity(), ActionMap.drop_all(), ActionMap.drop([occurs]), ActionMap.drop([60]), ActionMap.substitute({occurs: 36, 12: 0, 59: 58}),
            ActionMap.cost_tier(0), ActionMap.drop(range(1, 61, 2)), ActionMap.drop([12])]


def _small_rewrites(plans, maps):
    """[PlanRewrite] over _small_plans (indices 0..3 R, 4 runs, 5 empty, 6 L1, 7 L2) and the two policy plans behind them (8 short, 9 long)"""
    out = [PlanRewrite(0, 0, 0, 26, 3), PlanRewrite(0, 1, 3, 3, 3), PlanRewrite(1, 6, 0, 26, 0), PlanRewrite(4, 7, 0, 26, 3), PlanRewrite(4, 7, 2, 5, 1), PlanRewrite(4, 7, 3, 4, 2)]
    for p in range(4):
        for m in range(len(maps)):
            out += [PlanRewrite(p, m, f, t, 1 + (f + m) % 3) for f in range(26) for t in (f + 1, min(f + 6, 26), 26) if (f + p + m + t) % 10 == 0]
    out += [PlanRewrite(5, 1, 0, 26, 3), PlanRewrite(5, 6, 4, 9, 1), PlanRewrite(6, 1, 3, 26, 1), PlanRewrite(7, 6, 0, 26, 3), PlanRewrite(6, 5, 0, 13, 2)]
    s, l = len(plans) - 2, len(plans) - 1
    out += [PlanRewrite(s, 6, 0, 26, 3), PlanRewrite(s, 5, 10, 26, 1), PlanRewrite(s, 1, 12, 13, 2), PlanRewrite(l, 1, 4, 26, 1), PlanRewrite(l, 6, 0, 26, 3),
            PlanRewrite(l, 5, 0, 3, 3), PlanRewrite(l, 0, 0, 0, 0), PlanRewrite(l, 4, 1, 2, 1)]
    return out


def _random_rewrites(plans, maps, rng, n):
    out = []
    for _ in range(n):
        t = int(rng.integers(0, 27))
        out.append(PlanRewrite(int(rng.integers(0, len(plans))), int(rng.integers(0, len(maps))), int(rng.integers(0, t + 1)), t, int(rng.integers(0, 4))))
    return out


SMALL_LABELS = {"dropped run across a word boundary", "window wholly dropped", "nothing dropped but values changed", "a dropping map that drops nothing it meets",
                "some dropped", "from = 0", "to = 26", "whole plan", "empty window", "lists 0", "lists 1", "lists 2", "lists 3", "empty year at a window edge",
                "empty plan", "map index above 0", "plan index above 0"}


def small_inputs(short, long_, rng):
    """(plans, maps, rewrites) of the small-plans test, the coverage of its labels asserted; short, long_: the two policies' plans"""
    plans = _small_plans(rng) + [short, long_]
    assert len(short) == 28 and len(long_) >= 200
    maps = _small_maps(plans)
    rewrites = _small_rewrites(plans, maps)
    for which in (0, 1):
        covered = set().union(*[_labels(plans, maps, rw, which) for rw in rewrites])
        assert covered >= SMALL_LABELS, (which, SMALL_LABELS - covered)
        cover = _residue_cover(covered)
        assert all(len(cover[r]) >= 3 for r in range(8)), (which, cover)
    assert "long parent, short child" in set().union(*[_labels(plans, maps, rw, 0) for rw in rewrites])
    return plans, maps, rewrites


def _wide_plan(rng):
    """one year of 700 entries in both lists (two steps of the wave and more), runs of one action in it that straddle its 512-byte steps"""
    def lists(year):
        l = [[int(a) for a in rng.integers(0, 60, 3)] for _ in range(26)]
        wide = [int(a) for a in rng.integers(0, 60, 700)]
        for at in (180, 500, 690):
            wide[at:at + 30] = [60] * len(wide[at:at + 30])
        l[year] = wide
        return l
    return Plan(lists(4), lists(9), "wide")


def full_inputs(short, rng):
    """(plans, maps, rewrites) of the full-plans test, the coverage of its labels asserted"""
    f1, f2 = _full_plan(rng, 3, 13, 25, 1), _full_plan(rng, 20, 10, 18, 22)
    plans = [f1, f2, _wide_plan(rng), short]
    maps = [ActionMap.identity(), ActionMap.drop_all(), ActionMap.drop(range(0, 30)), ActionMap.cost_tier(1), ActionMap.drop([60]), ActionMap.drop(range(1, 61, 2)),
            ActionMap.substitute({a: (a + 7) % 61 for a in range(61)})]
    rewrites = [PlanRewrite(0, 1, 0, 26, 3), PlanRewrite(1, 1, 0, 26, 1), PlanRewrite(0, 3, 0, 26, 3), PlanRewrite(1, 6, 0, 26, 3), PlanRewrite(0, 2, 0, 26, 3),
                PlanRewrite(1, 2, 2, 24, 3), PlanRewrite(0, 5, 3, 4, 3), PlanRewrite(1, 1, 4, 19, 2), PlanRewrite(0, 1, 13, 14, 3), PlanRewrite(1, 2, 20, 21, 1),
                PlanRewrite(2, 4, 0, 26, 3), PlanRewrite(2, 4, 4, 5, 1), PlanRewrite(2, 4, 9, 10, 2), PlanRewrite(2, 1, 4, 10, 3), PlanRewrite(2, 5, 3, 26, 3),
                PlanRewrite(2, 3, 0, 26, 3), PlanRewrite(0, 0, 0, 0, 0), PlanRewrite(3, 5, 0, 26, 3), PlanRewrite(1, 5, 25, 26, 3), PlanRewrite(0, 2, 0, 1, 3), PlanRewrite(1, 2, 22, 24, 2)]
    want = {"dropped run across a 512-byte step boundary", "child much shorter than its parent", "child of 0 entries from a full plan",
            "full plan, values changed, nothing dropped", "window year of more than 512 entries", "window year of more than 64 entries", "empty year at a window edge",
            "dropped run across a word boundary", "to = 26", "from = 0", "whole plan"}
    for which in (0, 1):
        covered = set().union(*[_labels(plans, maps, rw, which) for rw in rewrites])
        assert covered >= want, (which, want - covered)
    return plans, maps, rewrites


# ---------------------------------------------------------------- the blocks
def test_blocks_are_write_lists_byte_for_byte_on_small_and_policy_plans(world, engine):
    rng = np.random.default_rng(23)
    pol = _seeded(engine)
    plans, maps, rewrites = small_inputs(Plan.from_policy(pol), Plan.from_policy(_long_policy()), rng)
    # batches of 1, 5 and 301 variants: the last workgroup holds one wave
    _check_blocks(engine, pol, plans, maps, rewrites[3:4], "1 variant")
    _check_blocks(engine, pol, plans, maps, rewrites[-5:], "5 variants")
    batch = (rewrites + _random_rewrites(plans, maps, rng, 301))[:301]
    assert len(batch) == 301 and len(rewrites) < 301
    _check_blocks(engine, pol, plans, maps, batch, "301 variants")


def test_blocks_of_full_plans_and_years_longer_than_a_step_of_the_wave(world, engine):
    rng = np.random.default_rng(3)
    plans, maps, rewrites = full_inputs(Plan.from_policy(_seeded(engine)), rng)
    _check_blocks(engine, ActionWeights(), plans, maps, rewrites, "full plans")


# ---------------------------------------------------------------- the records
def _record_inputs(engine, rng):
    pol = _seeded(engine)
    small = _small_plans(rng)
    plans = [Plan.from_policy(pol), Plan.from_policy(_long_policy())] + small[-2:]      # short, long, L1, L2
    maps = [ActionMap.identity(), ActionMap.drop_all(), ActionMap.cost_tier(0), ActionMap.drop_technology(4), ActionMap.replace_technology(0, 12),
            ActionMap.drop(range(1, 61, 2)), ActionMap.substitute({a: 36 for a in range(21, 27)})]
    rewrites = [PlanRewrite(0, 0, 0, 0, 0), PlanRewrite(1, 0, 0, 26, 3), PlanRewrite(0, 1, 10, 26, 1), PlanRewrite(1, 1, 5, 26, 1), PlanRewrite(0, 2), PlanRewrite(1, 2),
                PlanRewrite(0, 3), PlanRewrite(1, 3), PlanRewrite(0, 4, 0, 26, 3), PlanRewrite(1, 4, 0, 26, 3), PlanRewrite(0, 5, 0, 13, 1), PlanRewrite(1, 5, 13, 26, 1),
                PlanRewrite(0, 6, 0, 26, 2), PlanRewrite(1, 6, 0, 26, 2), PlanRewrite(2, 1, 13, 26, 1), PlanRewrite(3, 1, 0, 13, 1), PlanRewrite(2, 5), PlanRewrite(3, 2, 0, 26, 3),
                PlanRewrite(1, 1, 0, 26, 1), PlanRewrite(0, 1, 7, 7, 3)]
    return pol, plans, maps, rewrites


@pytest.mark.parametrize("helper", ["0", "all"])
def test_rewrites_are_the_host_built_children(world, engine, helper):
    rng = np.random.default_rng(17)
    pol, plans, maps, rewrites = _record_inputs(engine, rng)
    assert "long parent, short child" in set().union(*[_labels(plans, maps, rw, 0) for rw in rewrites])
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        for n in (1, 5, 40):
            batch = (rewrites + _random_rewrites(plans, maps, rng, max(n - len(rewrites), 0)))[:n]
            children = [apply_rewrite(plans, maps, rw) for rw in batch]
            want = eng.evaluate_plans(pol, children, 77, 3000)
            got = eng.evaluate_plan_rewrites(pol, plans, maps, batch, 77, 3000, same_index=False)
            _same_records(got, want, (helper, n, "index + j"))
            got = eng.evaluate_plan_rewrites(pol, plans, maps, batch, 77, 3000, same_index=True)
            for j, p in enumerate(children):
                one = eng.evaluate_plans(pol, [p], 77, 3000)
                _same_records(got, one, (helper, n, "same index", j, batch[j]), [j], [0])
        assert len({want.metrics[j].tobytes() for j in range(len(batch))}) >= 4      # (the rewrites matter)
    finally:
        eng.close()


def test_deficit_lists_that_run_out_draw_the_same_fallbacks(world, engine):
    """dropped deficit-list entries make a year's list run out, and seeded fallbacks are drawn: a rewritten variant draws what the
    host-built child draws"""
    pol = _seeded(engine)
    plans = [Plan.from_policy(pol), Plan.from_policy(_long_policy())]
    maps = [ActionMap.drop_all(), ActionMap.drop(range(0, 61, 2)), ActionMap.drop(range(30, 61))]
    rewrites = [PlanRewrite(p, m, f, t, l) for p in (0, 1) for m in range(3) for f, t, l in ((0, 26, 2), (0, 26, 3), (5, 20, 2), (13, 14, 3))]
    children = [apply_rewrite(plans, maps, rw) for rw in rewrites]
    assert any(sum(len(l) for l in c.best_deficit_actions) < sum(len(l) for l in plans[rw.plan].best_deficit_actions) for c, rw in zip(children, rewrites))
    for pol2 in (pol, ActionWeights()):
        want = engine.evaluate_plans(pol2, children, 41, 700)
        assert (want.n_draws > 0).any()
        got = engine.evaluate_plan_rewrites(pol2, plans, maps, rewrites, 41, 700, same_index=False)
        _same_records(got, want, "dropped, index + j")
        got = engine.evaluate_plan_rewrites(pol2, plans, maps, rewrites, 41, 700 + 3, same_index=True)
        _same_records(got, want, "dropped, same index", [3], [3])


def test_every_variant_is_the_oracles_replay_of_the_child(world, engine):
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    pol = _seeded(engine)
    plans = [Plan.from_policy(pol), Plan.from_policy(_long_policy())]
    maps = [ActionMap.identity(), ActionMap.drop_all(), ActionMap.cost_tier(0), ActionMap.replace_technology(1, 0), ActionMap.drop(range(1, 61, 2))] + \
           [ActionMap.drop_technology(t) for t in (0, 4, 12)]
    rewrites = [PlanRewrite(0, 0, 0, 0, 0), PlanRewrite(1, 0, 0, 26, 3)] + [PlanRewrite(p, m, 0, 26, 1) for p in (0, 1) for m in (2, 3, 4, 5, 6, 7)] + \
               [PlanRewrite(p, 1, f, 26, 1) for p in (0, 1) for f in (3, 15)] + [PlanRewrite(1, 4, 6, 20, 3), PlanRewrite(0, 2, 0, 26, 2)]
    assert len(rewrites) == 20
    seed, first = 1234, 90_000
    eng = _engine(world, EIRGRID_HELPER_WAVES="0")
    try:
        for same in (True, False):
            got = eng.evaluate_plan_rewrites(pol, plans, maps, rewrites, seed, first, same_index=same)
            small = engine.evaluate_plan_rewrites(pol, plans, maps, rewrites, seed, first, same_index=same)      # (the small-batch kernel)
            for j, rw in enumerate(rewrites if same else rewrites[:8]):
                st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, apply_rewrite(plans, maps, rw)), seed + first + (0 if same else j), replay=True)
                assert st == 0, (j, rw)
                assert_episode_equal(got, j, ref, f"same_index {same}, rewrite {j} {rw}")
                assert_episode_equal(small, j, ref, f"(small-batch kernel) same_index {same}, rewrite {j} {rw}")
    finally:
        eng.close()


# ---------------------------------------------------------------- technology_report
def test_technology_report_is_a_host_loop_over_the_children(world):
    eng = _engine(world)
    try:
        pol = ActionWeights()
        res = eng.rollout_batch(pol, 4711, 4)
        plans = [Plan.from_result(res, e, f"sampled {e}") for e in range(4)]
        # the context's own archive, started before the call and holding a training batch's front
        eng.track_pareto(16)
        eng.rollout_batch(pol, 5, 48)
        before = eng.fetch_pareto()
        assert len(before[1]) >= 1
        seed, index = 91, 7
        for kw in ({}, {"deficit": "keep", "cost_only": True}, {"substitute_with": 0}):
            deficit, sub = kw.get("deficit", "substitute"), kw.get("substitute_with", 36)
            # the children, by the restatement: t out of best_actions, and t in best_deficit_actions built as `sub`
            want = []
            for p, plan in enumerate(plans):
                want.append((p, -1, 0, plan))
                used = [a for l in plan.best_actions for a in l]
                for t in sorted({a // 3 for a in used if a < 45}):
                    child = apply_rewrite([plan], [ActionMap.drop_technology(t)], PlanRewrite(0, 0, 0, 26, 1))
                    if deficit == "substitute":
                        child = apply_rewrite([child], [ActionMap.substitute({3 * t + k: sub for k in range(3)})], PlanRewrite(0, 0, 0, 26, 2))
                        assert all(a // 3 != t or a == sub for l in child.best_deficit_actions for a in l)
                    want.append((p, t, sum(1 for a in used if a // 3 == t), child))
            if deficit == "substitute":      # (the case where the substituted plan rides as a parent of its own is reached)
                assert len(technology_rewrites(plans, deficit, sub)[0]) > len(plans)
            assert len(want) > 24
            rows = [eng.evaluate_plans(pol, [c], seed, index) for _, _, _, c in want]      # (every variant at global index 7)
            report = eng.technology_report(pol, plans, seed, index, max_variants=7, **kw)
            assert N.lib().eg_last_batch_size(eng.h) == (len(want) - 1) % 7 + 1      # (chunks of 7: the last one stays behind)
            assert [(r.plan, r.type, r.removed) for r in report] == [w[:3] for w in want]
            own = 0.0
            for r, one in zip(report, rows):
                assert np.array(r.metrics).tobytes() == one.metrics[0].tobytes() and r.status == one.status[0], (r.plan, r.type)
                score = rank_score(one.metrics[0], bool(kw.get("cost_only")))
                own = score if r.type < 0 else own
                assert r.score == score and r.delta == score - own
            assert len({np.array(r.metrics).tobytes() for r in report}) > 8
            assert eng.technology_report(pol, plans, seed, index, **kw) == report      # one chunk
        after = eng.fetch_pareto()
        assert after[1].tolist() == before[1].tolist() and after[2].tobytes() == before[2].tobytes() and after[3] == before[3]
        assert after[0].metrics.tobytes() == before[0].metrics.tobytes()
    finally:
        eng.close()


# ---------------------------------------------------------------- refusals on the device side
def test_an_invalid_rewrite_is_refused_and_the_last_batch_stays(world, engine):
    import ctypes as C
    pol = _seeded(engine)
    short = Plan.from_policy(pol)
    prev = engine.evaluate_plans(pol, [short, short], 9, 40)
    to = list(range(61)); to[17] = 200
    bad = N.EgActionMap((C.c_uint8 * 61)(*to))
    with pytest.raises(EirgridError, match=r"map 1: to\[17\] = 200 \(0..60 or 0xFF drop\)"):
        engine.evaluate_plan_rewrites(pol, [short, short], [ActionMap.identity(), bad], [PlanRewrite()], 1)
    with pytest.raises(EirgridError, match="rewrite 2: plan 2 >= n_plans 2"):
        engine.evaluate_plan_rewrites(pol, [short, short], [ActionMap.drop_all()], [PlanRewrite(), PlanRewrite(1, 0, 3, 9), PlanRewrite(2, 0, 3, 9)], 1)
    assert N.lib().eg_last_batch_size(engine.h) == 2
    _same_records(engine.fetch(), prev, "the batch before the refusals")


def test_a_rank_of_a_group_is_refused(world):
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        base = Plan([[3, 12]] + [[] for _ in range(25)], [[] for _ in range(26)])
        with pytest.raises(EirgridError, match="eg_evaluate_plan_rewrites: the context is a rank of an eg_group"):
            g.ranks[0].evaluate_plan_rewrites(ActionWeights(), [base, base], [ActionMap.identity()], [PlanRewrite()], 1)
    finally:
        g.close()
