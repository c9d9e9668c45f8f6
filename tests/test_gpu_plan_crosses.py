"""GPU: plan crosses (include/eirgrid_hip.h eg_evaluate_plan_crosses; csrc/eg_plan_crosses.h k_plan_crosses; eg_plans.cpp).  Variant j of a
plan-cross batch is parent a with the years [from_year, to_year) of both lists taken from parent b, evaluated exactly as eg_evaluate_plans
evaluates the host-built child: the plan blocks the device writes must equal, byte for byte, the blocks the host builds for the children,
the records must be those of the host-built children and the tabled oracle's, and Engine.cross_front must return the non-dominated
variants by eg_pareto_track's definitions without touching the context's archive."""
import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.engine import ActionWeights, HostTables, Plan, PlanCross, cross_pairs, rank_score
from oracle import api as O
from tests.helpers import assert_episode_equal
from tests.test_gpu_plan_edits import _junk_plan, _long_policy
from tests.test_gpu_plans import _engine, _oracle_plan, _same_records
from tests.test_gpu_replay_hoist import _seeded
from tests.test_plan_crosses import apply_cross, front_restated

pytestmark = pytest.mark.gpu

SHORT_MAX = 96      # kShortReplayMax (csrc/eg_internal.h): the best_actions length up to which a plan takes the short replay route


def _lists(plan, which):
    return (plan.best_actions, plan.best_deficit_actions)[which]


def _offsets(plan, which):
    return np.concatenate([[0], np.cumsum([len(l) for l in _lists(plan, which)])]).astype(int)


def _labels(parents, x, which):
    """what cross x exercises on list `which` of the kernel's word selection, by name"""
    A, B = parents[x.a], parents[x.b]
    oA, oB = _offsets(A, which), _offsets(B, which)
    cA, cB = [len(l) for l in _lists(A, which)], [len(l) for l in _lists(B, which)]
    f, t = x.from_year, x.to_year
    p0, m = int(oA[f]), int(oB[t] - oB[f])
    p1, tail = p0 + m, int(oA[26] - oA[t])
    child = p1 + tail
    out = set()
    if f == t:
        out.add("from == to")
    if x.a == x.b:
        out.add("a == b")
    if f == t or x.a == x.b:
        return out
    if m > 0:
        out.add(f"residue {p0 % 8} against {int(oB[f]) % 8}")
        if p1 % 8 == 0:
            out.add("middle ends on a word boundary")
    k = p0 % 8
    if m == 0 and k >= 1 and tail > 0:
        out.add("middle of 0 bytes inside a word")           # (the word holds head and tail)
    if m == 1 and 1 <= k <= 6 and tail > 0:
        out.add("middle of 1 byte inside a word")            # (the word holds all three segments)
    if m == 7 and k <= 1 and (k == 1 or tail > 0):
        out.add("middle of 7 bytes inside a word")
    if m >= 1 and k >= 1 and k + m < 8 and tail > 0:
        out.add("a word of three segments")
    if f == 0:
        out.add("from = 0")
    if t == 26:
        out.add("to = 26")
    if f == 0 and t == 26:
        out.add("whole plan")
    if 0 in (cA[f], cA[t - 1], cB[f], cB[t - 1]):
        out.add("empty year at the window's edge")
    if oA[26] == 0 or oB[26] == 0:
        out.add("empty parent")
    if max(cA[:f] + cB[f:t] + cA[t:]) > 64:
        out.add("year of more than 64 entries")
    if oA[26] == 4096 and oB[26] == 4096 and child == 4096:
        out.add("child of 4 096 entries from two full plans")
    if child <= oA[26] - 512:
        out.add("child much shorter than parent a")
    if which == 0:
        if oA[26] <= SHORT_MAX and oB[26] <= SHORT_MAX and child > SHORT_MAX:
            out.add("short parents, long child")
        if oA[26] > SHORT_MAX and oB[26] > SHORT_MAX and child <= SHORT_MAX:
            out.add("long parents, short child")
    return out


def _residue_cover(labels):
    """{residue of oA[from]: the residues of oB[from] it met}"""
    cover = {r: set() for r in range(8)}
    for l in labels:
        if l.startswith("residue "):
            cover[int(l.split()[1])].add(int(l.split()[3]))
    return cover


def _valid(parents, x):
    return all(len([a for l in _lists(apply_cross(parents, x), w) for a in l]) <= 4096 for w in (0, 1))


def _check_blocks(eng, pol, parents, crosses, what):
    """The plan blocks k_plan_crosses writes against the blocks the host's write_lists builds for the children, all 8 832 bytes of each
    (eg_debug_fetch_plan_block) — with the pool overwritten in between, so that nothing is left over from the host's blocks."""
    n = len(crosses)
    children = [apply_cross(parents, x) for x in crosses]
    assert all(x.apply(parents) == c for x, c in zip(crosses, children))
    eng.evaluate_plans(pol, children, 1, 0)
    host = [eng.debug_fetch_plan_block(j) for j in range(n)]
    eng.evaluate_plans(pol, [_junk_plan()] * n, 1, 0)
    assert eng.debug_fetch_plan_block(n - 1)[640:].min() == 59
    eng.evaluate_plan_crosses(pol, parents, crosses, 1, 0)
    for j in range(n):
        dev = eng.debug_fetch_plan_block(j)
        if dev.tobytes() != host[j].tobytes():
            bad = np.flatnonzero(dev != host[j])
            raise AssertionError(f"{what}: block {j} ({crosses[j]}) differs at bytes {bad[:8].tolist()} ({len(bad)} in all)")


def _counted(rng, counts, dcounts, name=""):
    return Plan([[int(a) for a in rng.integers(0, 61, c)] for c in counts], [[int(a) for a in rng.integers(0, 61, c)] for c in dcounts], name)


def _small_parents(rng):
    """crafted plans: G and H place middle segments of 0, 1 and 7 bytes inside a word on both lists (G's offsets 0, 3, 5, 9, 9, 12, ...);
    four plans of 0..4 entries a year, the two lists counted apart, give every alignment of the two parents' offsets; an empty plan;
    S1, S2 short with a long child, L1, L2 long with a short one"""
    g = [3, 2, 4, 0, 3] + [1] * 21
    h = [2, 1, 0, 7, 2] + [2] * 21
    out = [_counted(rng, g, g, "G"), _counted(rng, h, h, "H")]
    out += [_counted(rng, rng.integers(0, 5, 26), rng.integers(0, 5, 26), f"R{k}") for k in range(4)]
    out.append(Plan([[] for _ in range(26)], [[] for _ in range(26)], "empty"))
    early = lambda a, b: [a] * 10 + [0] * 3 + [b] * 10 + [0] * 3      # a a year in ten of the years 0..12, b a year in ten of 13..25
    out += [_counted(rng, early(8, 1), early(1, 2), "S1"), _counted(rng, early(1, 8), early(2, 1), "S2"),
            _counted(rng, early(1, 10), early(2, 2), "L1"), _counted(rng, early(10, 1), early(2, 2), "L2")]
    assert [len(p) for p in out[-4:]] == [90, 90, 110, 110]
    return out


def _small_crosses(parents):
    """[PlanCross] over _small_parents (indices 0 G, 1 H, 2..5 R, 6 empty, 7 S1, 8 S2, 9 L1, 10 L2)"""
    out = [PlanCross(0, 1, 1, 2), PlanCross(0, 1, 2, 3), PlanCross(0, 1, 3, 4), PlanCross(0, 1, 0, 26), PlanCross(1, 0, 3, 4), PlanCross(0, 1, 7, 7), PlanCross(1, 1, 2, 9)]
    for a in range(2, 6):
        for b in range(2, 6):
            if a != b:
                out += [PlanCross(a, b, f, t) for f in range(26) for t in (f + 1, 26) if (f + a + b) % 3 == 0]
    out += [PlanCross(2, 6, 4, 9), PlanCross(6, 2, 0, 13), PlanCross(6, 3, 25, 26), PlanCross(3, 6, 0, 26)]
    out += [PlanCross(7, 8, 13, 26), PlanCross(8, 7, 13, 26), PlanCross(9, 10, 13, 26), PlanCross(10, 9, 13, 26), PlanCross(7, 10, 0, 5)]
    return out


def _random_crosses(parents, rng, n):
    out = []
    while len(out) < n:
        t = int(rng.integers(0, 27))
        x = PlanCross(int(rng.integers(0, len(parents))), int(rng.integers(0, len(parents))), int(rng.integers(0, t + 1)), t)
        if _valid(parents, x):
            out.append(x)
    return out


def _full_plan(rng, run_long, run_empty, dfc_long, dfc_empty):
    """both lists at the 4 096-entry capacity: 150 entries a year, one year empty, the rest in one year"""
    def lists(extra_year, empty_year):
        l = [[int(a) for a in rng.integers(0, 61, 150)] for _ in range(26)]
        l[empty_year] = []
        l[extra_year] += [int(a) for a in rng.integers(0, 61, 4096 - 25 * 150)]
        return l
    plan = Plan(lists(run_long, run_empty), lists(dfc_long, dfc_empty))
    assert len(plan) == 4096 and sum(len(l) for l in plan.best_deficit_actions) == 4096
    return plan


SMALL_LABELS = {"middle of 0 bytes inside a word", "middle of 1 byte inside a word", "middle of 7 bytes inside a word", "a word of three segments",
                "middle ends on a word boundary", "from = 0", "to = 26", "whole plan", "from == to", "a == b", "empty year at the window's edge", "empty parent"}


# ---------------------------------------------------------------- the blocks
def test_blocks_are_write_lists_byte_for_byte_on_small_and_policy_parents(world, engine):
    rng = np.random.default_rng(23)
    pol = _seeded(engine)
    parents = _small_parents(rng) + [Plan.from_policy(pol), Plan.from_policy(_long_policy())]
    assert len(parents[-2]) == 28 and len(parents[-1]) >= 200
    s, l = len(parents) - 2, len(parents) - 1
    crosses = _small_crosses(parents) + [PlanCross(s, l, 10, 26), PlanCross(l, s, 10, 26), PlanCross(s, l, 12, 13), PlanCross(l, s, 0, 3), PlanCross(l, 6, 5, 26),
                                         PlanCross(s, s, 0, 0), PlanCross(l, l, 0, 0), PlanCross(l, 0, 1, 2)]
    assert all(_valid(parents, x) for x in crosses)
    for which in (0, 1):
        covered = set().union(*[_labels(parents, x, which) for x in crosses])
        assert covered >= SMALL_LABELS, (which, SMALL_LABELS - covered)
        cover = _residue_cover(covered)
        assert all(len(cover[r]) >= 3 for r in range(8)), (which, cover)
    routes = set().union(*[_labels(parents, x, 0) for x in crosses])
    assert {"short parents, long child", "long parents, short child"} <= routes
    # batches of 1, 5 and 301 variants: the last workgroup holds one wave
    _check_blocks(engine, pol, parents, crosses[:1], "1 variant")
    _check_blocks(engine, pol, parents, crosses[-5:], "5 variants")
    batch = (crosses + _random_crosses(parents, rng, 301))[:301]
    assert len(batch) == 301 and len(crosses) < 301
    _check_blocks(engine, pol, parents, batch, "301 variants")


def test_blocks_of_full_plans_and_years_longer_than_a_wave(world, engine):
    rng = np.random.default_rng(3)
    pol = ActionWeights()
    f1, f2 = _full_plan(rng, 3, 13, 25, 1), _full_plan(rng, 20, 10, 18, 22)
    short = Plan.from_policy(_seeded(engine))
    empty = Plan([[] for _ in range(26)], [[] for _ in range(26)])
    parents = [f1, f2, short, empty]
    # years 4..7 hold 150 entries in both lists of both plans: the windows are equally long and the child holds 4 096 entries again
    crosses = [PlanCross(0, 1, 4, 8), PlanCross(1, 0, 4, 8), PlanCross(0, 1, 3, 4), PlanCross(1, 0, 13, 14), PlanCross(0, 1, 25, 26), PlanCross(1, 0, 0, 1),
               PlanCross(0, 2, 2, 26), PlanCross(0, 3, 0, 26), PlanCross(2, 0, 3, 4), PlanCross(3, 1, 20, 21), PlanCross(0, 0, 0, 0), PlanCross(1, 0, 9, 9)]
    assert all(_valid(parents, x) for x in crosses)
    for which in (0, 1):
        child = apply_cross(parents, crosses[0])
        assert sum(len(l) for l in _lists(child, which)) == 4096 and child != f1 and child != f2
        covered = set().union(*[_labels(parents, x, which) for x in crosses])
        want = {"child of 4 096 entries from two full plans", "year of more than 64 entries", "child much shorter than parent a", "empty year at the window's edge",
                "empty parent", "to = 26", "from = 0", "whole plan"}
        assert covered >= want, (which, want - covered)
    _check_blocks(engine, pol, parents, crosses, "full plans")


# ---------------------------------------------------------------- the records
def _record_parents(engine, rng):
    pol = _seeded(engine)
    small = _small_parents(rng)
    parents = [Plan.from_policy(pol), Plan.from_policy(_long_policy())] + small[-4:]      # short, long, S1, S2, L1, L2
    crosses = [PlanCross(0, 0, 0, 0), PlanCross(1, 1, 0, 0), PlanCross(0, 1, 10, 26), PlanCross(1, 0, 10, 26), PlanCross(0, 1, 5, 6), PlanCross(1, 0, 5, 6),
               PlanCross(0, 1, 0, 4), PlanCross(1, 0, 20, 26), PlanCross(0, 1, 24, 26), PlanCross(1, 0, 1, 26), PlanCross(2, 3, 13, 26), PlanCross(3, 2, 13, 26),
               PlanCross(4, 5, 13, 26), PlanCross(5, 4, 13, 26), PlanCross(0, 4, 13, 26), PlanCross(1, 2, 0, 13), PlanCross(0, 1, 0, 26), PlanCross(0, 1, 7, 7)]
    return pol, parents, crosses


@pytest.mark.parametrize("helper", ["0", "all"])
def test_crosses_are_the_host_built_children(world, engine, helper):
    rng = np.random.default_rng(17)
    pol, parents, crosses = _record_parents(engine, rng)
    routes = set().union(*[_labels(parents, x, 0) for x in crosses])
    assert {"short parents, long child", "long parents, short child"} <= routes
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        for n in (1, 5, 40):
            batch = (crosses + _random_crosses(parents, rng, max(n - len(crosses), 0)))[:n]
            children = [apply_cross(parents, x) for x in batch]
            want = eng.evaluate_plans(pol, children, 77, 3000)
            got = eng.evaluate_plan_crosses(pol, parents, batch, 77, 3000, same_index=False)
            _same_records(got, want, (helper, n, "index + j"))
            got = eng.evaluate_plan_crosses(pol, parents, batch, 77, 3000, same_index=True)
            for j, p in enumerate(children):
                one = eng.evaluate_plans(pol, [p], 77, 3000)
                _same_records(got, one, (helper, n, "same index", j, batch[j]), [j], [0])
        assert len({want.metrics[j].tobytes() for j in range(len(batch))}) > 3      # (the crosses matter)
    finally:
        eng.close()


def test_lists_that_run_out_draw_the_same_fallbacks(world, engine):
    """parents cut short draw seeded fallbacks when a year's list runs out: a crossed variant draws what the host-built child draws"""
    pol = _seeded(engine)
    short, long_ = Plan.from_policy(pol), Plan.from_policy(_long_policy())
    cut = lambda p, keep: Plan([l[:len(l) // 2] if keep(y) else [] for y, l in enumerate(p.best_actions)], [l[:1] for l in p.best_deficit_actions])
    parents = [cut(short, lambda y: True), cut(long_, lambda y: y % 3 != 1)]
    crosses = cross_pairs(2, cuts=range(2, 26, 3)) + [PlanCross(0, 1, 4, 6), PlanCross(1, 0, 4, 6), PlanCross(0, 1, 13, 14), PlanCross(1, 0, 0, 2)]
    children = [apply_cross(parents, x) for x in crosses]
    for pol2 in (pol, ActionWeights()):
        want = engine.evaluate_plans(pol2, children, 41, 700)
        assert (want.n_draws > 0).any()
        got = engine.evaluate_plan_crosses(pol2, parents, crosses, 41, 700, same_index=False)
        _same_records(got, want, "cut, index + j")
        got = engine.evaluate_plan_crosses(pol2, parents, crosses, 41, 700 + 3, same_index=True)
        _same_records(got, want, "cut, same index", [3], [3])


def test_every_variant_is_the_oracles_replay_of_the_child(world, engine):
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    pol = _seeded(engine)
    parents = [Plan.from_policy(pol), Plan.from_policy(_long_policy())]
    crosses = [PlanCross(0, 0, 0, 0), PlanCross(1, 1, 0, 0)] + [PlanCross(a, 1 - a, c, 26) for a in (0, 1) for c in (1, 6, 11, 17, 22, 25)] + \
              [PlanCross(a, 1 - a, f, t) for a in (0, 1) for f, t in ((0, 1), (5, 6), (9, 14), (0, 26), (25, 26))]
    assert len(crosses) == 24
    seed, first = 1234, 90_000
    eng = _engine(world, EIRGRID_HELPER_WAVES="0")
    try:
        for same in (True, False):
            got = eng.evaluate_plan_crosses(pol, parents, crosses, seed, first, same_index=same)
            small = engine.evaluate_plan_crosses(pol, parents, crosses, seed, first, same_index=same)      # (the small-batch kernel)
            for j, x in enumerate(crosses if same else crosses[:8]):
                st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, apply_cross(parents, x)), seed + first + (0 if same else j), replay=True)
                assert st == 0, (j, x)
                assert_episode_equal(got, j, ref, f"same_index {same}, cross {j} {x}")
                assert_episode_equal(small, j, ref, f"(small-batch kernel) same_index {same}, cross {j} {x}")
    finally:
        eng.close()


# ---------------------------------------------------------------- cross_front
def test_cross_front_is_the_filter_over_the_host_built_children(world):
    eng = _engine(world)
    try:
        pol = ActionWeights()
        res = eng.rollout_batch(pol, 4711, 4)
        parents = [Plan.from_result(res, e, f"sampled {e}") for e in range(4)]
        # the context's own archive, started before the call and holding a training batch's front
        eng.track_pareto(16)
        eng.rollout_batch(pol, 5, 48)
        before = eng.fetch_pareto()
        assert len(before[1]) >= 1
        seed, index = 91, 7
        crosses = cross_pairs(4)
        assert len(crosses) == 4 + 4 * 3 * 25
        rows = [eng.evaluate_plans(pol, [apply_cross(parents, x)], seed, index) for x in crosses]      # (every variant at global index 7)
        metrics = np.array([r.metrics[0] for r in rows]); status = np.array([r.status[0] for r in rows])
        assert (status == 0).sum() > 100 and len({m.tobytes() for m in metrics}) > 20
        for kw, mask in (({}, 15), ({"objectives": ("emissions", "cost"), "cost_only": True}, 5)):
            front = eng.cross_front(pol, parents, seed, index, max_variants=100, **kw)
            want = front_restated(metrics, status, mask)
            assert front.variant.tolist() == want and len(want) >= 1
            assert front.crosses == [crosses[j] for j in want]
            assert front.metrics.tobytes() == metrics[want].tobytes()
            assert front.score.tobytes() == np.array([rank_score(metrics[j], bool(kw.get("cost_only"))) for j in want]).tobytes()
            assert front.is_parent.tolist() == [j < 4 for j in want]
            assert front.n_variants == len(crosses) and front.n_valid == int(((status == 0) & ~np.isnan(metrics).any(axis=1)).sum())
            assert N.lib().eg_last_batch_size(eng.h) == len(crosses) - 300      # (the last of the four chunks stays behind)
        assert eng.cross_front(pol, parents, seed, index).variant.tolist() == front_restated(metrics, status, 15)      # one chunk
        after = eng.fetch_pareto()
        assert after[1].tolist() == before[1].tolist() and after[2].tobytes() == before[2].tobytes() and after[3] == before[3]
        assert after[0].metrics.tobytes() == before[0].metrics.tobytes()
    finally:
        eng.close()


# ---------------------------------------------------------------- refusals on the device side
def test_an_invalid_cross_is_refused_and_the_last_batch_stays(world, engine):
    rng = np.random.default_rng(5)
    pol = _seeded(engine)
    short = Plan.from_policy(pol)
    f1, f2 = _full_plan(rng, 3, 13, 25, 1), _full_plan(rng, 20, 10, 18, 22)
    prev = engine.evaluate_plans(pol, [short, short], 9, 40)
    # f1's empty year 13 takes f2's 150 entries: 4 246
    with pytest.raises(EirgridError, match=r"cross 1: best_actions would hold 4246 entries \(at most 4096\)"):
        engine.evaluate_plan_crosses(ActionWeights(), [f1, f2], [PlanCross(0, 1, 4, 8), PlanCross(0, 1, 13, 14)], 1)
    with pytest.raises(EirgridError, match="cross 2: a 2 >= n_plans 2"):
        engine.evaluate_plan_crosses(pol, [short, short], [PlanCross(), PlanCross(1, 0, 3, 9), PlanCross(2, 0, 3, 9)], 1)
    assert N.lib().eg_last_batch_size(engine.h) == 2
    _same_records(engine.fetch(), prev, "the batch before the refusals")


def test_a_rank_of_a_group_is_refused(world):
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        base = Plan([[3, 12]] + [[] for _ in range(25)], [[] for _ in range(26)])
        with pytest.raises(EirgridError, match="eg_evaluate_plan_crosses: the context is a rank of an eg_group"):
            g.ranks[0].evaluate_plan_crosses(ActionWeights(), [base, base], [PlanCross()], 1)
    finally:
        g.close()
