"""GPU: plan moves (include/eirgrid_hip.h eg_evaluate_plan_moves; csrc/eg_plan_moves.h k_plan_moves; eg_plans.cpp).  Variant j of a
plan-move batch is the base plan with move j applied — one entry taken out of its year and put into another — evaluated exactly as
eg_evaluate_plans evaluates the moved plan: the plan blocks the device writes must equal, byte for byte, the blocks the host builds for the
moved plans, the records must be those of the host-built plans, and for the short base the tabled oracle's."""
import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.engine import ActionWeights, HostTables, Plan, PlanMove, rank_score, refine_moves
from oracle import api as O
from tests.helpers import assert_episode_equal
from tests.test_gpu_plan_edits import _junk_plan, _long_policy
from tests.test_gpu_plans import _engine, _oracle_plan, _same_records
from tests.test_gpu_replay_hoist import _seeded
from tests.test_plan_moves import apply_move, round_moves
from tests.test_refine import round_edits

pytestmark = pytest.mark.gpu

BOTH_LISTS = ("same word", "same word, back", "adjacent words", "adjacent words, back", "byte 7 to byte 0", "byte 0 to byte 7", "first to last", "last to first",
              "reorder", "identity", "bit clears", "bit stays")


def _lists(plan, which):
    return (plan.best_actions, plan.best_deficit_actions)[which]


def _flat_move(plan, which, S, D):
    """the move that takes flat entry S of a list to flat position D, counted after the removal"""
    count = [len(l) for l in _lists(plan, which)]
    off = np.concatenate([[0], np.cumsum(count)])
    y = int(np.searchsorted(off, S, side="right") - 1)
    count[y] -= 1
    off2 = np.concatenate([[0], np.cumsum(count)])
    ty = int(np.searchsorted(off2, D, side="right") - 1) if D < off2[26] else max(t for t in range(26) if count[t] or t == 0)
    m = PlanMove(which, y, int(S - off[y]), ty, int(D - off2[ty]))
    before = [a for l in _lists(plan, which) for a in l]
    after = [a for l in _lists(apply_move(plan, m), which) for a in l]
    rest = before[:S] + before[S + 1:]
    assert after == rest[:D] + [before[S]] + rest[D:], (which, S, D, m)
    return m


def _move_set(plan):
    """[(label, move)]: on each of the two lists the flat positions at which the kernel's word selection can go wrong, the whole list
    shifted both ways, reorders, the identity, what the masks see, and — where the plan has them — an empty target year and a year longer
    than a wave as source and as target"""
    out = []
    for which in (0, 1):
        lists = _lists(plan, which)
        other = _lists(plan, 1 - which)
        count = [len(l) for l in lists]
        total = sum(count)
        if total == 0:
            continue
        k = 8 if total >= 20 else 0      # (a list too short for a case goes without it: the callers check what their bases cover)
        for label, S, D in (("same word", k + 1, k + 5), ("same word, back", k + 5, k + 1), ("adjacent words", k + 2, k + 11), ("adjacent words, back", k + 11, k + 2),
                            ("byte 7 to byte 0", k + 7, k + 8), ("byte 0 to byte 7", k + 8, k + 7)):
            if max(S, D) < total:
                out.append((label, _flat_move(plan, which, S, D)))
        years = [y for y in range(26) if count[y]]
        first, last = years[0], years[-1]
        # (with entries in years 0 and 25: the first entry of year 0 behind the last of year 25 and back — every offset moves)
        out.append(("first to last", PlanMove(which, first, 0, 25, count[25] - (first == 25))))
        out.append(("last to first", PlanMove(which, last, count[last] - 1, 0, 0)))
        y3 = max(years, key=lambda y: count[y])
        out.append(("identity", PlanMove(which, last, count[last] - 1, last, count[last] - 1)))
        if count[y3] >= 2:
            out += [("reorder", PlanMove(which, y3, 0, y3, count[y3] - 1)), ("reorder", PlanMove(which, y3, count[y3] - 1, y3, 0)), ("identity", PlanMove(which, y3, 1, y3, 1))]
        if count[y3] >= 3:
            out.append(("reorder", PlanMove(which, y3, 1, y3, 2)))
        empty = [y for y in range(26) if not count[y]]
        if empty:
            out += [("empty target", PlanMove(which, first, 0, empty[0], 0)), ("empty target", PlanMove(which, last, count[last] - 1, empty[-1], 0))]
        wide = [y for y in range(26) if count[y] > 64]
        if wide:
            w = wide[-1]
            t = next(y for y in range(26) if y != w)
            out += [("long source", PlanMove(which, w, 66, t, count[t] // 2)), ("long source", PlanMove(which, w, count[w] - 1, t, 0)),
                    ("long target", PlanMove(which, t, 0, w, 65)), ("long target", PlanMove(which, t, count[t] - 1, w, count[w]))]
        # the masks: an entry whose action the year's two lists hold once / more than once (in this list or the other)
        seen = set()
        for y in years:
            for i, a in enumerate(lists[y]):
                kind = "once" if lists[y].count(a) + other[y].count(a) == 1 else ("twice in the list" if lists[y].count(a) > 1 else "in the other list too")
                t = y + 1 if y < 25 else y - 1
                if kind not in seen:
                    seen.add(kind); out.append(("bit clears" if kind == "once" else "bit stays", PlanMove(which, y, i, t, count[t])))
    return out


def _random_moves(plan, rng, n):
    out = []
    while len(out) < n:
        which = int(rng.integers(0, 2))
        lists = _lists(plan, which)
        y = int(rng.integers(0, 26)); ty = int(rng.integers(0, 26))
        if lists[y]:
            out.append(PlanMove(which, y, int(rng.integers(0, len(lists[y]))), ty, int(rng.integers(0, len(lists[ty]) - (ty == y) + 1))))
    return out


def _labels(moves, which):
    return {label for label, m in moves if m.list == which}


def _check_blocks(eng, pol, base, moves, what):
    """The plan blocks k_plan_moves writes against the blocks the host's write_lists builds for the moved plans, all 8 832 bytes of
    each (eg_debug_fetch_plan_block) — with the pool overwritten in between, so that nothing is left over from the host's blocks."""
    n = len(moves)
    eng.evaluate_plans(pol, [apply_move(base, m) for m in moves], 1, 0)
    host = [eng.debug_fetch_plan_block(j) for j in range(n)]
    eng.evaluate_plans(pol, [_junk_plan()] * n, 1, 0)
    assert eng.debug_fetch_plan_block(n - 1)[640:].min() == 59
    eng.evaluate_plan_moves(pol, base, moves, 1, 0)
    for j in range(n):
        dev = eng.debug_fetch_plan_block(j)
        if dev.tobytes() != host[j].tobytes():
            bad = np.flatnonzero(dev != host[j])
            raise AssertionError(f"{what}: block {j} ({moves[j]}) differs at bytes {bad[:8].tolist()} ({len(bad)} in all)")


def _bases(engine):
    short, long_ = _seeded(engine), _long_policy()
    assert len(Plan.from_policy(short)) == 28 and len(Plan.from_policy(long_)) >= 200
    return short, long_


def _full_plan(rng):
    """both lists at the 4 096-entry capacity: 150 entries a year, one year empty, the rest in one year"""
    def lists(extra_year, empty_year):
        l = [[int(a) for a in rng.integers(0, 61, 150)] for _ in range(26)]
        l[empty_year] = []
        l[extra_year] += [int(a) for a in rng.integers(0, 61, 4096 - 25 * 150)]
        return l
    plan = Plan(lists(3, 13), lists(25, 1))
    assert len(plan) == 4096 and sum(len(l) for l in plan.best_deficit_actions) == 4096
    return plan


# ---------------------------------------------------------------- the blocks
def test_blocks_are_write_lists_byte_for_byte_on_the_two_bases(world, engine):
    rng = np.random.default_rng(31)
    covered = [set(), set()]
    for name, pol in zip(("short", "long"), _bases(engine)):
        base = Plan.from_policy(pol)
        moves = _move_set(base)
        for which in (0, 1):
            covered[which] |= _labels(moves, which)
        only = [m for _, m in moves]
        if name == "short":      # batches of 1, 5 and 301 variants: the last workgroup holds one wave
            _check_blocks(engine, pol, base, only[:1], "short, 1 variant")
            _check_blocks(engine, pol, base, only[-5:], "short, 5 variants")
            only = (only + _random_moves(base, rng, 301))[:301]
            assert len(only) == 301
        _check_blocks(engine, pol, base, only, name)
    for which in (0, 1):
        assert covered[which] >= set(BOTH_LISTS), (which, set(BOTH_LISTS) - covered[which])


def test_blocks_of_full_lists_long_years_and_the_masks(world, engine):
    pol = ActionWeights()
    rng = np.random.default_rng(3)
    full = _full_plan(rng)
    moves = _move_set(full)
    for which in (0, 1):
        assert _labels(moves, which) >= set(BOTH_LISTS) | {"empty target", "long source", "long target"}, _labels(moves, which)
    # the first entry of year 0 behind the last of year 25: 4 095 bytes shift and every offset but the first moves — and back
    assert ("first to last", PlanMove(0, 0, 0, 25, 150)) in moves and ("last to first", PlanMove(0, 25, 149, 0, 0)) in moves
    assert ("first to last", PlanMove(1, 0, 0, 25, 150 + 346)) in moves and ("last to first", PlanMove(1, 25, 149 + 346, 0, 0)) in moves
    _check_blocks(engine, pol, full, [m for _, m in moves], "full lists")
    # masks on a small plan, where every case can be read off: the only occurrence of an action leaves its year (the bit clears in the
    # source year and is set in the target year), one of two occurrences leaves, the other occurrence sits in the other list
    run = [[] for _ in range(26)]; dfc = [[] for _ in range(26)]
    run[4] = [5, 9, 5, 33]; dfc[4] = [9, 24]; run[25] = [60]; run[5] = [33]; dfc[3] = [24, 9]
    small = Plan(run, dfc)
    moves = [PlanMove(0, 4, 3, 10, 0), PlanMove(0, 4, 3, 5, 1), PlanMove(0, 4, 0, 25, 1), PlanMove(0, 4, 2, 0, 0), PlanMove(0, 4, 1, 3, 0), PlanMove(0, 25, 0, 4, 2),
             PlanMove(1, 4, 0, 7, 0), PlanMove(1, 4, 1, 0, 0), PlanMove(1, 4, 1, 3, 1), PlanMove(1, 3, 1, 4, 0), PlanMove(1, 3, 0, 4, 2), PlanMove(0, 4, 0, 4, 2),
             PlanMove(0, 4, 3, 4, 0), PlanMove(1, 4, 0, 4, 1), PlanMove(0, 5, 0, 5, 0), PlanMove(1, 4, 1, 4, 1)]
    _check_blocks(engine, pol, small, moves, "masks")
    # a year of 200 entries whose only occurrence of an action sits behind the first 64 entries, as source and as target
    run = [[] for _ in range(26)]; dfc = [[] for _ in range(26)]
    run[7] = [3] * 130 + [44] + [3] * 69; run[8] = [6, 44]; dfc[7] = [24] * 70 + [21] + [24] * 5; dfc[9] = [21]
    wide = Plan(run, dfc)
    moves = [PlanMove(0, 7, 130, 8, 0), PlanMove(0, 7, 130, 6, 0), PlanMove(0, 8, 1, 7, 199), PlanMove(0, 8, 0, 7, 200), PlanMove(0, 7, 0, 7, 199), PlanMove(0, 7, 130, 7, 0),
             PlanMove(1, 7, 70, 9, 1), PlanMove(1, 7, 70, 25, 0), PlanMove(1, 9, 0, 7, 76), PlanMove(1, 7, 75, 7, 0)]
    _check_blocks(engine, pol, wide, moves, "years longer than a wave")


def test_blocks_through_a_slot_table_with_two_bases(world, engine):
    """k_plan_moves behind a slot table: one refinement round with moves over two plans in ONE launch (eg_refine_plans_moves; the round's
    variants stay behind as the last batch), a segment of edits then moves per plan.  Every move variant's block must be write_lists'
    block for the move applied to the base of ITS segment, all 8 832 bytes: a kernel that took base 0 for every variant, or the other
    segment's, would write the other plan's lists.  The moves land in another year of the moved list, up to two years away, at the two
    ends of the 26 years; an action leaves a year that holds it once, twice, and in the deficit list as well."""
    pol = ActionWeights()
    run = [[] for _ in range(26)]; dfc = [[] for _ in range(26)]
    run[0] = [0, 13]; run[3] = [36]; run[25] = [21]; dfc[3] = [36, 24]; dfc[12] = [24]
    a = Plan(run, dfc)
    run = [[] for _ in range(26)]; dfc = [[] for _ in range(26)]
    run[1] = [12, 12, 4]; run[24] = [7]; run[25] = [7, 2]; dfc[0] = [21]; dfc[24] = [7]
    b = Plan(run, dfc)
    plans = [a, b]
    engine.refine_plans(pol, plans, 7, 0, 1, 1, max_shift=2)
    picks, first = [], 0
    for plan in plans:
        n_edits, moves = len(round_edits(plan)), round_moves(plan, 2)
        picks += [(first + n_edits + k, apply_move(plan, m), m) for k, m in enumerate(moves)]
        first += n_edits + len(moves)
    assert N.lib().eg_last_batch_size(engine.h) == first == 18 + 25 and len(picks) == 10 + 16
    dev = [engine.debug_fetch_plan_block(j).copy() for j, _, _ in picks]
    engine.evaluate_plans(pol, [moved for _, moved, _ in picks], 7, 0)
    for k, ((j, _, m), d) in enumerate(zip(picks, dev)):
        host = engine.debug_fetch_plan_block(k)
        assert d.tobytes() == host.tobytes(), (j, m, np.flatnonzero(d != host)[:8])


# ---------------------------------------------------------------- the records
@pytest.mark.parametrize("helper", ["0", "all"])
def test_moves_are_the_host_built_plans(world, engine, helper):
    rng = np.random.default_rng(17)
    eng = _engine(world, EIRGRID_HELPER_WAVES=helper)
    try:
        for name, pol in zip(("short", "long"), _bases(engine)):
            base = Plan.from_policy(pol)
            moves = [m for _, m in _move_set(base)]
            sizes = (1, 5, 301) if name == "short" else (len(moves),)
            for n in sizes:
                batch = (moves + _random_moves(base, rng, max(n - len(moves), 0)))[:n]
                moved = [apply_move(base, m) for m in batch]
                want = eng.evaluate_plans(pol, moved, 77, 3000)
                got = eng.evaluate_plan_moves(pol, base, batch, 77, 3000, same_index=False)
                _same_records(got, want, (helper, name, n, "index + j"))
                got = eng.evaluate_plan_moves(pol, base, batch, 77, 3000, same_index=True)
                for j, p in enumerate(moved):
                    one = eng.evaluate_plans(pol, [p], 77, 3000)
                    _same_records(got, one, (helper, name, n, "same index", j, batch[j]), [j], [0])
            assert len({want.metrics[j].tobytes() for j in range(len(batch))}) > 3      # (the moves matter)
    finally:
        eng.close()


def test_lists_that_run_out_draw_the_same_fallbacks(world, engine):
    """a plan cut short draws seeded fallbacks when a year's list runs out: a moved variant draws what the host-built moved plan draws"""
    pol = _seeded(engine)
    base = Plan.from_policy(pol)
    cut = Plan([l[:len(l) // 2] for l in base.best_actions], [l[:1] for l in base.best_deficit_actions])
    moves = [PlanMove(0, y, 0, y, 0) for y in range(26) if cut.best_actions[y]][:1] + round_moves(cut, 2)[:30]
    for pol2 in (pol, ActionWeights()):
        want = engine.evaluate_plans(pol2, [apply_move(cut, m) for m in moves], 41, 700)
        assert (want.n_draws > 0).any()
        got = engine.evaluate_plan_moves(pol2, cut, moves, 41, 700, same_index=False)
        _same_records(got, want, "cut, index + j")
        got = engine.evaluate_plan_moves(pol2, cut, moves, 41, 700 + 3, same_index=True)
        _same_records(got, want, "cut, same index", [3], [3])


def test_every_variant_is_the_oracles_replay_of_the_moved_plan(world, engine):
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    pol = _seeded(engine)
    base = Plan.from_policy(pol)
    moves = [m for _, m in _move_set(base)][:24] + round_moves(base, 3)[::9]
    seed, first = 1234, 90_000
    eng = _engine(world, EIRGRID_HELPER_WAVES="0")
    try:
        for same in (True, False):
            got = eng.evaluate_plan_moves(pol, base, moves, seed, first, same_index=same)
            small = engine.evaluate_plan_moves(pol, base, moves, seed, first, same_index=same)      # (the small-batch kernel)
            for j, m in enumerate(moves if same else moves[:12]):
                st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, apply_move(base, m)), seed + first + (0 if same else j), replay=True)
                assert st == 0, (j, m)
                assert_episode_equal(got, j, ref, f"same_index {same}, move {j} {m}")
                assert_episode_equal(small, j, ref, f"(small-batch kernel) same_index {same}, move {j} {m}")
    finally:
        eng.close()


# ---------------------------------------------------------------- the timing report
def test_plan_timing_rows_are_the_moved_plans_scores(world, engine):
    pol = _seeded(engine)
    base = Plan.from_policy(pol)
    for mode, shift in ((1, 1), (2, 2)):
        t = engine.plan_timing(pol, base, 11, mode, shift)
        moves = round_moves(base, shift)
        assert t.moves[1:] == moves == refine_moves(base, shift) and len(t.moves) == 1 + len(moves)
        assert apply_move(base, t.moves[0]) == base      # row 0: the plan itself
        plans = [base] + [apply_move(base, m) for m in moves]
        rows = [engine.evaluate_plans(pol, [p], 11, 0) for p in plans]      # (every variant at global index 0)
        status = np.array([r.status[0] for r in rows]); metrics = np.array([r.metrics[0] for r in rows])
        score = np.array([rank_score(metrics[j], mode == 2) if status[j] == 0 else np.nan for j in range(len(plans))])
        assert t.status.tolist() == status.tolist() and (status == 0).all()
        assert t.metrics.tobytes() == metrics.tobytes() and t.score.tobytes() == score.tobytes()
        assert t.d_metrics.tobytes() == (metrics - metrics[0]).tobytes() and t.d_score.tobytes() == (score - score[0]).tobytes()
        assert (t.d_metrics[0] == 0).all() and t.d_score[0] == 0 and len(set(score.tolist())) > 3


# ---------------------------------------------------------------- refusals on the device side
def test_a_rank_of_a_group_is_refused(world):
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        base = Plan([[3, 12]] + [[] for _ in range(25)], [[] for _ in range(26)])
        with pytest.raises(EirgridError, match="eg_evaluate_plan_moves: the context is a rank of an eg_group"):
            g.ranks[0].evaluate_plan_moves(ActionWeights(), base, [PlanMove()], 1)
        with pytest.raises(EirgridError, match="eg_refine_plans_moves: the context is a rank of an eg_group"):
            g.ranks[0].refine_plans(ActionWeights(), [base], 1, max_shift=1)
    finally:
        g.close()


def test_an_invalid_move_is_refused_before_anything_runs(world, engine):
    pol = _seeded(engine)
    base = Plan.from_policy(pol)
    with pytest.raises(EirgridError, match="move 1: to_year 26"):
        engine.evaluate_plan_moves(pol, base, [PlanMove(), PlanMove(0, 0, 0, 26, 0)], 1)
