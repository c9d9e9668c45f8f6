"""GPU: build constraints (include/eirgrid_hip.h eg_build_constraints_set; csrc/eg_build_constraints.h k_build_constraints,
csrc/eg_constraints.cpp).  The fused kernel over crafted rows and crafted lists against the two restatements (tests/test_plan_constraints.py
judge for the row constraints, tests/test_build_constraints.py judge_built for the build constraints), byte for byte; the real 239-variant
edit batch of tests/test_gpu_plan_constraints.py under a bound chosen from its own lists; refine and repair against their host
restatements fed the restated judgment; build constraints without the yearly rows; and a plan whose emptied deficit lists draw fallbacks."""
import dataclasses
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.constraints import BuildConstraint, Constraint
from eirgrid_amd.engine import ActionMap, ActionWeights, Plan, PlanRewrite
from tests.test_build_constraints import NAMES, built_counts, judge_mixed
from tests.test_gpu_plan_constraints import NAME, _crafted, _excess_bytes, _other_bytes, constrained, short      # noqa: F401 (short: the module's fixture, reused)
from tests.test_gpu_plan_rewrites import _long_policy, _seeded
from tests.test_gpu_refine import _assert_same_trajectory
from tests.test_refine import CASES, SEED, apply_edit, refine_restated
from tests.test_repair import repair_restated

pytestmark = pytest.mark.gpu

OK, INFEASIBLE = N.EG_EP_OK, N.EG_EP_INFEASIBLE
LENGTHS = np.array([0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 4095, 4096])
WEIGHTS = np.array([0.0, 1.0, -1.0, 0.5, 3.25, 1e300])


def _lists_of(res):
    return res.n_gens, res.gen_pack, res.n_offsets, res.off_pack


def _assert_judged(got_status, got_violated, got_excess, want, what):
    status, violated, excess = want
    assert got_status.tolist() == status.tolist(), (what, "status")
    assert got_violated.tolist() == violated.tolist(), (what, "violated")
    assert got_excess.shape == (len(status), len(excess[0])) and _excess_bytes(got_excess) == excess, (what, "excess")


# ---------------------------------------------------------------- 1: crafted rows and lists through the debug hooks
def _crafted_lists(n, k_builds, rng):
    """lists over all 16 x 32 nibble / year values with random bytes behind the counts, lengths on the edges of a load and of the
    wave's stride, two records with count fields out of range, and k_builds constraints of which every third sits on a value"""
    gen_pack = rng.integers(0, 1 << 16, (n, N.MAX_GENS)).astype(np.uint16)
    off_pack = rng.integers(0, 1 << 16, (n, N.MAX_OFFSETS)).astype(np.uint16)
    n_gens, n_offsets = rng.choice(LENGTHS, n).astype(np.int32), rng.choice(LENGTHS, n).astype(np.int32)
    if n >= 3:
        n_gens[1], n_offsets[1] = -1, 5000
        n_gens[2], n_offsets[2] = 5000, -7
    counts = np.array(built_counts(gen_pack[0], n_gens[0], off_pack[0], n_offsets[0]))
    cs = []
    for i in range(k_builds):
        lo = int(rng.integers(0, 26)); hi = int(rng.integers(lo + 1, 27))
        if i % 5 == 0:
            lo, hi = 0, 26
        w = rng.choice(WEIGHTS, 19)
        if i % 4 == 1:
            w = rng.choice(WEIGHTS[:5], 19) * (rng.random(19) < 0.2) + 0.0
        if not w.any():
            w[int(rng.integers(0, 19))] = 1.0
        c = BuildConstraint(tuple(w), "<=" if rng.random() < 0.5 else ">=", 0.0, lo, hi, "sum" if i % 3 == 1 else "every")
        if i % 3 == 0:      # a bound that record 0's value sits on exactly (for EVERY: the value of the window's first year)
            bound = c.value(counts[lo:hi].sum(axis=0) if c.aggregate == "sum" else counts[lo])
        else:
            bound = float(rng.choice([0.0, 1.0, 40.0, -3.0, 2e300, float(rng.integers(0, 300))]))
        cs.append(dataclasses.replace(c, bound=bound))
    return n_gens, gen_pack, n_offsets, off_pack, cs


@pytest.mark.parametrize("k_rows, k_builds", [(0, 1), (0, 32), (1, 31), (31, 1), (16, 16)])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 64])
def test_crafted_lists_and_rows_are_judged_as_the_two_definitions_say(engine, n, k_rows, k_builds):
    rows, row_cs, status, metrics = _crafted(n, max(k_rows, 1), 1000 * n + k_rows)
    row_cs = row_cs[:k_rows]
    n_gens, gen_pack, n_offsets, off_pack, build_cs = _crafted_lists(n, k_builds, np.random.default_rng(77 * n + k_builds))
    with constrained(engine, row_cs + build_cs):
        engine._debug_load_batch(metrics, status, 40)
        engine._debug_load_yearly(rows)
        engine._debug_load_built(n_gens, gen_pack, n_offsets, off_pack)
        before = engine.fetch(n)
        assert before.status.tolist() == status.tolist() and before.n_gens.tolist() == n_gens.tolist() and before.n_offsets.tolist() == n_offsets.tolist()
        width = min(max(int(n_gens.max()), 0), N.MAX_GENS)      # (a fetch copies the lists as far as the longest count goes)
        assert before.gen_pack[:, :width].tobytes() == gen_pack[:, :width].tobytes()
        engine._debug_constrain_last_batch()
        violated, excess = engine.fetch_feasibility()
        judged_under = engine.last_batch_constraints()
        after = engine.fetch(n)
    assert judged_under == row_cs + build_cs
    want = judge_mixed(rows, n_gens, gen_pack, n_offsets, off_pack, status, row_cs, build_cs)
    _assert_judged(after.status, violated, excess, want, (n, k_rows, k_builds))
    assert _other_bytes(after) == _other_bytes(before)      # the rows, the metrics, the tags, the lists, the counts: nothing but the status moved
    if n >= 9 and k_builds >= 16:      # the crafted data does what it is there for
        built_bits = (want[1] >> np.uint32(k_rows))[status == OK]
        full = (1 << k_builds) - 1
        assert (built_bits != 0).any() and (built_bits != full).any()                                  # both outcomes
        assert (want[0][status != OK] == status[status != OK]).all() and (status != OK).any()           # failed records left alone
        for agg in ("every", "sum"):                                                                    # both aggregates, both outcomes each
            bits = sum(1 << i for i, c in enumerate(build_cs) if c.aggregate == agg)
            assert bits and (built_bits & bits != 0).any() and (built_bits & bits != bits).any(), agg
        on_bound = [i for i, c in enumerate(build_cs) if i % 3 == 0]
        if status[0] == OK:      # record 0 sits on every third bound: EVERY's excess is then >= 0 (the first year's is +0.0), SUM's exactly 0
            for i in on_bound:
                e = struct.unpack("<d", want[2][0][k_rows + i])[0]
                assert e == 0.0 if build_cs[i].aggregate == "sum" or build_cs[i].to_year == build_cs[i].from_year + 1 else e >= 0.0, i


def test_the_two_kernels_agree_on_the_row_constraints(engine):
    """k_plan_constraints under 31 row constraints, k_build_constraints under the same 31 and one build constraint: the staging and
    everything behind the fold are one piece of text (csrc/eg_plan_constraints.h pcons::stage_rows, store_judgment), so the 31 excess
    columns, the 31 mask bits and — where the build constraint holds — the statuses are the same bytes"""
    n = 5
    rows, row_cs, status, metrics = _crafted(n, 31, 5031)
    n_gens, gen_pack, n_offsets, off_pack, build_cs = _crafted_lists(n, 1, np.random.default_rng(5031))
    assert (status == OK).any() and (status != OK).any()

    def judged(cs):
        with constrained(engine, cs):
            engine._debug_load_batch(metrics, status, 40)
            engine._debug_load_yearly(rows)
            engine._debug_load_built(n_gens, gen_pack, n_offsets, off_pack)
            engine._debug_constrain_last_batch()
            violated, excess = engine.fetch_feasibility()
            return engine.fetch(n).status, violated, excess

    status_rows, violated_rows, excess_rows = judged(row_cs)
    status_both, violated_both, excess_both = judged(row_cs + build_cs)
    assert excess_rows.shape == (n, 31) and excess_both.shape == (n, 32)
    assert np.ascontiguousarray(excess_both[:, :31]).tobytes() == excess_rows.tobytes()
    assert (violated_both & np.uint32(2**31 - 1)).tolist() == violated_rows.tolist()
    built = (violated_both >> np.uint32(31)).astype(bool)
    assert status_both[~built].tolist() == status_rows[~built].tolist()
    assert built[status == OK].any() and not built[status == OK].all() and violated_rows.any()      # the crafted data does what it is there for


def test_the_hooks_and_the_setters_refuse_what_they_cannot_do(engine):
    L = N.lib()
    engine._debug_load_batch(np.zeros((2, 4)), np.zeros(2, np.int32), 0)
    with pytest.raises(EirgridError, match="no constraints are set"):
        engine._debug_constrain_last_batch()
    with pytest.raises(EirgridError, match="eg_debug_load_built: n = 3, the last batch holds 2 records"):
        engine._debug_load_built(np.zeros(3, np.int32), np.zeros((3, 4096), np.uint16), np.zeros(3, np.int32), np.zeros((3, 4096), np.uint16))
    assert L.eg_debug_load_built(engine.h, None, None, None, None, 2) == N.EG_ERR_BAD_ARG and "eg_debug_load_built: bad argument" in L.eg_last_error().decode()
    assert L.eg_last_batch_build_constraints(engine.h, None) == 0
    # together at most 32, whichever kind comes second; n = 0 clears one kind only
    rows = [Constraint("balance", ">=", float(i)) for i in range(32)]
    builds = [BuildConstraint({"Nuclear": 1.0}, "<=", float(i)) for i in range(32)]
    barr = (N.EgBuildConstraint * 32)(*[c.struct() for c in builds])
    rarr = (N.EgPlanConstraint * 32)(*[c.struct() for c in rows])
    try:
        assert L.eg_plan_constraints_set(engine.h, rarr, 20) == N.EG_OK
        assert L.eg_build_constraints_set(engine.h, barr, 13) == N.EG_ERR_BAD_ARG
        assert L.eg_last_error().decode() == "eg_build_constraints_set: n = 13 with 20 plan constraints set (together at most 32)"
        assert L.eg_build_constraints_set(engine.h, barr, 12) == N.EG_OK
        assert L.eg_plan_constraints_set(engine.h, rarr, 21) == N.EG_ERR_BAD_ARG
        assert L.eg_last_error().decode() == "eg_plan_constraints_set: n = 21 with 12 build constraints set (together at most 32)"
        assert L.eg_build_constraints_set(engine.h, barr, 33) == N.EG_ERR_BAD_ARG
        assert L.eg_last_error().decode() == "eg_build_constraints_set: n = 33 (0..32)"
        assert L.eg_plan_constraints_set(engine.h, None, 0) == N.EG_OK       # clears the rows only: the 12 build constraints still judge
        engine._debug_constrain_last_batch()
        assert engine.fetch_feasibility()[1].shape == (2, 12) and L.eg_last_batch_constraints(engine.h, None) == 0
        assert L.eg_last_batch_build_constraints(engine.h, None) == 12
        assert L.eg_build_constraints_set(engine.h, barr, 32) == N.EG_OK and L.eg_build_constraints_set(engine.h, None, 0) == N.EG_OK
        with pytest.raises(ValueError, match="is a row constraint behind a build constraint"):
            engine.set_constraints([builds[0], rows[0]])
        with pytest.raises(EirgridError, match=r"eg_build_constraints_set: n = 2 with 31 plan constraints set \(together at most 32\)"):
            engine.set_constraints(rows[:31] + builds[:2])
    finally:
        engine.clear_constraints()
    with pytest.raises(EirgridError, match="no constraints are set"):
        engine._debug_constrain_last_batch()


# ---------------------------------------------------------------- 2: the real edit batch under a bound chosen from its own lists
def _totals(res):
    """[n][19]: what every record of a batch built, per class, over all years"""
    return np.array([np.array(built_counts(*[a[j] for a in (res.gen_pack, res.n_gens, res.off_pack, res.n_offsets)])).sum(axis=0) for j in range(len(res.status))])


def _choose(totals, base_violates_by_one):
    """(class T, bound b) for `sum(built(T)) <= b`, chosen from the batch's own totals [n][19]: T is built by some variants and not by
    others or in different numbers, b splits the batch into variants at or under it and variants above it, and the base (variant 0) is at
    the bound — or, for a repair, one build above it.  Of the pairs that qualify, the one whose smaller side is largest."""
    n, best = len(totals), None
    for t in range(19):
        b = int(totals[0, t]) - (1 if base_violates_by_one else 0)
        if b < 0:
            continue
        under = int((totals[:, t] <= b).sum())
        if 0 < under < n and (best is None or min(under, n - under) > best[0]):
            best = (min(under, n - under), t, b)
    assert best is not None, "no class splits the batch around the base"
    return best[1], best[2]


@pytest.fixture(scope="module")
def chosen(short):
    pol, base, edits, free, row_cs = short
    totals = _totals(free)
    (t, b), (tr, br) = _choose(totals, False), _choose(totals, True)
    cap = BuildConstraint({NAMES[t]: 1.0}, "<=", float(b), aggregate="sum")
    broken = BuildConstraint({NAMES[tr]: 1.0}, "<=", float(br), aggregate="sum")
    # both outcomes exist under either, by the data: neither side of a split is empty, and at most half the batch lies on the smaller one
    for c, tt, bb in ((cap, t, b), (broken, tr, br)):
        under = int((totals[:, tt] <= bb).sum())
        assert 0 < min(under, len(totals) - under) <= len(totals) // 2, (str(c), under)
    print(f"chosen: {cap} (base at the bound), {broken} (base one build above)")
    return cap, broken


def _judged_free(free, row_cs, build_cs):
    return judge_mixed(free.yearly, *_lists_of(free), free.status, row_cs, build_cs)


def test_an_edit_batch_is_judged_on_what_its_variants_built(engine, short, chosen):
    pol, base, edits, free, row_cs = short
    cap, broken = chosen
    for cs in ([cap], [broken], [cap, broken]):
        with constrained(engine, cs):
            got = engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True)
            violated, excess = engine.fetch_feasibility()
            assert engine.last_batch_constraints() == cs
        _assert_judged(got.status, violated, excess, _judged_free(free, [], cs), [str(c) for c in cs])
        assert set(got.status.tolist()) == {OK, INFEASIBLE}
        assert _other_bytes(got) == _other_bytes(free)
    assert got.status[0] == INFEASIBLE and violated[0] == 2 and excess[0].tolist() == [0.0, 1.0]      # the base: at the cap, one build above the other bound
    # the fetch serves what the batch was judged under, whatever is set now
    assert engine.fetch_feasibility()[1].shape == (len(edits), 2) and engine.last_batch_constraints() == [cap, broken]


def _demoting_loop(eng, pol, row_cs, build_cs):
    def evaluate(plan, edits):
        res = eng.evaluate_plan_edits(pol, plan, edits, SEED, 0, same_index=True)
        return judge_mixed(res.yearly, *_lists_of(res), res.status, row_cs, build_cs)[0], res.metrics.copy()
    return evaluate


def _judging(eng, pol, row_cs, build_cs):
    def evaluate(plan, edits, moves):
        res = [eng.evaluate_plan_edits(pol, plan, edits, SEED, 0, same_index=True)]
        if moves:
            res.append(eng.evaluate_plan_moves(pol, plan, moves, SEED, 0, same_index=True))
        cat = lambda f: np.concatenate([getattr(r, f) for r in res])      # noqa: E731
        judged, violated, excess = judge_mixed(cat("yearly"), cat("n_gens"), cat("gen_pack"), cat("n_offsets"), cat("off_pack"), cat("status"), row_cs, build_cs)
        return judged, cat("metrics").copy(), excess
    return evaluate


def test_refine_plans_follows_the_restated_judgment(engine, short, chosen):
    pol, base, edits, free, row_cs = short
    case, (cap, broken) = CASES[NAME], chosen
    kw = dict(replace_with=case["replace_with"])
    with constrained(engine, [cap]):
        got = engine.refine_plans(pol, [base, apply_edit(base, edits[2])], SEED, 0, case["mode"], case["max_rounds"], **kw)
    for p, start in enumerate((base, apply_edit(base, edits[2]))):
        want = refine_restated(_demoting_loop(engine, pol, [], [cap]), start, case["mode"], case["max_rounds"], case["replace_with"])
        _assert_same_trajectory(got[p], want, ("refine_plans", p))
    assert got[0][2] != "base_failed" and got[0][1] and got[0][1][0].n_failed > 0      # the base is at the cap; the variants above it count as failed
    with constrained(engine, [broken]):
        stuck = engine.refine_plans(pol, [base], SEED, 0, case["mode"], 2, **kw)
    assert stuck[0][2] == "base_failed" and stuck[0][1] == []      # one build above the bound: refinement has no base to stand on


def _assert_repaired(engine, pol, got, want, row_cs, build_cs, what):
    plan, steps, stop, start, final, rec = got
    wplan, wsteps, wstop, wstart, wfinal = want
    assert stop == wstop and len(steps) == len(wsteps), (what, stop, wstop, len(steps), len(wsteps))
    assert (np.float64(start).tobytes(), np.float64(final).tobytes()) == (np.float64(wstart).tobytes(), np.float64(wfinal).tobytes()), (what, start, wstart, final, wfinal)
    for r, (s, w) in enumerate(zip(steps, wsteps)):
        assert type(s.edit) is type(w[0]) and s.edit == w[0], (what, r, s.edit, w[0])
        assert (s.variant, s.n_variants, s.n_failed, s.n_feasible, s.violated) == w[1:6], (what, r, s, w[1:6])
        assert np.float64(s.violation).tobytes() == np.float64(w[6]).tobytes() and np.float64(s.score).tobytes() == np.float64(w[7]).tobytes(), (what, r)
        assert s.metrics.tobytes() == w[8].tobytes(), (what, r)
    assert plan == wplan, what
    alone = engine.evaluate_plans(pol, [wplan], SEED, 0)      # the record: the returned plan's, but for the status the judgment gives it
    status = judge_mixed(alone.yearly, *_lists_of(alone), alone.status, row_cs, build_cs)[0]
    assert rec is not None and rec.status.tolist() == status.tolist() and rec.metrics.tobytes() == alone.metrics.tobytes(), (what, rec.status, status)
    assert rec.gen_pack[0, :rec.n_gens[0]].tobytes() == alone.gen_pack[0, :alone.n_gens[0]].tobytes(), what


def test_a_plan_one_build_above_the_bound_is_repaired_as_the_definition_says(engine, short, chosen):
    pol, base, edits, free, row_cs = short
    case, (cap, broken) = CASES[NAME], chosen
    hood = dict(replace_with=case["replace_with"])
    want = repair_restated(_judging(engine, pol, [], [broken]), base, 2, 4, **hood)
    assert want[2] == "feasible" and len(want[1]) >= 1 and want[3] == 1.0 and want[4] == 0.0, want[1:]      # one build above, and it comes out
    with constrained(engine, [broken]):
        got = engine.repair_plans(pol, [base], SEED, 0, 2, 4, **hood)
    _assert_repaired(engine, pol, got[0], want, [], [broken], "one build above")
    st, names, ex = engine.plan_feasibility(pol, [got[0][0]], SEED, 0, constraints=[broken])      # replayed alone, the repaired plan is legal
    assert st.tolist() == [OK] and names == [[]] and ex[0, 0] <= 0.0


def test_a_row_and_a_build_constraint_together_under_weights(engine, short, chosen):
    pol, base, edits, free, row_cs = short
    case, (cap, broken) = CASES[NAME], chosen
    hood = dict(replace_with=case["replace_with"])
    bad = apply_edit(base, edits[1])      # the plan that dips under the reserve on the balance (tests/test_gpu_repair.py)
    rows, builds, weights = row_cs[:1], [broken], [2.0, 0.5]
    with constrained(engine, rows + builds):
        got_batch = engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True)
        violated, excess = engine.fetch_feasibility()
        assert engine.last_batch_constraints() == rows + builds
        got = engine.repair_plans(pol, [base, bad], SEED, 0, 2, 3, violation_weights=weights, **hood)
    _assert_judged(got_batch.status, violated, excess, _judged_free(free, rows, builds), "a row and a build constraint")
    assert (violated & 1).any() and (violated & 2).any() and (violated == 0).any()      # either kind stops some variant, neither stops others
    for p, start in enumerate((base, bad)):
        want = repair_restated(_judging(engine, pol, rows, builds), start, 2, 3, weights=weights, **hood)
        _assert_repaired(engine, pol, got[p], want, rows, builds, ("mixed", p))
    assert got[0][3] == 0.5      # the base: one build above the bound at weight 0.5, the reserve met
    with constrained(engine, rows + builds):
        with pytest.raises(ValueError, match="1 violation weights for 2 constraints"):
            engine.repair_plans(pol, [base], SEED, 0, 2, 3, violation_weights=[1.0], **hood)


# ---------------------------------------------------------------- 3: build constraints do not need the yearly rows
def test_build_constraints_alone_are_judged_without_the_yearly_rows(engine, short, chosen):
    pol, base, edits, free, row_cs = short
    cap, broken = chosen
    with constrained(engine, [cap, broken]):
        got = engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True, write_yearly=False)
        violated, excess = engine.fetch_feasibility()
    _assert_judged(got.status, violated, excess, _judged_free(free, [], [cap, broken]), "write_yearly=False")
    assert got.metrics.tobytes() == free.metrics.tobytes() and set(got.status.tolist()) == {OK, INFEASIBLE}
    with constrained(engine, row_cs[:1] + [cap]):      # a row constraint keeps its refusal
        with pytest.raises(EirgridError, match="write_yearly = 0 while 1 plan constraints are set"):
            engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True, write_yearly=False)


# ---------------------------------------------------------------- 4: emptied deficit lists draw fallbacks, which are built all the same
def test_fallback_builds_are_judged_like_any_other(engine):
    """The deficit lists emptied as tests/test_gpu_plan_rewrites.py test_deficit_lists_that_run_out_draw_the_same_fallbacks empties them, under
    "no new gas".  Whether a fallback draw builds gas at this size is not known in advance: the judgment must equal the restatement on
    the fetched lists either way, and the case seen is printed."""
    pol = _seeded(engine)
    plans = [Plan.from_policy(pol), Plan.from_policy(_long_policy())]
    maps = [ActionMap.drop_all(), ActionMap.drop(range(30, 61))]
    rewrites = [PlanRewrite(p, m, f, t, l) for p in (0, 1) for m in range(2) for f, t, l in ((0, 26, 2), (0, 26, 3), (5, 20, 2))]
    no_gas = BuildConstraint.parse("built(GasPeaker + GasCombinedCycle) <= 0")
    for pol2 in (pol, ActionWeights()):
        free = engine.evaluate_plan_rewrites(pol2, plans, maps, rewrites, 41, 700, same_index=False)
        assert (free.n_draws > 0).any()      # fallbacks were drawn
        with constrained(engine, [no_gas]):
            got = engine.evaluate_plan_rewrites(pol2, plans, maps, rewrites, 41, 700, same_index=False)
            violated, excess = engine.fetch_feasibility()
        _assert_judged(got.status, violated, excess, _judged_free(free, [], [no_gas]), "fallbacks")
        assert _other_bytes(got) == _other_bytes(free)
        gas = [int(np.array(built_counts(free.gen_pack[j], free.n_gens[j], free.off_pack[j], free.n_offsets[j]))[:, [7, 8]].sum()) for j in range(len(rewrites))]
        print(f"gas built per variant with the deficit lists dropped: {gas}; infeasible: {int((got.status == INFEASIBLE).sum())} of {len(rewrites)}")
        assert [(g > 0) for g, s in zip(gas, free.status) if s == OK] == [bool(v) for v, s in zip(violated, free.status) if s == OK]
