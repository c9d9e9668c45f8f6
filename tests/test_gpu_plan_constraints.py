"""GPU: plan constraints (include/eirgrid_hip.h eg_plan_constraints_set; csrc/eg_plan_constraints.h k_plan_constraints, csrc/eg_constraints.cpp).
The kernel over crafted rows against the Python restatement (tests/test_plan_constraints.py excess_bytes / judge), byte for byte; a real
edit batch with and without constraints; and every search — refine, breed, explore — against the host restatement its own tests use,
fed the statuses as the restatement demotes them."""
import contextlib
import dataclasses
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.constraints import Constraint
from eirgrid_amd.engine import ActionMap, ActionWeights, Engine, Plan, PlanRewrite, refine_edits
from tests.test_gpu_breed import _assert_is as _assert_breed_is, breed_restated
from tests.test_gpu_explore import _assert_is as _assert_explore_is, explore_restated
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plans import _same_records
from tests.test_gpu_refine import _assert_same_trajectory
from tests.test_plan_constraints import judge
from tests.test_refine import CASES, SEED, apply_edit, refine_restated, round_edits

pytestmark = pytest.mark.gpu

OK, INFEASIBLE = N.EG_EP_OK, N.EG_EP_INFEASIBLE
NAME = "short, mode 2"


@contextlib.contextmanager
def constrained(eng, constraints):
    """the engine under `constraints`; none afterwards, whatever happened (the engine fixture is the session's)"""
    eng.set_constraints(constraints)
    try:
        yield eng
    finally:
        eng.clear_constraints()


def _excess_bytes(excess):
    return [[struct.pack("<d", v) for v in row] for row in np.asarray(excess)]


def _assert_judged(got_status, got_violated, got_excess, yearly, status_in, constraints, what):
    status, violated, excess = judge(yearly, status_in, constraints)
    assert got_status.tolist() == status.tolist(), (what, "status")
    assert got_violated.tolist() == violated.tolist(), (what, "violated")
    assert got_excess.shape == (len(status_in), len(constraints)) and _excess_bytes(got_excess) == excess, (what, "excess")


def _other_bytes(res):
    """every field of a fetched batch but the status, as bytes"""
    return {f.name: getattr(res, f.name).tobytes() for f in dataclasses.fields(res) if f.name != "status"}


# ---------------------------------------------------------------- 1: crafted rows through the debug hooks
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 7.0])


def _crafted(n, k, seed):
    rng = np.random.default_rng(seed)
    rows = rng.normal(0.0, 10.0, (n, 26, 21)).round(1)
    hit = rng.random(rows.shape) < 0.03
    rows[hit] = rng.choice(SPECIAL, int(hit.sum()))
    rows[:, :, 3] = 7.0      # a column that equals a bound everywhere
    cs = []
    for i in range(k):
        lo = int(rng.integers(0, 26)); hi = int(rng.integers(lo + 1, 27))
        if i % 5 == 0:
            lo, hi = 0, 26
        col = 3 if i % 7 == 3 else int(rng.integers(0, 21))
        bound = 7.0 if col == 3 else float(rng.choice([0.0, -0.0, 7.0, -12.5, 30.0, 250.0, float(rows[0, lo, col]) if np.isfinite(rows[0, lo, col]) else 1.0]))
        cs.append(Constraint(col, "<=" if rng.random() < 0.5 else ">=", bound, lo, hi, "sum" if i % 3 == 1 else "every"))
    status = rng.choice(np.array([0, 0, 0, -1, -2], np.int32), n).astype(np.int32)
    status[0] = 0
    metrics = rng.normal(0.0, 1.0, (n, 4))
    return rows, cs, status, metrics


@pytest.mark.parametrize("k", [1, 31, 32])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 64])
def test_crafted_rows_are_judged_as_the_definition_says(engine, n, k):
    rows, cs, status, metrics = _crafted(n, k, 1000 * n + k)
    with constrained(engine, cs):
        engine._debug_load_batch(metrics, status, 40)
        engine._debug_load_yearly(rows)
        before = engine.fetch(n)
        assert before.status.tolist() == status.tolist() and before.yearly.tobytes() == rows.tobytes()
        engine._debug_constrain_last_batch()
        violated, excess = engine.fetch_feasibility()
        after = engine.fetch(n)
    _assert_judged(after.status, violated, excess, rows, status, cs, (n, k))
    assert _other_bytes(after) == _other_bytes(before)      # the rows, the metrics, the tags, the lists: nothing but the status moved
    want = judge(rows, status, cs)[0]
    if n >= 9:      # the crafted data does what it is there for: both outcomes, and failed records left alone
        assert (want == INFEASIBLE).any() and (want[status != OK] == status[status != OK]).all()


def test_the_hooks_refuse_what_they_cannot_do(engine):
    engine._debug_load_batch(np.zeros((2, 4)), np.zeros(2, np.int32), 0)
    with pytest.raises(EirgridError, match="no constraints are set"):
        engine._debug_constrain_last_batch()
    with pytest.raises(EirgridError, match="n = 3, the last batch holds 2 records"):
        engine._debug_load_yearly(np.zeros((3, 26, 21)))


# ---------------------------------------------------------------- 2: a real edit batch
@pytest.fixture(scope="module")
def short(engine):
    """(policy, base, edits, the unconstrained batch of the 239 round-0 variants, [floor on the balance, floor on the summed generation])"""
    case = CASES[NAME]
    pol = case["policy"]()
    base = Plan.from_policy(pol)
    edits = refine_edits(base, replace_with=case["replace_with"])
    assert edits == round_edits(base, case["replace_with"]) and len(edits) == 239
    free = engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True)
    assert free.status[0] == OK
    gen = Constraint("gen", ">=", 0.0, aggregate="sum")
    gen = dataclasses.replace(gen, bound=-gen.excess(free.yearly[0]))      # the base's own sum, folded in year order
    cs = [Constraint("balance", ">=", float(free.yearly[0][:, 4].min())), gen]
    return pol, base, edits, free, cs


def test_an_edit_batch_is_demoted_and_otherwise_untouched(engine, short):
    pol, base, edits, free, cs = short
    assert (free.status == OK).all()
    with constrained(engine, cs):
        got = engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True)
        violated, excess = engine.fetch_feasibility()
    _assert_judged(got.status, violated, excess, free.yearly, free.status, cs, "239 edits")
    assert got.metrics.tobytes() == free.metrics.tobytes() and got.yearly.tobytes() == free.yearly.tobytes()      # byte for byte
    for name in _ALL_FIELDS + ("n_chunks",):      # ... and every other field but the status, as far as an episode fills it
        assert name == "status" or _used(got, name).tobytes() == _used(free, name).tobytes(), name
    feasible = int((got.status == OK).sum())
    assert 0 < feasible < len(edits) and got.status[0] == OK and excess[0].tolist() == [0.0, 0.0]
    assert set(got.status.tolist()) == {OK, INFEASIBLE}
    # plan_feasibility says the same of the same plans evaluated one by one at the same index
    few = [0, 1, 2, int(np.flatnonzero(got.status != OK)[-1])]
    for j in few:
        st, names, ex = engine.plan_feasibility(pol, [apply_edit(base, edits[j])], SEED, 0, constraints=cs)
        assert st[0] == got.status[j] and names[0] == [c for i, c in enumerate(cs) if violated[j] >> i & 1] and ex.tobytes() == excess[j:j + 1].tobytes(), j
    with pytest.raises(EirgridError, match="ran without plan constraints"):      # plan_feasibility put the engine's own (none) back ...
        engine.evaluate_plans(pol, [base], SEED, 0)
        engine.fetch_feasibility()


# ---------------------------------------------------------------- 3: refinement under the constraint
def _demoting_loop(eng, pol, constraints, seen=None):
    """a round's variants evaluated WITHOUT constraints and demoted by the restatement"""
    def evaluate(plan, edits):
        res = eng.evaluate_plan_edits(pol, plan, edits, SEED, 0, same_index=True)
        status = judge(res.yearly, res.status, constraints)[0]
        if seen is not None:
            seen.append(int(status[0]))
        return status, res.metrics.copy()
    return evaluate


def test_refine_plan_and_refine_plans_follow_the_demoted_definition(engine, short):
    pol, base, edits, free, cs = short
    case = CASES[NAME]
    cs = cs[:1]      # the reserve on the balance
    second = apply_edit(base, edits[2])      # another base that meets the reserve (the test checks it)
    kw = dict(replace_with=case["replace_with"])
    unconstrained = engine.refine_plan(pol, base, SEED, 0, case["mode"], case["max_rounds"], **kw)
    with constrained(engine, cs):
        one = engine.refine_plan(pol, base, SEED, 0, case["mode"], case["max_rounds"], **kw)
        many = engine.refine_plans(pol, [base, second], SEED, 0, case["mode"], case["max_rounds"], **kw)
    for what, got, start in (("refine_plan", one, base), ("refine_plans[0]", many[0], base), ("refine_plans[1]", many[1], second)):
        bases_seen = []
        want = refine_restated(_demoting_loop(engine, pol, cs, bases_seen), start, case["mode"], case["max_rounds"], case["replace_with"])
        _assert_same_trajectory(got, want, what)
        assert got[2] != "base_failed" and bases_seen and all(s == OK for s in bases_seen), (what, bases_seen)      # every visited base is feasible
    assert one[1] and unconstrained[1] and one[1][0].n_failed > 0      # (the infeasible variants are counted as failed)
    assert (one[1][0].variant, one[1][0].edit) != (unconstrained[1][0].variant, unconstrained[1][0].edit)      # the constraint turned the search
    # the refined plan, replayed alone, is feasible
    st, names, ex = engine.plan_feasibility(pol, [one[0], many[1][0]], SEED, 0, constraints=cs)
    assert st.tolist() == [OK, OK] and names == [[], []]


def test_refining_an_infeasible_base_stops_with_base_failed(engine, short):
    pol, base, edits, free, cs = short
    bad = apply_edit(base, edits[1])      # the unconstrained winner: it dips under the reserve
    with constrained(engine, cs[:1]):
        plan, steps, stop, start, rec = engine.refine_plan(pol, bad, SEED, 0, 2, 3)
    assert stop == "base_failed" and steps == [] and plan == bad and np.isnan(start)


# ---------------------------------------------------------------- 4: breed and explore
class DemotingEngine:
    """what breed_restated / explore_restated evaluate with: the engine WITHOUT constraints, the statuses demoted by the restatement"""

    def __init__(self, eng, constraints):
        self.eng, self.constraints = eng, constraints

    def _demote(self, res):
        res.status[:] = judge(res.yearly, res.status, self.constraints)[0]
        return res

    def evaluate_plan_edits(self, *a, **kw):
        return self._demote(self.eng.evaluate_plan_edits(*a, **kw))

    def evaluate_plan_moves(self, *a, **kw):
        return self._demote(self.eng.evaluate_plan_moves(*a, **kw))

    def evaluate_plan_crosses(self, *a, **kw):
        return self._demote(self.eng.evaluate_plan_crosses(*a, **kw))


ALL = ("emissions", "opinion", "cost", "reliability")
CUTS = (5, 13, 20)
HOOD = dict(replace_with=(12,), append_with=None, max_shift=0)


def _three(short):
    pol, base, edits, free, cs = short
    return pol, [Plan(base.best_actions, base.best_deficit_actions, "base"), apply_edit(base, edits[2]), apply_edit(base, edits[1])], cs[0]


def _cutting_reserve(engine, pol, members, base_reserve):
    """a reserve on the balance that cuts at least one of `members` (an unconstrained front; the callers verify the cut): the largest of
    their minimum balances, each plan evaluated alone at the searches' index — or, where they all dip to the same minimum, the base
    plan's own reserve"""
    res = engine.evaluate_plan_rewrites(pol, members, [ActionMap.identity()], [PlanRewrite(p, 0, 0, 0, 0) for p in range(len(members))], SEED, 0)
    assert (res.status == OK).all()
    lows = res.yearly[:, :, 4].min(axis=1)
    return [Constraint("balance", ">=", float(lows.max()))] if lows.min() < lows.max() else [base_reserve]


def _statuses_alone(engine, pol, plans, cs):
    """the status of every plan evaluated alone at the searches' index, under the constraints"""
    with constrained(engine, cs):
        return engine.evaluate_plan_rewrites(pol, plans, [ActionMap.identity()], [PlanRewrite(p, 0, 0, 0, 0) for p in range(len(plans))], SEED, 0).status.tolist()


def test_breed_front_keeps_feasible_members_only(engine, short):
    pol, plans, reserve = _three(short)
    free = engine.breed_front(pol, plans, SEED, 0, objectives=ALL, cuts=CUTS, generations=2, cap=8)
    cs = _cutting_reserve(engine, pol, free.plans, reserve)
    assert INFEASIBLE in _statuses_alone(engine, pol, free.plans, cs)      # the constraint cuts a member of the unconstrained front
    with constrained(engine, cs):
        front = engine.breed_front(pol, plans, SEED, 0, objectives=ALL, cuts=CUTS, generations=2, cap=8)
    ref = breed_restated(DemotingEngine(engine, cs), pol, plans, SEED, 0, ALL, False, CUTS, 2, 8, N.CROSS_MAX_VARIANTS)
    _assert_breed_is(front, ref, "breed under the reserve")
    assert front.plans and front.plans == ref["pops"][-1]
    assert _statuses_alone(engine, pol, front.plans, cs) == [OK] * len(front.plans)


def test_explore_front_keeps_feasible_members_only(engine, short):
    pol, plans, reserve = _three(short)
    free = engine.explore_front(pol, plans, SEED, 0, objectives=ALL, generations=2, cap=8, launch=N.REFINE_MAX_VARIANTS, **HOOD)
    cs = _cutting_reserve(engine, pol, free.plans, reserve)
    assert INFEASIBLE in _statuses_alone(engine, pol, free.plans, cs)
    with constrained(engine, cs):
        front = engine.explore_front(pol, plans, SEED, 0, objectives=ALL, generations=2, cap=8, launch=N.REFINE_MAX_VARIANTS, **HOOD)
    ref = explore_restated(DemotingEngine(engine, cs), pol, plans, SEED, 0, ALL, False, 2, 8, N.REFINE_MAX_VARIANTS, HOOD)
    _assert_explore_is(front, ref, "explore under the reserve")
    assert front.plans and _statuses_alone(engine, pol, front.plans, cs) == [OK] * len(front.plans)


def test_explore_front_repairs_an_infeasible_start(engine, short):
    pol, base, edits, free, cs = short
    bad = apply_edit(base, edits[1])      # the unconstrained winner of the refinement: its balance dips furthest
    hood = refine_edits(bad, replace_with=HOOD["replace_with"])
    lows = engine.evaluate_plan_edits(pol, bad, hood, SEED, 0, same_index=True).yearly[:, :, 4].min(axis=1)
    assert lows.max() > lows[0]      # some one-entry edit lifts the plan's minimum balance: a reserve there is out of the plan's reach, not its neighbours'
    cs = [Constraint("balance", ">=", float(lows.max()))]
    assert _statuses_alone(engine, pol, [bad], cs) == [INFEASIBLE]
    with constrained(engine, cs):
        front = engine.explore_front(pol, [bad], SEED, 0, objectives=ALL, generations=1, cap=8, launch=N.REFINE_MAX_VARIANTS, **HOOD)
    ref = explore_restated(DemotingEngine(engine, cs), pol, [bad], SEED, 0, ALL, False, 1, 8, N.REFINE_MAX_VARIANTS, HOOD)
    _assert_explore_is(front, ref, "explore from an infeasible start")
    # the start is not a member; its feasible neighbours are
    assert front.plans and bad not in front.plans and _statuses_alone(engine, pol, front.plans, cs) == [OK] * len(front.plans)


# ---------------------------------------------------------------- 5: state
def test_clearing_restores_the_unconstrained_bytes(engine, short):
    pol, base, edits, free, cs = short
    with constrained(engine, cs):
        engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True)
    again = engine.evaluate_plan_edits(pol, base, edits, SEED, 0, same_index=True)
    assert again.status.tobytes() == free.status.tobytes() and again.metrics.tobytes() == free.metrics.tobytes() and again.yearly.tobytes() == free.yearly.tobytes()
    _same_records(again, free, "after clear_constraints")
    with pytest.raises(EirgridError, match="eg_fetch_plan_feasibility: the last batch ran without plan constraints"):
        engine.fetch_feasibility()


def test_a_fetch_serves_the_constraints_the_batch_ran_under_whatever_is_set_since(engine, short):
    """the excess matrix is [n][k] with k the constraints of the BATCH: clearing them, or setting more or fewer, between the batch and
    the fetch changes neither its shape nor its bytes, and last_batch_constraints says which they were"""
    pol, base, edits, free, cs = short
    three = cs + [Constraint("net_co2", "<=", 0.0, 15, 26)]
    with constrained(engine, three):
        engine.evaluate_plan_edits(pol, base, edits[:9], SEED, 0, same_index=True)
        violated, excess = engine.fetch_feasibility()
        assert excess.shape == (9, 3) and engine.last_batch_constraints() == three
    # cleared: the batch's three columns still
    v0, e0 = engine.fetch_feasibility()
    assert e0.shape == (9, 3) and e0.tobytes() == excess.tobytes() and v0.tobytes() == violated.tobytes() and engine.last_batch_constraints() == three
    many = [Constraint("balance", ">=", -1e300)] * 32
    with constrained(engine, many):      # 32 set now, 3 judged
        v1, e1 = engine.fetch_feasibility()
        assert e1.shape == (9, 3) and e1.tobytes() == excess.tobytes() and v1.tobytes() == violated.tobytes()
        engine.evaluate_plan_edits(pol, base, edits[:5], SEED, 0, same_index=True)
    with constrained(engine, cs[:1]):      # 1 set now, 32 judged
        v2, e2 = engine.fetch_feasibility()
        assert e2.shape == (5, 32) and (v2 == 0).all() and (e2 <= 0.0).all() and engine.last_batch_constraints() == many
    engine.set_constraints(c for c in three)      # a generator is walked once: uploaded AND remembered
    try:
        engine.evaluate_plan_edits(pol, base, edits[:9], SEED, 0, same_index=True)
        assert engine.fetch_feasibility()[1].tobytes() == excess.tobytes() and engine._constraints == three
    finally:
        engine.clear_constraints()
    engine.evaluate_plans(pol, [base], SEED, 0)
    assert engine.last_batch_constraints() == []


def test_write_yearly_off_is_refused_under_constraints(engine, short):
    pol, base, edits, free, cs = short
    with constrained(engine, cs):
        for call in (lambda: engine.evaluate_plans(pol, [base], SEED, 0, write_yearly=False),
                     lambda: engine.evaluate_plan_edits(pol, base, edits[:3], SEED, 0, write_yearly=False),
                     lambda: engine.refine_plan(pol, base, SEED, 0, 2, 1, write_yearly=False)):
            with pytest.raises(EirgridError, match="write_yearly = 0 while 2 plan constraints are set"):
                call()
    assert engine.evaluate_plans(pol, [base], SEED, 0, write_yearly=False).status[0] == OK      # without constraints it is allowed as before


def test_set_refuses_bad_constraints_and_keeps_none(engine, short):
    pol, base, edits, free, cs = short
    with pytest.raises(EirgridError, match="eg_plan_constraints_set: constraint 0: to_year 27"):
        engine.set_constraints([Constraint("balance", ">=", 0.0, 0, 27)])
    with pytest.raises(EirgridError, match=r"n = 33 \(0\.\.32\)"):
        engine.set_constraints([Constraint("balance", ">=", 0.0)] * 33)
    assert engine.evaluate_plans(pol, [base], SEED, 0).status[0] == OK
    with pytest.raises(EirgridError, match="ran without plan constraints"):
        engine.fetch_feasibility()


def test_a_rank_of_a_group_is_refused(world):
    from eirgrid_amd.engine import Group
    g = Group(world, devices=(0, 0))
    try:
        with pytest.raises(EirgridError, match="eg_plan_constraints_set: the context is a rank of an eg_group"):
            g.ranks[0].set_constraints([Constraint("balance", ">=", 0.0)])
    finally:
        g.close()


def test_training_between_constrained_plan_batches_is_unaffected(world, short):
    pol_eval, base, edits, free, cs = short
    out = []
    for constrain in (False, True):
        eng = Engine(world, device=0)
        try:
            if constrain:
                eng.set_constraints([Constraint("balance", ">=", 1e12)])      # nothing meets it: every variant of a plan batch is demoted
            eng.push(ActionWeights())
            eng.device_step(3, 0, 256, 10, 3)
            a = eng.evaluate_plan_edits(pol_eval, base, edits[:8], SEED, 0)
            eng.device_step(3, 256, 256, 10, 4)
            batch = eng.fetch(256)
            if constrain:
                with pytest.raises(EirgridError, match="ran without plan constraints"):      # the last batch is the training step's
                    eng.fetch_feasibility()
            b = eng.evaluate_plan_edits(pol_eval, base, edits[:8], SEED, 0)
            assert (a.status == (INFEASIBLE if constrain else OK)).all() and (b.status == a.status).all()
            pol = ActionWeights(); eng.pull(pol)
            out.append((batch, [t.tobytes() for t in pol.tables()], [pol.lists(0), pol.lists(1)]))
        finally:
            eng.close()
    (ba, ta, la), (bb, tb, lb) = out
    assert (ba.status == OK).any() and ba.status.tobytes() == bb.status.tobytes() and ba.metrics.tobytes() == bb.metrics.tobytes()
    _same_records(ba, bb, "the training step's records")
    assert ta == tb and la == lb      # the policy the two steps left
