"""GPU: plan streams end to end (include/eirgrid_hip.h eg_plan_streams_set; csrc/eg_streams.cpp, eg_plans.cpp launch_plans, csrc/eg_ensemble.h).
The base is config 1's episode (seed 12345) with its deficit list cut to one entry a year: its replay runs short of deficit actions and
falls back to seeded draws, so its outcome depends on the stream (the tabled oracle at seeds 1000..1003: 7, 3, 3 and 4 draws, four
different outcomes; the plan as recorded draws nothing and gives the same bits at every seed).

  streams are the batches they claim to be   fetch_streams()[r] of an R = 4 edit batch is the batch without streams at index + r, and the
                                             tabled oracle's replay for the base variant; the records are stream 0's but for metrics and
                                             status, which are engine.ensemble_reduce of the streams; so are the masks under a constraint
  same bits across streams                   the uncut plan commits its own metrics, for the mean and for the worst stream
  refinement                                 refine_plans under R = 3, tail = 1 against the host restatement fed reduced batches
  clearing, training batches                 nothing runs differently once the streams are cleared, and a training batch never sees them
  repair                                     refused while streams are set
  the long route                             a 120-action plan beside a short one in an R = 2 batch on the per-episode replay kernels"""
import contextlib
import dataclasses

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.constraints import Constraint
from eirgrid_amd.engine import HostTables, Plan, PlanEdit, ensemble_reduce
from oracle import api as O
from tests.test_gpu_parity import _used
from tests.test_gpu_plan_edits import _sized_plan
from tests.test_gpu_plans import _engine, _oracle_plan
from tests.test_gpu_refine import _assert_same_trajectory
from tests.test_gpu_replay_hoist import _seeded
from tests.test_refine import refine_restated, round_edits

pytestmark = pytest.mark.gpu

OK, INFEASIBLE = N.EG_EP_OK, N.EG_EP_INFEASIBLE
SEED, INDEX = 990, 10      # the streams of a batch at INDEX are the seeds 1000, 1001, ...


@contextlib.contextmanager
def streams(eng, n, tail=None, cost_only=False):
    """the engine under n streams; none afterwards, whatever happened (the engine fixture is the session's)"""
    eng.set_streams(n, tail, cost_only)
    try:
        yield eng
    finally:
        eng.clear_streams()


@pytest.fixture(scope="module")
def case(engine):
    """(policy, the plan as recorded, the cut plan, 40 one-entry edits of the cut plan: none, every delete, ten replaces)"""
    pol = _seeded(engine)
    base = Plan.from_policy(pol)
    cut = Plan(base.best_actions, [l[:1] for l in base.best_deficit_actions])
    assert len(base) == 28 and sum(len(l) for l in cut.best_deficit_actions) == 2
    edits = round_edits(cut)
    assert len(edits) == 31
    where = [(y, i) for y, l in enumerate(cut.best_actions) for i in range(len(l))]
    edits += [PlanEdit("replace", 0, y, i, 12) for y, i in where[::3]][:9]
    assert len(edits) == 40 and edits[0] == PlanEdit()
    return pol, base, cut, edits


def _outside(res):
    """every field of a fetched batch but metrics and status, as bytes; a list as far as its count goes (the records are not cleared
    between batches or passes: what lies behind a list's end is whatever was written there last)"""
    return {f.name: _used(res, f.name).tobytes() for f in dataclasses.fields(res) if f.name not in ("metrics", "status")}


def _assert_committed(res, rows, kept_m, kept_st, tail, cost_only=False):
    """the records' metrics and status, and the ensemble rows, are ensemble_reduce of the kept streams"""
    for j in range(kept_m.shape[1]):
        want = ensemble_reduce(kept_m[:, j], kept_st[:, j], tail, cost_only)
        assert res.metrics[j].tobytes() == want["committed"].tobytes() == rows.committed[j].tobytes(), j
        assert res.status[j] == want["status"] == rows.status[j], j
        assert rows.nominal[j].tobytes() == want["nominal"].tobytes(), j
        for name in ("score_min", "score_max", "score_sum"):
            assert np.float64(getattr(rows, name)[j]).tobytes() == np.float64(want[name]).tobytes(), (j, name)
        for name in ("n_ok", "n_infeasible", "n_failed", "worst_stream"):
            assert getattr(rows, name)[j] == want[name], (j, name)


def test_streams_are_the_batches_they_claim_to_be(world, engine, case):
    pol, base, cut, edits = case
    R, n = 4, len(edits)
    alone = [engine.evaluate_plan_edits(pol, cut, edits, SEED, INDEX + r, same_index=True) for r in range(R)]
    assert engine.last_batch_streams()[0] == 0
    with streams(engine, R):
        got = engine.evaluate_plan_edits(pol, cut, edits, SEED, INDEX, same_index=True)
        assert engine.last_batch_streams() == (R, R, False) and N.lib().eg_last_batch_size(engine.h) == n
        kept_m, kept_st = engine.fetch_streams()
        rows = engine.fetch_ensemble()
    assert kept_m.shape == (R, n, 4) and kept_st.shape == (R, n)
    for r in range(R):      # 1: every stream is the batch without streams at INDEX + r
        assert kept_m[r].tobytes() == alone[r].metrics.tobytes() and kept_st[r].tobytes() == alone[r].status.tobytes(), r
    assert (kept_st == OK).all()
    # the precondition: the base variant draws, and its streams differ
    assert got.n_draws[0] > 0 and len({kept_m[r, 0].tobytes() for r in range(R)}) >= 2
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    for r in range(R):      # 2: ... and the tabled oracle's replay of the cut plan at that seed
        st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, cut), SEED + INDEX + r, replay=True)
        assert st == 0 and np.array(ref.metrics).tobytes() == kept_m[r, 0].tobytes(), r
        assert ref.n_draws == alone[r].n_draws[0]
    assert _outside(got) == _outside(alone[0])      # 3: the records are stream 0's
    _assert_committed(got, rows, kept_m, kept_st, R)
    assert got.metrics.tobytes() != alone[0].metrics.tobytes()      # (the mean of four different outcomes is none of them)
    # 4: under one row constraint that some variants violate in some streams, the masks are stream 0's and the status is committed
    floor = float(np.median([a.yearly[:, :, 4].min(axis=1) for a in alone]))
    engine.set_constraints([Constraint("balance", ">=", floor)])
    try:
        judged = [engine.evaluate_plan_edits(pol, cut, edits, SEED, INDEX + r, same_index=True) for r in range(R)]
        engine.evaluate_plan_edits(pol, cut, edits, SEED, INDEX, same_index=True)
        masks = engine.fetch_feasibility()
        with streams(engine, R, tail=1):
            got = engine.evaluate_plan_edits(pol, cut, edits, SEED, INDEX, same_index=True)
            got_masks = engine.fetch_feasibility()
            kept_m, kept_st = engine.fetch_streams()
            rows = engine.fetch_ensemble()
            assert len(engine.last_batch_constraints()) == 1 and engine.last_batch_streams() == (R, 1, False)
    finally:
        engine.clear_constraints()
    assert got_masks[0].tobytes() == masks[0].tobytes() and got_masks[1].tobytes() == masks[1].tobytes()
    for r in range(R):
        assert kept_m[r].tobytes() == judged[r].metrics.tobytes() and kept_st[r].tobytes() == judged[r].status.tobytes(), r
    assert _outside(got) == _outside(judged[0])
    _assert_committed(got, rows, kept_m, kept_st, 1)
    differ = (kept_st != kept_st[0]).any(axis=0)
    assert set(kept_st.ravel().tolist()) == {OK, INFEASIBLE} and differ.any(), "the floor cuts through the streams"
    assert (got.status[differ] == INFEASIBLE).all() and (rows.n_infeasible[differ] > 0).all() and (rows.n_ok[differ] > 0).all()


@pytest.mark.parametrize("tail", [4, 1])
def test_the_same_bits_in_every_stream_commit_themselves(engine, case, tail):
    pol, base, cut, edits = case
    free = engine.evaluate_plan_edits(pol, base, [PlanEdit()], SEED, INDEX, same_index=True)
    assert free.status[0] == OK and free.n_draws[0] == 0
    with streams(engine, 4, tail):
        got = engine.evaluate_plan_edits(pol, base, [PlanEdit()], SEED, INDEX, same_index=True)
        kept_m, kept_st = engine.fetch_streams()
        rows = engine.fetch_ensemble()
    assert all(kept_m[r].tobytes() == free.metrics.tobytes() for r in range(4)) and (kept_st == OK).all()
    assert got.metrics.tobytes() == free.metrics.tobytes() and got.status.tobytes() == free.status.tobytes()      # (x + x + x + x) / 4.0 is x
    assert _outside(got) == _outside(free)
    assert rows.worst_stream[0] == 0 and rows.score_min[0] == rows.score_max[0] and rows.n_ok[0] == 4


def test_refinement_works_on_committed_outcomes(engine, case):
    pol, base, cut, edits = case
    emptied = Plan(base.best_actions, [[] for _ in range(26)])
    R, tail, rounds, index = 3, 1, 3, INDEX + 2      # (seeds 1002..1004: the cut plan's worst stream is the last)

    def reduced(plan, round_edits_):
        """three batches without streams, reduced on the host: what a round's pick reads under streams"""
        runs = [engine.evaluate_plan_edits(pol, plan, round_edits_, SEED, index + r, same_index=True) for r in range(R)]
        out = [ensemble_reduce([a.metrics[j] for a in runs], [a.status[j] for a in runs], tail) for j in range(len(round_edits_))]
        return np.array([o["status"] for o in out], np.int32), np.array([o["committed"] for o in out])

    want = [refine_restated(reduced, p, 1, rounds) for p in (cut, emptied)]
    with streams(engine, R, tail):
        got = engine.refine_plans(pol, [cut, emptied], SEED, index, 1, rounds)
        assert engine.last_batch_streams() == (R, tail, False)
    for p in range(2):
        _assert_same_trajectory(got[p], want[p], ("plan", p))
    assert sum(len(g[1]) for g in got) > 0, "a plan moves"
    # and the trajectory is not the one a single stream gives: the streams matter to the searches
    single = engine.refine_plans(pol, [cut, emptied], SEED, index, 1, rounds)
    assert any([(s.edit, s.score) for s in single[p][1]] != [(s.edit, s.score) for s in got[p][1]] for p in range(2))


def test_clearing_leaves_nothing_behind_and_training_never_sees_streams(world, engine, case):
    pol, base, cut, edits = case
    plans = [_sized_plan(120), cut, base, Plan(_sized_plan(130).best_actions, [l[:1] for l in _sized_plan(130).best_deficit_actions])]
    fresh = _engine(world)
    try:
        want = fresh.evaluate_plans(pol, plans, SEED, INDEX)
        want_training = fresh.rollout_batch(pol, SEED, 16, INDEX)
    finally:
        fresh.close()
    with streams(engine, 5, 2):
        under = engine.evaluate_plans(pol, plans, SEED, INDEX)
        assert engine.last_batch_streams() == (5, 2, False)
        training = engine.rollout_batch(pol, SEED, 16, INDEX)
        assert engine.last_batch_streams()[0] == 0
        with pytest.raises(N.EirgridError, match="the last batch ran without plan streams"):
            engine.fetch_streams()
    got = engine.evaluate_plans(pol, plans, SEED, INDEX)
    assert engine.last_batch_streams() == (0, 0, False)
    for f in dataclasses.fields(got):
        assert _used(got, f.name).tobytes() == _used(want, f.name).tobytes(), f.name
        assert _used(training, f.name).tobytes() == _used(want_training, f.name).tobytes(), f.name
    assert _outside(under) == _outside(want) and under.metrics.tobytes() != want.metrics.tobytes()


def test_repair_is_refused_under_streams(engine, case):
    pol, base, cut, edits = case
    engine.set_constraints([Constraint("balance", ">=", 0.0)])
    try:
        with streams(engine, 2):
            with pytest.raises(N.EirgridError, match=r"eg_repair_plans: 2 plan streams are set \(eg_plan_streams_set\): a repair reads the excess rows, which are stream 0's"):
                engine.repair_plans(pol, [cut], SEED, INDEX, max_rounds=2)
        assert len(engine.repair_plans(pol, [cut], SEED, INDEX, max_rounds=1)) == 1      # (and runs again once they are cleared)
    finally:
        engine.clear_constraints()


def test_the_passes_take_the_long_route(world, case):
    """EIRGRID_HELPER_WAVES=0: the long plan of a small batch runs k_replay_solo and the long-replay kernel, through launch_plans' chunk loop"""
    pol, base, cut, edits = case
    long_cut = Plan(_sized_plan(120).best_actions, [l[:1] for l in _sized_plan(120).best_deficit_actions])
    assert len(long_cut) == 120 > 96
    eng = _engine(world, EIRGRID_HELPER_WAVES="0")
    try:
        alone = [eng.evaluate_plans(pol, [long_cut, cut], SEED, INDEX + r) for r in range(2)]
        eng.set_streams(2)
        got = eng.evaluate_plans(pol, [long_cut, cut], SEED, INDEX)
        kept_m, kept_st = eng.fetch_streams()
        rows = eng.fetch_ensemble()
    finally:
        eng.close()
    for r in range(2):
        assert kept_m[r].tobytes() == alone[r].metrics.tobytes() and kept_st[r].tobytes() == alone[r].status.tobytes(), r
    assert _outside(got) == _outside(alone[0]) and got.n_gens[0] >= 120
    _assert_committed(got, rows, kept_m, kept_st, 2)
    assert got.n_draws[0] > 0 and kept_m[0, 0].tobytes() != kept_m[1, 0].tobytes(), "the long plan's streams differ"
