"""GPU: the batch update at the batch sizes the project trains at, against the oracle's independent libm restatement
(oracle/eg_oracle.c og_reduced_batch_update).

Above helper_max_episodes (4 x the CUs: 1 024 on an MI355X) a batch runs the one-wave kernels: their statistics epilogue, k_replay_solo's
own epilogue call for long replays, the hoisted replay's statistics (one evaluation counted n_replay times) and, from 4 096 episodes, the
64 replicas of the statistics that k_fold_stats sums into the packet and clears.  The bar is the one of
test_gpu_reduced_oracle.py::test_statistics_epilogue_equals_restatement: counters and deficit counts exact, the Q32 logarithm sums within
2 units (ocml against glibc pow / log), the candidate the restatement's winner, slot 3 within 8 units."""
import numpy as np
import pytest
import torch

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, Plan
from oracle import api as O
from tests.helpers import oracle_weights_like
from tests.test_gpu_plans import _engine
from tests.test_gpu_reduced_oracle import assert_same_policy, batch_arrays
from tests.test_gpu_replay_hoist import _full_script, _seeded

pytestmark = pytest.mark.gpu

A = N.YEARS * N.N_ACTIONS
BEST = ("best_net_emissions", "best_opinion", "best_cost", "best_reliability")


def _best_score(pol):
    return O.score_metrics([pol.get(k) for k in BEST])


def _compare_packet(host, res, pol, what):
    """The packet of a batch against the restatement of the same episodes from the same policy: (the restatement's statistics, its
    winner, how many Q32 sums are identical)."""
    n = len(res.status)
    dev = host[:8 * N.STATS_LEN].view(np.int64)
    _, ref, winner = O.reduced_batch_update(oracle_weights_like(pol), *batch_arrays(res), noise_seed=1)
    assert dev[0] + dev[1] == n, (what, "every episode counted once", dev[:3].tolist())
    assert (dev[:3] == ref[:3]).all(), (what, dev[:3].tolist(), ref[:3].tolist())
    assert (dev[8 + 2 * A:] == ref[8 + 2 * A:]).all(), (what, "deficit counts")
    diff = np.abs(dev[8:8 + 2 * A] - ref[8:8 + 2 * A])
    assert diff.max() <= 2, f"{what}: logarithm sums differ by {diff.max()} Q32 units (worst entry {int(diff.argmax())})"
    assert abs(int(dev[3]) - int(ref[3])) <= 8, (what, int(dev[3]), int(ref[3]))
    return ref, winner, int((diff == 0).sum())


def _packet_batch(eng, pol, seed, first, n, mask=None, period=None):
    """One batch with the statistics epilogue: launch_update (a host mask) or device_rollout (a period; the pushed policy)."""
    packet = torch.zeros(N.PACKET_BYTES, dtype=torch.uint8, device="cuda")
    if period is None:
        eng.upload_snapshot(pol)
        eng.launch_update(seed, first, n, packet.data_ptr(), replay_mask=mask)
    else:
        eng.push(pol)
        eng.device_rollout(seed, first, n, period, packet.data_ptr())
    res = eng.fetch(n)
    return packet.cpu().numpy(), res


def _check(eng, pol, seed, first, n, mask=None, period=None, what=""):
    host, res = _packet_batch(eng, pol, seed, first, n, mask, period)
    ref, winner, same = _compare_packet(host, res, pol, what)
    assert host[8 * N.STATS_LEN + 8:8 * N.STATS_LEN + 16].view(np.int64)[0] == first + winner, (what, "candidate")
    return res, ref, same


# (n, replays, hoist, best list, stall, launch): every path of the one-wave kernels at least once — without replicas (1 025, 4 095),
# with them (4 096 and up), k_replay_solo (a long list without the hoist), the hoisted replay with and without replicas, forced contrast.
# (An all-replay batch runs under forced contrast: its episodes are one computation, which without it need not qualify.)
CASES = [
    (1025, "none", False, "short", 0, "mask"),
    (1025, "10th", False, "long", 900, "period"),
    (1025, "all", True, "short", 900, "period"),
    (4095, "10th", False, "short", 650, "mask"),
    (4095, "all", True, "long", 1500, "period"),
    (4096, "10th", False, "long", 0, "mask"),
    (4096, "10th", True, "short", 900, "period"),
    (4096, "none", False, "short", 1500, "period"),
    (4097, "all", False, "long", 900, "mask"),
    (4097, "10th", True, "long", 650, "mask"),
    (16384, "10th", False, "short", 0, "period"),
    (16384, "10th", False, "long", 900, "mask"),
    (16384, "10th", True, "long", 650, "period"),
    (16384, "all", True, "short", 1500, "mask"),
    (16384, "none", False, "short", 900, "mask"),
    (16384, "all", False, "long", 1500, "period"),
]


@pytest.mark.parametrize("n,replays,hoist,best,stall,launch", CASES)
def test_full_size_packet_equals_restatement(world, n, replays, hoist, best, stall, launch):
    eng = _engine(world, EIRGRID_REPLAY_HOIST="1" if hoist else "0")
    try:
        if best == "short":
            pol = _seeded(eng)
        else:      # ~230 generators per replay: beyond the short-replay variant, k_replay_solo's work without the hoist
            pol = _full_script(np.random.default_rng(n + stall), 9, [0, 4, 12, 7, 5, 1, 13, 2], offsets_per_year=1)
        forced = stall > 800
        if forced:      # an episode of a small batch as the best (the median; the worst when every episode replays the same list):
            pre = eng.rollout_batch(pol, 4242, 256)      # forced contrast then meets episodes that beat it (det < 0)
            ok = np.flatnonzero(pre.status == 0)
            scores = np.array([O.score_metrics(pre.metrics[e]) for e in ok])
            mid = int(ok[np.argsort(scores)[0 if replays == "all" else len(ok) // 2]])
            for k, v in zip(BEST, pre.metrics[mid]):
                pol.set(k, float(v))
        pol.set("iterations_without_improvement", stall)
        first, seed = 3 * n + 7, 20261 + n
        idx = first + np.arange(n)
        if replays == "none":
            mask, period = np.zeros(n, np.uint8), 0
        elif replays == "10th":
            mask, period = (idx % 10 == 0).astype(np.uint8), 10
        else:
            mask, period = np.ones(n, np.uint8), 1
        if launch == "mask":
            res, ref, same = _check(eng, pol, seed, first, n, mask=mask, what="mask")
        else:
            res, ref, same = _check(eng, pol, seed, first, n, period=period, what="period")
        # the batch reached what it claims to test
        assert (res.status == 0).all()
        rep = np.flatnonzero(mask)
        if replays != "none":
            assert len(rep) > 0
            assert all(res.metrics[rep[0]].tobytes() == res.metrics[e].tobytes() for e in rep), "replay episodes are one computation"
            if best == "long":
                assert res.n_gens[rep[0]] > 200, int(res.n_gens[rep[0]])
        armed, served = eng.replay_hoist_stats()
        if hoist and replays != "none":
            assert armed == 1 and served, (armed, served)
        else:
            assert armed == 0
        assert ref[2] > 0, "no episode qualified"
        beat = 0
        if forced:      # every successful episode qualifies, and some of them beat the best (det < 0: the kLnNanPenalty branch)
            ok = np.flatnonzero(res.status == 0)
            assert ref[2] == len(ok), (int(ref[2]), len(ok))
            s_best = _best_score(pol)
            beat = sum(O.score_metrics(res.metrics[e]) > s_best for e in ok)
            assert beat >= 1, "forced contrast never met a qualifying episode that beats the best"
        print(f"n {n} replays {replays} hoist {hoist} best {best} stall {stall} {launch}: qualifying {ref[2]}/{n}, beat the best {beat}, "
              f"Q32 sums identical in {same}/{2 * A}")
    finally:
        eng.close()


def test_replicas_start_clean_after_every_kind_of_call(world):
    """One engine, packet batches with and without the replicated statistics interleaved with a batch without statistics, a hoisted
    batch and a plan evaluation: every packet is the restatement's — nothing one batch added is found in the next one's."""
    eng = _engine(world)
    try:
        pol = _seeded(eng)
        pol.set("iterations_without_improvement", 900)      # forced contrast: every episode adds to the sums
        first = 0

        def mask(n):
            return ((first + np.arange(n)) % 10 == 0).astype(np.uint8)

        for step, n in enumerate((4096, 900)):
            _check(eng, pol, 100 + step, first, n, mask=mask(n), what=f"packet {n}")
            first += n
        plain = eng.rollout_batch(pol, 300, 16384, first_episode_index=first, replay_mask=mask(16384))
        assert (plain.status == 0).all()
        first += 16384
        eng.replay_hoist(True)
        _check(eng, pol, 400, first, 16384, mask=mask(16384), what="hoisted packet 16384")
        assert eng.replay_hoist_stats() == (1, True)
        eng.replay_hoist(False)
        first += 16384
        plans = [Plan.from_result(plain, e, f"episode {e}") for e in range(0, 3000, 10)]
        ev = eng.evaluate_plans(pol, plans, 500, first_episode_index=first)
        assert len(ev.status) == 300 and (ev.status == 0).all()
        first += 300
        for step, n in enumerate((5000, 4096)):
            _check(eng, pol, 600 + step, first, n, mask=mask(n), what=f"packet {n} after the plans")
            first += n
    finally:
        eng.close()


@pytest.mark.parametrize("hoist", [False, True])
def test_full_size_device_training_follows_the_restatement(world, hoist):
    """test_gpu_reduced_oracle.py::test_device_resident_training_follows_the_restatement at configs[2]'s size: 12 chained eg_device_step
    of 16 384 episodes, every 10th a replay, against the restatement's own chain fed with the device's records and never
    re-synchronised.  After every step lists, counters and best metrics are identical and every weight within 1e-9 relative: a Q32 unit
    is 2^-32 ~ 2.3e-10 of a logarithm, and across ~10^5 qualifying episodes some llrint will differ by one."""
    dev = _engine(world, EIRGRID_REPLAY_HOIST="1" if hoist else "0")
    try:
        pol = ActionWeights(); ow = O.OracleWeights()
        dev.push(pol)
        n, period, steps = 16384, 10, 12
        improvements = 0; max_stall = 0; worst = 0.0
        for step in range(steps):
            dev.device_step(8642, step * n, n, period, 100 + step)
            res = dev.fetch(n)
            assert (res.status == 0).all()
            improved, _, _ = O.reduced_batch_update(ow, *batch_arrays(res), noise_seed=100 + step)
            dev.pull(pol)
            for x, y in zip(pol.tables()[:2], ow.tables()[:2]):
                worst = max(worst, float(np.max(np.abs(x / y - 1.0))))
            assert_same_policy(pol, ow, 1e-9, f"step {step}")
            improvements += improved; max_stall = max(max_stall, int(ow.get("stall")))
        armed, _ = dev.replay_hoist_stats()
        assert armed == (steps if hoist else 0), armed
        assert improvements >= 2 and max_stall > 1200, (improvements, max_stall)
        print(f"hoist {hoist}: {steps} steps of {n}, {improvements} improvements, stall up to {max_stall}, "
              f"worst relative difference of a weight {worst:.2e}")
    finally:
        dev.close()
