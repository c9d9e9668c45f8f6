"""The throughput kernels with the episode's control state uniform (csrc/eg_rollout_episode.h under k_episodes<kind>: the lean and the
short-replay kind) against the kernels they replace (EIRGRID_UNIFORM=0: k_rollout<0, kind>) and the oracle.  The new kernels say of
values that are the same in every lane that they are — the result of weighted_pick —; a value that was NOT the same in every lane
would show as an episode that differs from the oracle's, so every sampler and the code behind it runs here: the weighted picks of the
action, the deficit action and the year's count; the heuristic count (rng_range32); the exploring branches (rng_range64); the stalled
sampler with the table rebuild behind a repair nudge; the short-replay kernel; and a batch whose replays are long ones on
k_replay_lazy (EIRGRID_SOLO_LAZY=all) beside the lean grid.

64 episodes on the one-wave kernels (EIRGRID_HELPER_WAVES=0), two engines: the default one and one with the switch off.
Bar: every record of both engines equals the tabled oracle's, bitwise (tests/helpers.py assert_episode_equal) — the two engines
therefore equal each other.  The seeds are ones for which the oracle alone ends all 64 episodes with status 0 (checked without a GPU by
test_the_oracle_completes_every_episode, and asserted again where the records are compared).  No episode is left out."""
import os

import numpy as np
import pytest

from eirgrid_amd.engine import ActionWeights, Engine, HostTables
from oracle import api as O
from tests.helpers import assert_episode_equal, oracle_weights_like

N_EPISODES = 64
FIRST = 5000
MASK = (np.arange(N_EPISODES) % 4 == 0).astype(np.uint8)
# policy -> seed (see the module docstring)
SEEDS = {"fresh": 777, "heuristic count": 778, "exploring": 779, "stalled": 780, "short replay": 777, "long replay": 777}
REPLAYS = ("short replay", "long replay")


def _installed(ep):
    """a fresh policy with the oracle episode's recorded lists as its best lists (the reference's sequential update, as
    tests/test_gpu_factor_planes.py installs a kernel's record)"""
    pol = ActionWeights()
    pol.apply_episode([-5e4, 0.7, 4e10, 1.0], np.array(ep.n_run), np.array(ep.run_log[:sum(ep.n_run)], dtype=np.uint8),
                      np.array(ep.n_def), np.array(ep.def_log[:sum(ep.n_def)], dtype=np.uint8))
    return pol


def _policy(name, tb):
    pol = ActionWeights()
    if name == "heuristic count":      # the year's action count from the heuristic range: rng_range32
        pol.set("has_count_weights", 0)
    elif name == "exploring":          # both samplers take their uniform draw nearly every time: rng_range64
        pol.set("exploration_rate", 0.97)
    elif name == "stalled":            # the sorted, powered table; rebuilt in a year whose repair actions nudged the row
        pol.set("iterations_without_improvement", 600)
    elif name in REPLAYS:
        # the short list: a sampled episode's record; the long one: a replay's record installed as the next best lists, three times
        # over (a replay records every action twice)
        _, ep = O.run_episode_tabled(tb, oracle_weights_like(pol), 12345, replay=False)
        assert ep.status == 0
        pol = _installed(ep)
        for _ in range(3 if name == "long replay" else 0):
            _, ep = O.run_episode_tabled(tb, oracle_weights_like(pol), 777 + 4096, replay=True)
            assert ep.status == 0
            pol = _installed(ep)
        n_actions = sum(len(l) for l in pol.lists(0))
        assert (n_actions > 96) == (name == "long replay"), n_actions
    return pol


@pytest.fixture(scope="module")
def tabled(world):
    return O.OracleTables(HostTables(world), len(world.existing_x))


@pytest.fixture(scope="module")
def references(tabled):
    """{policy: (the policy, the oracle's 64 episodes)}, computed once and left alone"""
    out = {}
    for name, seed in SEEDS.items():
        pol = _policy(name, tabled)
        replay = name in REPLAYS
        # (an episode nudges the weights it is given, as the reference's does: every episode starts from a copy of the batch's policy)
        out[name] = (pol, [O.run_episode_tabled(tabled, oracle_weights_like(pol), seed + FIRST + e, replay=replay and bool(MASK[e]))[1]
                           for e in range(N_EPISODES)])
    return out


@pytest.mark.parametrize("name", list(SEEDS))
def test_the_oracle_completes_every_episode(references, name):
    """CPU: the seeds are ones where nothing ends early, and each policy does run what it is here for."""
    pol, refs = references[name]
    assert [r.status for r in refs] == [0] * N_EPISODES
    if name == "stalled":      # a year with repair actions: the nudge that invalidates the stalled sampler's table
        assert any(sum(r.n_def) > 0 for r in refs)
    if name == "heuristic count":
        assert pol.get("has_count_weights") == 0


def _engine(world, uniform, lazy):
    env = {"EIRGRID_HELPER_WAVES": "0", "EIRGRID_UNIFORM": uniform}
    if lazy:
        env["EIRGRID_SOLO_LAZY"] = "all"
    os.environ.update(env)
    try:
        return Engine(world, device=0)
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def engines(world):
    made = {}
    try:
        for lazy in (False, True):
            for uniform in ("1", "0"):
                made[uniform == "1", lazy] = _engine(world, uniform, lazy)
        yield made
    finally:
        for eng in made.values():
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEEDS))
def test_both_kernel_families_equal_the_oracle(engines, references, name):
    pol, refs = references[name]
    replay = name in REPLAYS
    assert [r.status for r in refs] == [0] * N_EPISODES
    for uniform in (True, False):
        eng = engines[uniform, name == "long replay"]
        res = eng.rollout_batch(pol, SEEDS[name], N_EPISODES, first_episode_index=FIRST, replay_mask=MASK if replay else None)
        assert (res.status == 0).all(), (name, uniform, res.status.tolist())
        for e in range(N_EPISODES):
            assert_episode_equal(res, e, refs[e], f"{name}, {'k_episodes' if uniform else 'k_rollout'}, {'replay' if replay and MASK[e] else 'sampled'}")
