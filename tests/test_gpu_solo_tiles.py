"""GPU: the tile search of the per-episode replay kernel (csrc/eg_field.h place_tiles: the penalty field bounded per 8 x 8 tile
instead of scanned by rank) against the rank scan it stands in for (place_heavy, EIRGRID_SOLO_TILES=0) and against the classic
long-replay variant (EIRGRID_REPLAY_SOLO=0).

Bar: every used record byte of every episode, n_chunks included — the tile search derives the chunks the rank scan would have
requested from the M it finds —, in the states the benchmark measures (the grown-replay state of configs[2], and the state an
eight-GPU run of the loop reaches), and in worlds where many cells tie: the symmetric world (eight-way ties) and a world without
settlements, plant or coast, where every cell of a non-marine type has the same score and every marine score is subnormal-small."""
import os

import numpy as np
import pytest
import torch

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, Engine
from eirgrid_amd.parallel import BatchTrainer
from eirgrid_amd.world import World
from tests.test_gpu_parity import _ALL_FIELDS, _used

pytestmark = pytest.mark.gpu


def _engines(world):
    """{name: engine}: the classic long-replay variant only, k_replay_solo searching by rank, k_replay_solo searching by tiles
    (large-batch launch shape: the small-batch kernel has no per-episode replay kernel)"""
    settings = {"classic": {"EIRGRID_REPLAY_SOLO": "0"}, "rank": {"EIRGRID_SOLO_TILES": "0"}, "tiles": {"EIRGRID_SOLO_TILES": "1"}}
    engines = {}
    try:
        for name, env in settings.items():
            os.environ["EIRGRID_HELPER_WAVES"] = "0"
            os.environ.update(env)
            try:
                engines[name] = Engine(world, device=0)
            finally:
                for k in ("EIRGRID_HELPER_WAVES", "EIRGRID_REPLAY_SOLO", "EIRGRID_SOLO_TILES"):
                    os.environ.pop(k, None)
    except Exception:
        for eng in engines.values():
            eng.close()
        raise
    return engines


def _all_same(results, what):
    base = results["classic"]
    for name, res in results.items():
        for field in _ALL_FIELDS + ("n_chunks",):
            assert _used(base, field).tobytes() == _used(res, field).tobytes(), (what, name, field)


def _grown(eng, shards, batches=48, n=16384, seed=12345, period=10):
    """bench.py's grown-replay state: config 1's episode as the best strategy, then `batches` updates of the device-resident loop from
    there (replay hoist on: the same policies in a fraction of the time), each from `shards` packets of n episodes — shards = 8 is the
    state an eight-GPU run reaches (one k_apply_update over eight packets, as tests/test_gpu_rehearsals.py runs it)"""
    w = ActionWeights()
    first = eng.run_iteration(0, w, False, seed)
    w.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0], first.def_log[0, :first.n_def[0].sum()])
    eng.replay_hoist(True)
    try:
        if shards == 1:
            tr = BatchTrainer(eng, w, n, seed, 0, 1, None, replay_fraction=1.0 / period, device_resident=True)
            for _ in range(batches):
                tr.step()
            tr.sync()
        else:
            eng.push(w)
            PB, nstat = N.PACKET_BYTES, 8 * N.STATS_LEN
            packets = torch.zeros(shards * PB, dtype=torch.uint8, device="cuda")
            for step in range(batches):
                for r in range(shards):
                    eng.device_rollout(seed, (step * shards + r) * n, n, period, packets.data_ptr() + r * PB)
                eng.device_apply(packets.data_ptr(), shards, packets.data_ptr(), seed + step)
                for r in range(1, shards):
                    packets[r * PB:r * PB + nstat] = 0
            eng.pull(w)
    finally:
        eng.replay_hoist(False)
    return w


@pytest.mark.parametrize("shards", [1, 8])
def test_tile_search_is_the_rank_search_in_the_grown_states(world, shards):
    """A whole configs[2] batch (16 384 episodes, every 10th a replay) from the grown-replay state of one GPU and of eight: every search
    of every replay episode, through the records and n_chunks they leave, identical across the three engines."""
    engines = _engines(world)
    try:
        pol = _grown(engines["tiles"], shards)
        n = 16384
        mask = (np.arange(n) % 10 == 0).astype(np.uint8)
        results = {name: eng.rollout_batch(pol, 777, n, first_episode_index=5 * n, replay_mask=mask) for name, eng in engines.items()}
        reps = np.flatnonzero(mask)
        res = results["tiles"]
        assert (res.status[reps] == 0).all(), np.unique(res.status[reps])
        assert res.n_gens[reps].min() > 96, "the replays run the long-replay kernels"
        _all_same(results, f"{shards} shards")
        print(f"{shards} shard(s): {int(res.n_gens[reps].mean())} generators per replay episode, "
              f"{int(res.n_chunks[reps].mean())} chunks requested per replay episode")
    finally:
        for eng in engines.values():
            eng.close()


def _replay_policy(rng, per_year, types):
    pol = ActionWeights()
    run = [[int(3 * rng.choice(types) + rng.integers(0, 3)) for _ in range(per_year)] for _ in range(26)]
    dfl = [[int(3 * rng.choice([8, 7, 12, 0])) for _ in range(4)] for _ in range(26)]      # (four a year: the repair loop never runs out of them)
    pol.apply_episode([-5e4, 0.7, 4e10, 1.0], np.array([len(l) for l in run], np.int32), np.array([a for l in run for a in l], np.uint8),
                      np.full(26, 4, np.int32), np.array([a for l in dfl for a in l], np.uint8))
    return pol


@pytest.mark.parametrize("kind", ["symmetric", "flat"])
def test_tile_search_where_cells_tie(kind):
    """symmetric: one settlement in the middle of the map, no plant, no coast — up to eight cells share every score bit for bit, so
    searches meet several candidates within 2^-30 of M (place_tiles hands the ones that would share a lane of the rank scan to it).
    flat: no settlement, no plant, no coast — every cell has the same unpenalised score for the non-marine types (ties en masse: the
    exact scan decides) and a subnormal-small one for the marine types (the fallback below 1e-250)."""
    if kind == "symmetric":
        w = World(np.array([25000.0]), np.array([25000.0]), np.array([400000], dtype=np.uint32), np.zeros(0), np.zeros(0),
                  np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0))
    else:
        w = World(np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint32), np.zeros(0), np.zeros(0),
                  np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0))
    rng = np.random.default_rng(23)
    engines = _engines(w)
    try:
        for per_year, types in ((9, [0, 4, 12, 7, 8]), (20, [0, 4, 12, 7, 8, 1, 13])):
            pol = _replay_policy(rng, per_year, types)
            n = 24
            mask = (np.arange(n) % 3 != 2).astype(np.uint8)
            results = {name: eng.rollout_batch(pol, 91, n, replay_mask=mask) for name, eng in engines.items()}
            reps = np.flatnonzero(mask)
            assert results["classic"].n_gens[reps].min() >= 200
            _all_same(results, f"{kind} world, {per_year} a year")
    finally:
        for eng in engines.values():
            eng.close()
