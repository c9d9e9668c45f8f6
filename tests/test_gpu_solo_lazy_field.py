"""GPU: the lazy penalty field of the per-episode replay kernel (csrc/eg_replay_solo.h k_replay_lazy, csrc/eg_field.h tiles_refresh;
EIRGRID_SOLO_LAZY=0 switches it off: k_replay_solo).  With it a placement leaves the field alone, and a search by tiles brings the
64 values of every tile it is about to read up to date first: the generators the tile has not seen yet, in list order — the
multiplications the eager update performs, later.

Bar: every used record byte of every episode, n_chunks included, identical across the classic long-replay variant
(EIRGRID_REPLAY_SOLO=0), k_replay_solo with the eager field, with the lazy one at every script length (EIRGRID_SOLO_LAZY=all) and as
shipped (lazy for scripts of up to 384 generators); and the tabled oracle's records.
The scripts repeat entries of config 1's episode lists (seed 12345), the way a training loop's doubling does; every one completes
without a seeded draw, so nothing is left to the classic variant.  The shapes are the smallest at which catching up can go wrong: a
class away for a stretch of the list that starts and ends on and off a block of 64 generators, a wide class first searched when
nearly every generator reaches every tile, the edge tiles and a round's lone last tile, an absence across the end of the on-chip
window of the lists, and worlds where cells tie (the whole class caught up ahead of the rank scan)."""
import os

import numpy as np
import pytest

from eirgrid_amd.engine import ActionWeights, Engine, HostTables, Plan
from eirgrid_amd.world import World
from oracle import api as O
from tests.helpers import assert_episode_equal
from tests.test_gpu_parity import _ALL_FIELDS, _used
from tests.test_gpu_plans import _oracle_plan
from tests.test_gpu_replay_hoist import _seeded
from tests.test_gpu_solo_tiles import _replay_policy

pytestmark = pytest.mark.gpu

# action = 3 * generator type + size: the types the cases are built from (eirgrid_amd/world.py), all at the smallest size
OFFSHORE, DOMESTIC, COMMERCIAL, UTILITY, NUCLEAR, GAS_CC, BIOMASS, BATTERY, TIDAL, WAVE = (3 * t for t in (1, 2, 3, 4, 5, 7, 9, 12, 13, 14))
# (the default keeps the lazy field to scripts of up to 384 generators; "all": every script, so that every case below runs it)
_SETTINGS = {"classic": {"EIRGRID_REPLAY_SOLO": "0"}, "eager": {"EIRGRID_SOLO_LAZY": "0"}, "lazy": {"EIRGRID_SOLO_LAZY": "all"}, "default": {}}


def _engines(world):
    """{name: engine}, large-batch launch shape (as tests/test_gpu_solo_tiles.py::_engines): the classic long-replay variant only,
    k_replay_solo with the field kept current after every placement, k_replay_solo with the lazy field for scripts of any length,
    k_replay_solo as shipped (the lazy field up to 384 generators)"""
    engines = {}
    try:
        for name, env in _SETTINGS.items():
            os.environ["EIRGRID_HELPER_WAVES"] = "0"
            os.environ.update(env)
            try:
                engines[name] = Engine(world, device=0)
            finally:
                for k in ("EIRGRID_HELPER_WAVES", "EIRGRID_REPLAY_SOLO", "EIRGRID_SOLO_LAZY"):
                    os.environ.pop(k, None)
    except Exception:
        for eng in engines.values():
            eng.close()
        raise
    return engines


@pytest.fixture(scope="module")
def engines(world):
    e = _engines(world)
    yield e
    for eng in e.values():
        eng.close()


@pytest.fixture(scope="module")
def base_lists(oracle_world):
    """config 1's episode (seed 12345, index 0): its run and deficit lists per year.  The deficit list of the first year repairs it
    with eleven generators (a GasCombinedCycle, a UtilitySolar, a Biomass and seven BatteryStorage among them), then the run list
    of the year is applied entry by entry: a script's first year is those eleven placements followed by its own list."""
    st, ref = O.run_episode(oracle_world, O.OracleWeights(), 12345)
    assert st == 0
    return O.split_log(ref.run_log, ref.n_run), O.split_log(ref.def_log, ref.n_def)


def _script(base_lists, year0, name):
    """config 1's lists with `year0` as the first year's run list and fifty more BatteryStorage in the third year: the classes of the
    later years (PumpedStorage, CoalPlant, OnshoreWind, Nuclear, GasPeaker, Tidal, Offshore) join late, after a long list"""
    run, dfl = base_lists
    run = [list(year0)] + [list(l) for l in run[1:]]
    run[2] = run[2] + [BATTERY] * 50
    p = Plan(run, dfl, name)
    assert len(p) > 96, "a long plan: k_replay_solo's"
    return p


def _check(world, engines, plans, what, oracle_plans=4):
    pol = ActionWeights()
    assert len(plans) <= 64
    results = {name: eng.evaluate_plans(pol, plans, 41, 3000) for name, eng in engines.items()}
    for name, res in results.items():      # (nothing silently left to the classic variant)
        assert (res.status == 0).all(), (what, name, res.status.tolist())
        assert (res.n_draws == 0).all(), (what, name, res.n_draws.tolist())
    base = results["classic"]
    for name, res in results.items():
        for field in _ALL_FIELDS + ("n_chunks",):
            assert _used(base, field).tobytes() == _used(res, field).tobytes(), (what, name, field)
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    for j in np.linspace(0, len(plans) - 1, min(oracle_plans, len(plans))).astype(int):
        st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, plans[j]), 41 + 3000 + int(j), replay=True)
        assert st == 0 and ref.n_draws == 0
        assert_episode_equal(results["lazy"], int(j), ref, f"{what}, plan {j} ({plans[j].name})")
    return results["lazy"]


def test_long_absence(world, engines, base_lists):
    """GasCombinedCycle (8 km) searched eight times, then N BatteryStorage (3 km), then searched again: its tiles fold the N
    generators (and the eight of its own class) in one go.  The eight searches follow the 11 placements of the deficit list and
    `lead` BatteryStorage, so the tiles they leave hold 18 + lead generators: lead = 0 starts the pending range inside a block of
    64, lead = 46 on one; N = 63, 64, 65 and 130 end it on either side of the next boundaries, N = 45 and 109 (lead 0) on one."""
    plans = [_script(base_lists, [BATTERY] * lead + [GAS_CC] * 8 + [BATTERY] * n + [GAS_CC] * 2, f"lead {lead}, away {n}")
             for lead, n in ((0, 63), (0, 64), (0, 65), (0, 130), (46, 63), (46, 64), (46, 65), (46, 130), (0, 45), (0, 109), (46, 62), (46, 126))]
    res = _check(world, engines, plans, "long absence")
    for j, p in enumerate(plans):      # the script is what the docstring says it is
        lead, n = (int(x) for x in p.name.replace("lead ", "").replace(" away", "").split(","))
        types = (res.gen_pack[j, :res.n_gens[j]] & 15).tolist()
        assert types[11 + lead:11 + lead + 8] == [7] * 8 and types[19 + lead:19 + lead + n] == [12] * n and types[19 + lead + n] == 7, p.name


def test_cold_wide_class(world, engines, base_lists):
    """Nuclear (12 km: nearly every generator within reach of every tile) first searched after 150 and more placements of 3 km
    types: its first tiles start from 1.0 and fold the whole list, three blocks and more."""
    plans = [_script(base_lists, ([BATTERY, BIOMASS, UTILITY] * 90)[:n] + [NUCLEAR] * 3, f"{n} ahead of Nuclear") for n in (150, 181, 192, 245)]
    res = _check(world, engines, plans, "cold wide class")
    for j in range(len(plans)):
        types = (res.gen_pack[j, :res.n_gens[j]] & 15).tolist()
        assert types.index(5) >= 150


def test_edge_tiles(world, engines, base_lists):
    """Marine types (Offshore, Tidal, Wave: the coast — the grid's edge tiles, three cells wide, and few tiles with a positive bound,
    so that rounds end on a lone tile) interleaved with the solar types."""
    mix = [OFFSHORE, UTILITY, TIDAL, DOMESTIC, WAVE, COMMERCIAL]
    plans = [_script(base_lists, (mix * 40)[:n], f"marine and solar, {n}") for n in (90, 127, 150, 200)]
    plans += [_script(base_lists, [UTILITY] * 70 + [WAVE, TIDAL, OFFSHORE] * 10, "marine after solar"),
              _script(base_lists, [TIDAL] * 40 + [DOMESTIC] * 70 + [TIDAL] * 5, "tidal, solar, tidal")]
    _check(world, engines, plans, "edge tiles")


def test_absence_across_the_on_chip_window(world, engines, base_lists):
    """GasCombinedCycle away from before generator 512 (the end of the lists' window in LDS) until after it, in lists of about 600:
    the pending generators come from the window and from the record's tail; Nuclear joins beyond the window altogether."""
    plans = [_script(base_lists, [GAS_CC] * 4 + [BATTERY] * away + [GAS_CC] * 3 + [BATTERY] * 60 + [NUCLEAR, GAS_CC], f"away {away}")
             for away in (490, 497, 498, 560)]
    res = _check(world, engines, plans, "across the window", oracle_plans=4)
    assert res.n_gens.min() > 512


def _tie_world(kind):
    if kind == "symmetric":
        return World(np.array([25000.0]), np.array([25000.0]), np.array([400000], dtype=np.uint32), np.zeros(0), np.zeros(0),
                     np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0))
    return World(np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint32), np.zeros(0), np.zeros(0),
                 np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0))


@pytest.mark.parametrize("kind", ["symmetric", "flat"])
def test_where_cells_tie(kind):
    """The worlds of tests/test_gpu_solo_tiles.py::test_tile_search_where_cells_tie: up to eight cells share every score bit for bit
    (symmetric), every cell does (flat) — place_tiles returns kTilesUndecided, all 49 tiles of the class are caught up and
    place_heavy scans the field by rank; ties en masse and subnormal-small marine scores take the exact-scan fallbacks."""
    w = _tie_world(kind)
    rng = np.random.default_rng(23)
    engs = _engines(w)
    try:
        tb = O.OracleTables(HostTables(w), 0)
        for per_year, types in ((9, [0, 4, 12, 7, 8]), (20, [0, 4, 12, 7, 8, 1, 13])):
            pol = _replay_policy(rng, per_year, types)
            plan = Plan.from_policy(pol)
            plans = [plan] * 8
            results = {name: eng.evaluate_plans(pol, plans, 91, 0) for name, eng in engs.items()}
            for name, res in results.items():
                assert (res.status == 0).all() and (res.n_draws == 0).all(), (kind, name, res.status.tolist(), res.n_draws.tolist())
                assert res.n_gens.min() >= 200
                for field in _ALL_FIELDS + ("n_chunks",):
                    assert _used(results["classic"], field).tobytes() == _used(res, field).tobytes(), (kind, per_year, name, field)
            for j in (0, 3, 5, 7):
                st, ref = O.run_episode_tabled(tb, _oracle_plan(pol, plan), 91 + j, replay=True)
                assert_episode_equal(results["lazy"], j, ref, f"{kind} world, {per_year} a year")
    finally:
        for eng in engs.values():
            eng.close()


def test_switch(world, engines):
    """EIRGRID_SOLO_LAZY=0 is the eager kernel, =all the lazy one at any length: a 1 024-episode batch of configs[2]'s shape (every 10th episode a replay) from the
    seeded policy, and from the policies a loop's doubling grows out of it (every replay's recorded lists installed as the next
    best lists: 35, 66, 131, 262 generators), identical in all engines."""
    n = 1024
    mask = (np.arange(n) % 10 == 0).astype(np.uint8)
    reps = np.flatnonzero(mask)
    pol = _seeded(engines["lazy"])
    for step in range(4):
        results = {name: eng.rollout_batch(pol, 777, n, first_episode_index=5 * n, replay_mask=mask) for name, eng in engines.items()}
        res = results["lazy"]
        assert (res.status == 0).all() and (res.n_draws[reps] == 0).all()
        for name, other in results.items():
            for field in _ALL_FIELDS + ("n_chunks",):
                assert _used(results["classic"], field).tobytes() == _used(other, field).tobytes(), (step, name, field)
        e = int(reps[0])
        print(f"doubling {step}: {int(res.n_gens[e])} generators per replay episode, {int(res.n_chunks[e])} chunks requested")
        pol = ActionWeights()
        pol.apply_episode([-5e4, 0.7, 4e10, 1.0], res.n_run[e], res.run_log[e, :res.n_run[e].sum()], res.n_def[e], res.def_log[e, :res.n_def[e].sum()])
    assert res.n_gens[e] > 200
