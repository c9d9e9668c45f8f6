"""GPU: whole replays through the lazy field's staged catch-up (csrc/eg_field.h tiles_refresh), with scripts in which nearly every
search has a few generators to fold — tests/test_gpu_solo_lazy_field.py's scripts leave a class away for long stretches; here the
stretches are as short as the fold's pairs.

Bar (that file's, through its _check): every used record byte and n_chunks identical across the classic long-replay variant,
k_replay_solo with the eager field, k_replay_lazy at every script length and as shipped; status 0 and no draw for every plan, so
nothing is left to the classic variant; the sampled plans equal the tabled oracle."""
import pytest

from tests.test_gpu_solo_lazy_field import BATTERY, BIOMASS, GAS_CC, NUCLEAR, UTILITY, _check, _engines, _script, base_lists      # noqa: F401 (base_lists: a fixture)

pytestmark = pytest.mark.gpu

ONSHORE = 0      # action 3 * type + size: OnshoreWind, smallest size — the 5 km class


@pytest.fixture(scope="module")
def engines(world):
    e = _engines(world)
    yield e
    for eng in e.values():
        eng.close()


def test_three_classes_alternating(world, engines, base_lists):
    """BatteryStorage (3 km), GasCombinedCycle (8 km), OnshoreWind (5 km) in turn, every placement of another radius class than the one
    before: a search finds the two placements since its class's last one pending in the tiles it shares with that search, and more in
    the tiles it has not read for a while.  The lengths end the script on either side of a block of 64 generators; with UtilitySolar
    and Biomass (3 km both) two of three placements are of one class; a Nuclear (12 km) now and then reads tiles that hold next to
    nothing."""
    turn = [BATTERY, GAS_CC, ONSHORE]
    plans = [_script(base_lists, (turn * 70)[:n], f"three classes in turn, {n}") for n in (42, 53, 54, 117, 180)]
    plans += [_script(base_lists, ([UTILITY, GAS_CC, BIOMASS] * 70)[:n], f"two classes, three types in turn, {n}") for n in (43, 116)]
    plans += [_script(base_lists, ((turn * 9 + [NUCLEAR]) * 6)[:n], f"in turn with Nuclear, {n}") for n in (84, 140)]
    assert len(plans) <= 16
    res = _check(world, engines, plans, "three classes alternating")
    assert res.n_gens.min() > 96


def test_a_class_away_for_four_and_five_placements(world, engines, base_lists):
    """GasCombinedCycle away for exactly four and exactly five BatteryStorage, again and again: its tiles fold four or five pending
    generators (and the one of its own class) — two pairs, and two pairs and a half —; and the other way round."""
    plans = [_script(base_lists, ([GAS_CC] + [BATTERY] * 4 + [GAS_CC] + [BATTERY] * 5) * reps, f"away 4 and 5, {reps} times") for reps in (4, 10, 17)]
    plans += [_script(base_lists, ([BATTERY] + [GAS_CC] * 4 + [BATTERY] + [GAS_CC] * 5) * reps, f"the 3 km class away 4 and 5, {reps} times") for reps in (4, 9)]
    plans += [_script(base_lists, [GAS_CC] * 2 + ([BATTERY] * 4 + [GAS_CC]) * reps, f"away 4, {reps} times") for reps in (12, 25)]
    plans += [_script(base_lists, [GAS_CC] * 2 + ([BATTERY] * 5 + [GAS_CC]) * reps, f"away 5, {reps} times") for reps in (10, 21)]
    assert len(plans) <= 16
    res = _check(world, engines, plans, "a class away for 4 and 5")
    assert res.n_gens.min() > 96
