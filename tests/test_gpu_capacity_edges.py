"""Episodes at the capacities the per-episode kernels have and the oracle does not (csrc/eg_rollout_episode.h, csrc/eg_replay_script.h).

The on-chip window: EG_ONCHIP_GENS = 512 generators and 512 carbon offsets per sampled episode (kGenCap / kOffCap).  A year adds up to 20
actions, so a policy that puts its weight on one kind of action places 506-520 of them: the eighth staging block, the padding behind the
lists, year_gather at base + 64 >= 512, the prefix cache across 500 searches of one class and the >= kGenCap / >= kOffCap exits all run.
A year's repair list: 128 deficit actions in sm.ydef[0..127], the stalled sampler's permutation directly behind it.  A world of six times
the standard demand repairs 61-67 times in 2025 (the second register of the success bonus), twelve times 124-131 (the list full, and
the n_def_y >= 128 exits).

The bar.  The oracle has neither capacity, so its record says what an episode needs.  An episode whose oracle record stays within the
capacities (n_gens <= 512, n_offsets <= 512, every year's n_def <= 128 — the ones that fill a list exactly included) equals the oracle
bitwise (tests/helpers.py assert_episode_equal).  Every other episode ends with EG_EP_OVERFLOW, the list that overflowed stopped at its
capacity, what the episode did before is the oracle's — the placement lists are prefixes of the oracle's, the years before the one that
overflows are the oracle's counts, logs and yearly rows bit for bit —, and the kernel families agree byte for byte on the scalar fields
tests/test_gpu_parity.py::test_capacity_overflow_is_reported_not_hidden compares.  No episode is left out: each is judged one way or the
other, in k_episodes<lean> (EIRGRID_HELPER_WAVES=0), k_rollout<0, lean> (EIRGRID_UNIFORM=0 as well) and the two-wave kernel
(EIRGRID_HELPER_WAVES=all); replays of such lists in the large-batch launch shape (EIRGRID_HELPER_WAVES=0) with the hoist armed, on
k_replay_lazy, on k_replay_solo with the eager field and on the classic long-replay variant k_rollout<0, long replay>, and on the two-wave
kernel; and the batch update's statistics behind a batch most of whose episodes failed.

64 episodes per input.  test_the_oracle_puts_the_inputs_at_the_capacities checks without a GPU that the oracle alone ends every episode
with status 0 and that every class — below a capacity, at it, above it — holds at least three of them; the GPU tests judge by the same
records.  The records of an engine are not cleared between batches: lists are compared up to their lengths, yearly rows for the years
named, and between engines the counts of a year an episode did not finish (its overflow year and the years behind it hold whatever an
earlier batch left) are left out of the byte comparison."""
import dataclasses
import os

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd import synthetic_world
from eirgrid_amd.engine import ActionWeights, Engine, HostTables
from oracle import api as O
from tests.helpers import assert_episode_equal, oracle_weights_like
from tests.test_gpu_reduced_oracle import batch_arrays
from tests.test_gpu_uniform_kernels import _installed

N_EPISODES = 64
WINDOW = N.ONCHIP_GENS      # kGenCap / kOffCap of the lean and the short-replay kernels
YEAR_REPAIRS = 128          # sm.ydef[0..127]
MASK = (np.arange(N_EPISODES) % 4 == 0).astype(np.uint8)
SCALAR_FIELDS = ("status", "metrics", "n_run", "n_def", "n_act", "n_gens", "n_offsets", "n_draws")

# name -> (world, the columns of the action table that carry the weight, iterations_without_improvement); oracle seeds 7000 + e
CROWDED = {"all generator types": ("standard", range(45), 0),
           "one type": ("standard", [0, 1, 2], 0),
           "battery": ("standard", [36, 37, 38], 0),
           "all generator types, stalled": ("standard", range(45), 900),
           "offsets": ("light", range(45, 57), 0),
           "offsets, plant operational": ("light operational", range(45, 57), 0)}
CROWDED_SEED = 7000
# name -> (world, iterations_without_improvement): the default policy on k times the demand; oracle seeds 400 + e
REPAIRS = {f"demand x{k}{', stalled' if stall else ''}": (f"x{k}", stall) for k in (6, 10, 12) for stall in (0, 900)}
REPAIR_SEED = 400
# the batch behind the update test: the crowded all-types policy, stalled, with best lists (a default episode's record) to contrast with
UPDATE_CROWDED = "all generator types, stalled, best lists"
# name -> world: episode 400's record installed as the best lists, every fourth episode a replay; oracle seeds 400 + 9000 + e
REPLAYS = {"replay x6": "x6", "replay x12": "x12"}
REPLAY_FIRST = 9000

SAMPLED_KERNELS = {"k_episodes": {"EIRGRID_HELPER_WAVES": "0"},
                   "k_rollout": {"EIRGRID_HELPER_WAVES": "0", "EIRGRID_UNIFORM": "0"},
                   "two-wave": {"EIRGRID_HELPER_WAVES": "all"}}
# A batch of up to 4 x CUs episodes goes to the two-wave kernel whatever else is set (csrc/eg_api.cpp launch_batch: plan.helper_waves), and
# the per-episode replay kernels are armed only without it: the one-wave routes need EIRGRID_HELPER_WAVES=0, as in every other test of
# them.  With the hoist armed no solo kernel is: a script it leaves goes to the classic variant k_rollout<0, long replay>.
REPLAY_ROUTES = {"hoist": {"EIRGRID_HELPER_WAVES": "0"},
                 "k_replay_lazy": {"EIRGRID_HELPER_WAVES": "0", "EIRGRID_SOLO_LAZY": "all"},
                 "k_replay_solo": {"EIRGRID_HELPER_WAVES": "0", "EIRGRID_SOLO_LAZY": "0"},
                 "classic": {"EIRGRID_HELPER_WAVES": "0", "EIRGRID_REPLAY_SOLO": "0"},
                 "two-wave": {"EIRGRID_HELPER_WAVES": "all"}}


def _world(name):
    w = synthetic_world(existing_operational_at_start=name.endswith("operational"))
    if name.startswith("light"):      # a twentieth of the demand: the repairs leave the years' 20 actions to the offsets
        return dataclasses.replace(w, settlement_pop=np.maximum(w.settlement_pop // 20, 1).astype(np.uint32))
    if name.startswith("x"):
        return dataclasses.replace(w, settlement_pop=(w.settlement_pop * int(name[1:])).astype(np.uint32))
    return w


def crowd(cols, stall=0):
    """a policy whose action weight lies on `cols` and which takes 20 actions in every year but the last (13-20 there)"""
    pol = ActionWeights()
    w, dw, cw = pol.tables()
    w[:] = 1e-4; w[:, list(cols)] = 0.999
    cw[:] = 1e-9; cw[:, 20] = 1.0
    cw[25, :] = 1e-9; cw[25, 8:21] = 1.0
    pol.set_tables(w, dw, cw)
    pol.set("exploration_rate", 0)
    pol.set("iterations_without_improvement", stall)
    return pol


def _stalled(stall):
    pol = ActionWeights()
    pol.set("iterations_without_improvement", stall)
    return pol


class _References:
    """{input: (the policy, its batch arguments, the oracle's 64 episodes)}, each computed once, on first use, and left alone"""

    def __init__(self):
        self.worlds, self.tables, self.made = {}, {}, {}

    def world(self, name):
        if name not in self.worlds:
            self.worlds[name] = _world(name)
            self.tables[name] = O.OracleTables(HostTables(self.worlds[name]), len(self.worlds[name].existing_x))
        return self.worlds[name]

    def world_of(self, name):
        return CROWDED[name][0] if name in CROWDED else REPAIRS[name][0] if name in REPAIRS else REPLAYS[name] if name in REPLAYS else "standard"

    def __call__(self, name):
        if name in self.made:
            return self.made[name]
        self.world(self.world_of(name))
        tb = self.tables[self.world_of(name)]
        if name in CROWDED:
            pol, args = crowd(*CROWDED[name][1:]), dict(seed=CROWDED_SEED, first_episode_index=0, replay_mask=None)
        elif name == UPDATE_CROWDED:
            # (the best lists and what installing them did to the scalars come first; the tables and the stall of the crowded policy after)
            st, first = O.run_episode_tabled(tb, oracle_weights_like(ActionWeights()), 12345, replay=False)
            assert st == 0
            pol = _installed(first)
            w, dw, cw = crowd(range(45), 900).tables()
            pol.set_tables(w, dw, cw)
            pol.set("exploration_rate", 0)
            pol.set("iterations_without_improvement", 900)
            args = dict(seed=CROWDED_SEED, first_episode_index=0, replay_mask=None)
        elif name in REPAIRS:
            pol, args = _stalled(REPAIRS[name][1]), dict(seed=REPAIR_SEED, first_episode_index=0, replay_mask=None)
        else:
            first = self(f"demand {REPLAYS[name]}")[2][0]      # seed 400's record
            assert first.status == 0
            pol, args = _installed(first), dict(seed=REPAIR_SEED, first_episode_index=REPLAY_FIRST, replay_mask=MASK)
        # (an episode nudges the weights it is given, as the reference's does: every episode starts from a copy of the batch's policy)
        refs = [O.run_episode_tabled(tb, oracle_weights_like(pol), args["seed"] + args["first_episode_index"] + e,
                                     replay=args["replay_mask"] is not None and bool(MASK[e]))[1] for e in range(N_EPISODES)]
        self.made[name] = (pol, args, refs)
        return self.made[name]


@pytest.fixture(scope="module")
def references(built):
    return _References()


def _classes(values, cap):
    v = np.asarray(values)
    return int((v < cap).sum()), int((v == cap).sum()), int((v > cap).sum())


@pytest.mark.parametrize("name", list(CROWDED) + list(REPAIRS) + list(REPLAYS) + [UPDATE_CROWDED])
def test_the_oracle_puts_the_inputs_at_the_capacities(references, name):
    """CPU: the oracle alone ends all 64 episodes with status 0, and every class the GPU tests are here for holds at least three."""
    pol, args, refs = references(name)
    assert [r.status for r in refs] == [0] * N_EPISODES
    gens = np.array([r.n_gens for r in refs]); offs = np.array([r.n_offsets for r in refs])
    worst = np.array([max(r.n_def) for r in refs])      # the year's largest repair list
    if name in CROWDED or name == UPDATE_CROWDED:
        w, dw, cw = pol.tables()
        cols = list(CROWDED[name][1]) if name in CROWDED else list(range(45))
        assert (w[:, cols] == 0.999).all() and w.min() == 1e-4 and cw[3, 20] == 1.0 and cw[25, 7] == 1e-9, "set_tables keeps the values"
        if name == UPDATE_CROWDED:
            assert pol.get("has_best") == 1 and sum(map(len, pol.lists(0))) > 0 and pol.get("iterations_without_improvement") == 900
        lists = offs if cols[0] >= 45 else gens
        below, at, above = _classes(lists, WINDOW)
        print(f"{name}: {'offsets' if cols[0] >= 45 else 'generators'} <= 511: {below}, = 512: {at}, > 512: {above}, range {lists.min()}-{lists.max()}; "
              f"the other list {(gens if cols[0] >= 45 else offs).min()}-{(gens if cols[0] >= 45 else offs).max()}, repairs a year up to {worst.max()}")
        assert min(below, at, above) >= 3
        assert lists.max() <= WINDOW + 8, "a year adds 20 actions at the most"
        if cols[0] < 45:
            assert gens.min() >= 449, "every episode's last searches walk the eighth block of 64"
            assert offs.max() < WINDOW
        else:
            assert gens.max() < WINDOW
    elif name in REPAIRS:
        k = int(REPAIRS[name][0][1:])
        assert all(int(np.argmax(r.n_def)) == 0 for r in refs), "the largest repair list of an episode is 2025's"
        print(f"{name}: repairs in 2025 {worst.min()}-{worst.max()}: <= 64: {(worst <= 64).sum()}, 65-127: {((worst > 64) & (worst < 128)).sum()}, "
              f"= 128: {(worst == 128).sum()}, > 128: {(worst > 128).sum()}; generators {gens.min()}-{gens.max()}")
        assert gens.max() < WINDOW and offs.max() < WINDOW
        if k == 6:      # both sides of the 64 entries a register holds
            assert (worst <= 64).sum() >= 3 and ((worst > 64) & (worst < 128)).sum() >= 3
        elif k == 10:
            assert ((worst > 64) & (worst < 128)).all()
        else:
            assert min(_classes(worst, YEAR_REPAIRS)) >= 3
    else:
        k = int(REPLAYS[name][1:])
        lists, dlists = pol.lists(0), pol.lists(1)
        reps = [refs[e] for e in np.flatnonzero(MASK)]
        print(f"{name}: installed list {sum(map(len, lists))} actions, {len(dlists[0])} deficit entries in 2025; the replay: {reps[0].n_gens} generators, "
              f"{reps[0].n_def[0]} repairs in 2025, draws {sorted({int(r.n_draws) for r in reps})}; sampled episodes: repairs in 2025 "
              f"{min(refs[e].n_def[0] for e in range(N_EPISODES) if not MASK[e])}-{max(refs[e].n_def[0] for e in range(N_EPISODES) if not MASK[e])}")
        assert sum(map(len, lists)) > 96, "a long replay"
        assert all(r.n_gens > WINDOW // 4 for r in reps)
        if k == 6:      # past the 64 entries of the list a register keeps, within the year's 128
            assert len(dlists[0]) > 64 and all(64 < r.n_def[0] <= YEAR_REPAIRS and max(r.n_def) <= YEAR_REPAIRS for r in reps)
            assert all(r.n_draws == 0 for r in reps), "the script needs no fallback draw"
        else:           # a full list installed; the replay records every repair it applies twice and passes the 128
            assert len(dlists[0]) == YEAR_REPAIRS and all(r.n_def[0] > YEAR_REPAIRS for r in reps)


# ---- judging a device record by the oracle's ----

def _overflow_year(ref):
    """the year index in which the oracle's episode passes a capacity of the per-episode kernels; None: it stays within them"""
    years = [y for y in range(N.YEARS) if ref.n_def[y] > YEAR_REPAIRS][:1]
    if ref.n_gens > WINDOW:
        years.append(int(ref.gen_year[WINDOW]))
    if ref.n_offsets > WINDOW:
        years.append(int(ref.off_year[WINDOW]))
    return min(years) if years else None


def _assert_overflow(res, e, ref, what):
    """an episode beyond a capacity: reported, stopped at the capacity, and the oracle's up to there"""
    tag = f"{what} episode {e}"
    year = _overflow_year(ref)
    assert res.status[e] == N.EG_EP_OVERFLOW, f"{tag}: status {res.status[e]}, the oracle needs {ref.n_gens} generators, {ref.n_offsets} offsets, {max(ref.n_def)} repairs in a year"
    ng, no = int(res.n_gens[e]), int(res.n_offsets[e])
    assert 0 <= ng <= min(ref.n_gens, WINDOW) and 0 <= no <= min(ref.n_offsets, WINDOW), f"{tag}: {ng} generators, {no} offsets"
    if max(ref.n_def) <= YEAR_REPAIRS:      # the list that overflowed has stopped at the capacity
        stopped = [n for n, needs in ((ng, ref.n_gens), (no, ref.n_offsets)) if needs > WINDOW]
        assert WINDOW in stopped, f"{tag}: {ng} generators, {no} offsets"
    assert res.gen_cell[e, :ng].tolist() == list(ref.gen_cell[:ng]), f"{tag}: placement cells differ"
    assert res.gen_pack[e, :ng].tolist() == [t | (y << 4) | (m << 9) for t, y, m in zip(ref.gen_type[:ng], ref.gen_year[:ng], ref.gen_mult[:ng])], tag
    assert res.off_pack[e, :no].tolist() == [t | (y << 4) | (m << 9) for t, y, m in zip(ref.off_type[:no], ref.off_year[:no], ref.off_mult[:no])], tag
    # the years before: counts, logs and yearly rows
    for which, cnt, log in (("n_run", ref.n_run, ref.run_log), ("n_def", ref.n_def, ref.def_log), ("n_act", ref.n_act, ref.act_log)):
        assert getattr(res, which)[e, :year].tolist() == list(cnt[:year]), f"{tag}: {which} of the years before {2025 + year}"
        n = sum(cnt[:year])
        assert getattr(res, which[2:] + "_log")[e, :n].tolist() == list(log[:n]), f"{tag}: {which[2:]} log of the years before {2025 + year}"
    assert np.array(ref.yearly)[:year].tobytes() == res.yearly[e, :year].tobytes(), f"{tag}: yearly rows before {2025 + year}"
    # what the year itself recorded before it stopped is the oracle's as well (the placements of the year are a prefix: above).  A year's
    # repair list that overflows has taken its 128 entries first: every exit checks n_def_y >= 128 in front of the store it guards
    if ref.n_def[year] > YEAR_REPAIRS:
        base = sum(ref.n_def[:year])
        assert res.def_log[e, base:base + YEAR_REPAIRS].tolist() == list(ref.def_log[base:base + YEAR_REPAIRS]), f"{tag}: the 128 deficit actions of {2025 + year}"
    assert ng >= sum(1 for y in ref.gen_year[:ref.n_gens] if y < year) and no >= sum(1 for y in ref.off_year[:ref.n_offsets] if y < year), tag


def _judge(results, refs, name, replay_mask=None):
    """every episode of every engine's batch, one way or the other; then the engines against each other.  Returns (bitwise, overflow)."""
    counts = [0, 0]
    for kernel, res in results.items():
        for e in range(N_EPISODES):
            what = f"{name}, {kernel}, {'replay' if replay_mask is not None and replay_mask[e] else 'sampled'}"
            if _overflow_year(refs[e]) is None:
                assert_episode_equal(res, e, refs[e], what)
            else:
                _assert_overflow(res, e, refs[e], what)
            counts[_overflow_year(refs[e]) is not None] += 1
    # a year's counts are stored when the year ends: rows from the overflow year on were not written by this batch
    finished = np.array([[_overflow_year(r) is None or y < _overflow_year(r) for y in range(N.YEARS)] for r in refs])
    first = next(iter(results))
    for kernel, res in results.items():
        for field in SCALAR_FIELDS:
            a, b = getattr(results[first], field), getattr(res, field)
            if field in ("n_run", "n_def", "n_act"):
                a, b = np.where(finished, a, 0), np.where(finished, b, 0)
            assert a.tobytes() == b.tobytes(), f"{name}: {field} of {first} and {kernel}"
    return counts[0] // len(results), counts[1] // len(results)


# ---- engines: one world's at a time (three sampled kernels, five replay routes: eight at the most) ----

def _engine(world, env):
    os.environ.update(env)
    try:
        return Engine(world, device=0)
    finally:
        for k in env:
            os.environ.pop(k, None)


class _Engines:
    def __init__(self, references):
        self.references, self.world_name, self.made = references, None, {}

    def close(self):
        for eng in self.made.values():
            eng.close()
        self.made = {}

    def __call__(self, world_name, kinds):
        """{kind: engine} on that world, kinds = SAMPLED_KERNELS or REPLAY_ROUTES; another world's engines are closed first"""
        if world_name != self.world_name:
            self.close()
            self.world_name = world_name
        world = self.references.world(world_name)
        routes = kinds is REPLAY_ROUTES
        for kind, env in kinds.items():
            if (routes, kind) not in self.made:
                self.made[routes, kind] = _engine(world, env)
                if routes and kind == "hoist":
                    self.made[routes, kind].replay_hoist(True)
        return {kind: self.made[routes, kind] for kind in kinds}


@pytest.fixture(scope="module")
def engines(references):
    made = _Engines(references)
    try:
        yield made
    finally:
        made.close()


def _run(engine_set, pol, args):
    return {kind: eng.rollout_batch(pol, args["seed"], N_EPISODES, first_episode_index=args["first_episode_index"], replay_mask=args["replay_mask"])
            for kind, eng in engine_set.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CROWDED))
def test_sampled_episodes_at_the_onchip_window(engines, references, name):
    """506-520 generators or offsets per episode: up to and including 512 the oracle's bits, beyond it EG_EP_OVERFLOW with the list
    stopped at 512 and everything before it the oracle's, in the three sampled kernels."""
    pol, args, refs = references(name)
    assert [r.status for r in refs] == [0] * N_EPISODES
    lists = [r.n_offsets if "offsets" in name else r.n_gens for r in refs]
    assert min(_classes(lists, WINDOW)) >= 3
    bitwise, overflow = _judge(_run(engines(CROWDED[name][0], SAMPLED_KERNELS), pol, args), refs, name)
    print(f"{name}: {bitwise} episodes bitwise, {overflow} EG_EP_OVERFLOW")
    assert bitwise == sum(1 for n in lists if n <= WINDOW) and overflow == N_EPISODES - bitwise


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REPAIRS))
def test_sampled_episodes_at_a_years_repair_list(engines, references, name):
    """61-67, 103-109 and 124-131 repairs in 2025, with the stalled sampler's permutation behind the list and without: up to and including
    128 the oracle's bits — the success bonus over both registers of the list —, beyond it EG_EP_OVERFLOW in the three sampled kernels."""
    pol, args, refs = references(name)
    assert [r.status for r in refs] == [0] * N_EPISODES
    bitwise, overflow = _judge(_run(engines(REPAIRS[name][0], SAMPLED_KERNELS), pol, args), refs, name)
    print(f"{name}: {bitwise} episodes bitwise, {overflow} EG_EP_OVERFLOW")
    assert bitwise == sum(1 for r in refs if max(r.n_def) <= YEAR_REPAIRS) and overflow == N_EPISODES - bitwise
    assert (overflow >= 3 and bitwise >= 3) == name.startswith("demand x12")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REPLAYS))
def test_replays_of_a_long_repair_list(engines, references, name):
    """A best list with 65 deficit entries in 2025 is followed past the 64 a register keeps, bitwise; one with 128 needs 132 slots of
    the year's list: EG_EP_OVERFLOW on every route — the hoisted script, k_replay_lazy and k_replay_solo give the episode up at
    eg_replay_script.h's n_def_y >= 128 and the classic variant behind them reports it, as it does alone; the two-wave kernel reports it
    itself.  The sampled episodes beside the replays are judged like any other."""
    pol, args, refs = references(name)
    assert [r.status for r in refs] == [0] * N_EPISODES
    engine_set = engines(REPLAYS[name], REPLAY_ROUTES)
    results = _run(engine_set, pol, args)
    armed, served = engine_set["hoist"].replay_hoist_stats()
    bitwise, overflow = _judge(results, refs, name, MASK)
    reps = np.flatnonzero(MASK)
    print(f"{name}: {bitwise} episodes bitwise, {overflow} EG_EP_OVERFLOW; replay_hoist_stats() = ({armed}, {served})")
    assert armed >= 1
    if name == "replay x6":
        assert overflow == 0
        # a script is hoisted exactly when its replay episodes draw nothing (tests/test_gpu_replay_hoist.py)
        assert served != bool((results["hoist"].n_draws[reps] > 0).any())
        assert served, "the oracle's replay reads no draw and stays within every capacity: the hoist must have taken it"
    else:
        assert all(_overflow_year(refs[e]) == 0 for e in reps)
        for kind, res in results.items():
            assert (res.status[reps] == N.EG_EP_OVERFLOW).all(), kind
        assert not served, "a script beyond a capacity is left to the per-episode kernels"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all generator types", UPDATE_CROWDED, "replay x12"])
def test_the_update_behind_a_batch_at_the_capacities(engines, references, name):
    """tests/test_gpu_reduced_oracle.py::test_statistics_epilogue_equals_restatement, its bars unchanged, over a batch more than half of
    whose episodes end with EG_EP_OVERFLOW and over one whose years hold 100+ deficit actions: the failed episodes are counted and
    contribute nothing, and the candidate is a finished episode.  The crowded all-types policy has no best lists, so no episode of its
    batch qualifies (ref[2] == 0, asserted) and every logarithm sum is zero on both sides: the bar ref[2] > 0 is met by the same policy
    stalled and with a default episode's record as its best lists — the same seeds, the same 36 failures of 64."""
    import torch
    pol, args, refs = references(name)
    failed = [_overflow_year(r) is not None for r in refs]
    assert sum(failed) >= 20
    for kernel, eng in engines(references.world_of(name), SAMPLED_KERNELS).items():
        packet = torch.zeros(N.PACKET_BYTES, dtype=torch.uint8, device="cuda")
        eng.upload_snapshot(pol)
        eng.launch_update(args["seed"], args["first_episode_index"], N_EPISODES, packet.data_ptr(), replay_mask=args["replay_mask"])
        res = eng.fetch(N_EPISODES)
        host = packet.cpu().numpy()
        dev = host[:8 * N.STATS_LEN].view(np.int64)
        assert (res.status != 0).tolist() == failed and set(res.status.tolist()) == {0, N.EG_EP_OVERFLOW}, (name, kernel, res.status.tolist())
        _, ref, winner = O.reduced_batch_update(oracle_weights_like(pol), *batch_arrays(res), noise_seed=1)
        assert (dev[:3] == ref[:3]).all() and dev[0] + dev[1] == N_EPISODES, (name, kernel, dev[:3], ref[:3])
        assert (ref[2] > 0) == (name != "all generator types"), (name, ref[2])
        assert dev[1] == int((res.status != 0).sum()) == sum(failed)
        A = 26 * 61
        assert (dev[8 + 2 * A:] == ref[8 + 2 * A:]).all(), "deficit counts"
        diff = np.abs(dev[8:8 + 2 * A] - ref[8:8 + 2 * A])
        assert diff.max() <= 2, f"logarithm sums differ by {diff.max()} Q32 units"
        # the candidate record behind the statistics is the restatement's winner, a finished episode
        cand = host[8 * N.STATS_LEN:]
        assert cand[8:16].view(np.int64)[0] == args["first_episode_index"] + winner
        assert winner >= 0 and res.status[winner] == 0
        assert abs(int(dev[3]) - int(ref[3])) <= 8
        print(f"{name}, {kernel}: {sum(failed)} of {N_EPISODES} failed, qualifying {ref[2]}, winner {winner}, Q32 sums identical in "
              f"{int((diff == 0).sum())}/{diff.size} entries, deficit counts {int(dev[8 + 2 * A:].sum())}")
