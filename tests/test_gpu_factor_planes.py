"""The factor table as two planes of 32-bit words (csrc/eg_rollout.hip Smem::dr, factor_at<true>, chunk_product<true>: the lean grid,
the short-replay variant and k_place; the long-replay kernels keep the table of doubles in the same array): a factor's address is the
dot product of the doubled coordinate difference with itself on top of the class's offset, capped at the class's own radius squared,
and its two words come from places 384 words apart (the high plane ends in Smem::park).  What can go wrong is at the table's
edges — the last entry below a class's cap, the cap itself (1.0), distances beyond it, distance 0 (factor 0), the off-grid padding of a
staging row — and at the ends of the staging rows: the padding to groups of four, the kept row's end at 64, the second block.

Single searches (eg_place: k_place runs place_search<0>, the throughput chunk_product).  For a type of each of the six radius classes
and two years, c* is the oracle's winner for the empty list; the lists put generators at every (di, dj) around c* whose squared
distance is the largest sum of two squares below the class's cap, the cap, or the smallest sum of two squares above it (repeated in
that order up to the list's length), and a fourth kind starts with the grid's corners and a generator on c* itself.  Lengths 1, 3, 4,
5, 63, 64, 65 and the on-chip window's 512.  Bar: cell and score equal the oracle's, bitwise.  Without a GPU the file asserts that
the boundary entries decide something: the oracle's score differs between the "below" and the "cap" list of every case, and the "cap"
and "above" lists agree.

Rollouts on the one-wave kernels (EIRGRID_HELPER_WAVES=0): 64 episodes, every fourth a replay, from a short best list and from one
beyond the short-replay limit (96 actions), the latter with the eager field (EIRGRID_SOLO_LAZY=0, k_replay_solo) and with the lazy one
at any length (EIRGRID_SOLO_LAZY=all, k_replay_lazy): the lean grid, the short-replay variant and both per-episode replay kernels —
the two layouts of the one array side by side in a batch.
Bar: every record equals the tabled oracle's, bitwise, as tests/test_gpu_parity.py compares them."""
import os

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, Engine, HostTables
from oracle import api as O
from tests.helpers import assert_episode_equal, oracle_weights_like

GRID = 51
CAPS = (144, 64, 25, 49, 36, 9)      # squared radius in cells of the six classes (12, 8, 5, 7, 6, 3 km)
YEARS = (3, 20)
KINDS = ("below", "cap", "above", "corners")
LENGTHS = (1, 3, 4, 5, 63, 64, 65, N.ONCHIP_GENS)
_SUMS = sorted({a * a + b * b for a in range(14) for b in range(14)})


def _ring(c_star, q):
    """the cells at squared distance q from c_star, in (di, dj) order, those off the grid left out"""
    ci, cj = divmod(c_star, GRID)
    r = int(q ** 0.5) + 1
    out = []
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            if di * di + dj * dj == q and 0 <= ci + di < GRID and 0 <= cj + dj < GRID:
                out.append((ci + di) * GRID + cj + dj)
    return out


def _pattern(c_star, cap, kind):
    below, above = max(s for s in _SUMS if s < cap), min(s for s in _SUMS if s > cap)
    if kind == "corners":
        return [0, GRID - 1, GRID * (GRID - 1), GRID * GRID - 1, c_star] + _ring(c_star, below)
    return _ring(c_star, {"below": below, "cap": cap, "above": above}[kind])


def _xy(cells):
    return [((c // GRID) * 1000.0, (c % GRID) * 1000.0) for c in cells]


@pytest.fixture(scope="module")
def cases(world, oracle_world):
    """{(radius class, year, kind, length): (type, cells, oracle's cell, oracle's score)}, computed once"""
    rclass = HostTables(world).i32("rclass").tolist()
    out = {}
    for rc, cap in enumerate(CAPS):
        assert rc in rclass, f"no generator type of radius class {rc}"
        t = rclass.index(rc)
        for yi in YEARS:
            c_star, s_star = oracle_world.place(yi, t)
            assert c_star >= 0 and s_star > 0.0
            for kind in KINDS:
                pat = _pattern(c_star, cap, kind)
                assert pat, (rc, yi, kind)
                for n in LENGTHS:
                    cells = [pat[k % len(pat)] for k in range(n)]
                    out[rc, yi, kind, n] = (t, cells) + tuple(oracle_world.place(yi, t, _xy(cells)))
    return out


def test_boundary_entries_decide_the_oracle_score(cases):
    """CPU: a generator just inside the radius lowers the winner's score, one on the radius or just beyond leaves c* the winner with
    its score — a kernel that read the entry beside the one it should would show in the GPU test below."""
    for rc in range(len(CAPS)):
        for yi in YEARS:
            for n in LENGTHS:
                below, cap, above = (cases[rc, yi, kind, n][2:] for kind in ("below", "cap", "above"))
                assert below[1] != cap[1], (rc, yi, n)
                assert cap == above, (rc, yi, n)


@pytest.mark.gpu
@pytest.mark.parametrize("rc", range(len(CAPS)))
def test_single_searches_at_the_table_edges(engine, cases, rc):
    for (k_rc, yi, kind, n), (t, cells, ref_cell, ref_score) in cases.items():
        if k_rc != rc:
            continue
        cell, score = engine.find_suitable_location(t, yi, cells)
        assert (cell, float(score).hex()) == (ref_cell, float(ref_score).hex()), (rc, yi, kind, n)


def _one_wave_engine(world, lazy):
    os.environ["EIRGRID_HELPER_WAVES"] = "0"
    os.environ["EIRGRID_SOLO_LAZY"] = lazy
    try:
        return Engine(world, device=0)
    finally:
        for k in ("EIRGRID_HELPER_WAVES", "EIRGRID_SOLO_LAZY"):
            os.environ.pop(k, None)


@pytest.fixture(scope="module")
def one_wave_engines(world):
    engines = {}
    try:
        for name, lazy in (("eager", "0"), ("lazy", "all")):
            engines[name] = _one_wave_engine(world, lazy)
        yield engines
    finally:
        for eng in engines.values():
            eng.close()


def _installed(res, e):
    """a fresh policy with episode e's recorded lists as its best lists (the reference's sequential update)"""
    pol = ActionWeights()
    pol.apply_episode([-5e4, 0.7, 4e10, 1.0], res.n_run[e], res.run_log[e, :res.n_run[e].sum()], res.n_def[e], res.def_log[e, :res.n_def[e].sum()])
    return pol


@pytest.mark.gpu
def test_rollouts_on_the_one_wave_kernels(world, one_wave_engines):
    n = 64
    mask = (np.arange(n) % 4 == 0).astype(np.uint8)
    eager, lazy = one_wave_engines["eager"], one_wave_engines["lazy"]
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    # the short list: config 1's episode; the long one: a replay's recorded lists installed as the next best lists, three times over
    # (a replay records every action twice)
    first = eager.rollout_batch(ActionWeights(), 12345, 1)
    short = _installed(first, 0)
    long_ = short
    for _ in range(3):
        res = eager.rollout_batch(long_, 777, 4, first_episode_index=4096, replay_mask=mask[:4])
        assert res.status[0] == 0
        long_ = _installed(res, 0)
    assert sum(len(l) for l in short.lists(0)) <= 96 < sum(len(l) for l in long_.lists(0))
    for what, pol, runs in (("short list", short, (eager,)), ("long list", long_, (eager, lazy))):
        results = [eng.rollout_batch(pol, 777, n, first_episode_index=5000, replay_mask=mask) for eng in runs]
        for res in results:
            assert (res.status == 0).all(), (what, res.status.tolist())
        for e in range(n):
            st, ref = O.run_episode_tabled(tb, oracle_weights_like(pol), 777 + 5000 + e, replay=bool(mask[e]))
            for k, res in enumerate(results):
                assert_episode_equal(res, e, ref, f"{what}, engine {k}, {'replay' if mask[e] else 'sampled'}")
