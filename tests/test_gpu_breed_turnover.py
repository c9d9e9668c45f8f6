"""GPU: k_breed_gather, k_breed_turnover (csrc/eg_breed.h) and k_explore_turnover (csrc/eg_explore.h) on crafted archives, through the
test hooks eg_debug_breed_begin / _chunk / _turnover / _fetch (include/eirgrid_hip.h): synthetic records and tagged plan blocks, no
rollout.  Every scenario is built in tests/test_breed_turnover.py, which asserts on the CPU what it was built for; here its steps run
on the device beside the restatement (Archive), and after EVERY step — begin, chunk, turnover — the whole of the device's memory the
kernels may write is compared with the restatement's model byte for byte: the state and all its entries, the 256 block slots (the
owner's block, the last owner's, or canary), the tag of the 256 record slots, both parent / frontier arrays, the readback buffer (header,
rows, canary or an earlier turnover's rows beyond the count) and the counters.  There are no tolerances."""
import json
import os
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from tests.test_breed_turnover import (BIG_N, BLOCK, BREED, CANARY, ENTRY, EXPLORE, FAR, HEADER, ROW, WINDOW_N, Run, anti, below, case1_breed,
                                       case1_explore, case_count, case_empty, case_evict, case_window, ok)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


@pytest.fixture(scope="module")
def eng(built):
    from eirgrid_amd.engine import Engine
    from eirgrid_amd.world import World
    e = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    yield e
    e.close()


def _units(got, want, unit):
    g, w = np.asarray(got).reshape(-1, unit), np.asarray(want).reshape(-1, unit)
    return np.flatnonzero((g != w).any(1)).tolist()


def _tag(block):
    """The variant number's hash a block carries, or "canary" / "torn" (a block that is not one tagged block)."""
    b = np.asarray(block)
    if (b == CANARY).all():
        return "canary"
    w = b.view("<u4").astype(np.int64)
    return hex(int(w[0])) if ((w - w[0]) % 2**32 == np.arange(len(w))).all() else "torn"


def check(eng, arch, what):
    """The device against the restatement's model, everything the kernels may write."""
    d = eng._debug_breed_fetch()
    state, want = d["state"], arch.state()
    head = struct.unpack("<iiiiqq", state[:32].tobytes())
    assert head == struct.unpack("<iiiiqq", want[:32].tobytes()), (what, "state header (cap, n_held, objectives, mode, n_dropped, pad)", head)
    bad = _units(state[32:], want[32:], ENTRY.itemsize)
    assert not bad, (what, "state entries", bad[:8], np.frombuffer(state[32:].tobytes(), ENTRY)[bad[:2]], np.frombuffer(want[32:].tobytes(), ENTRY)[bad[:2]])
    bad = _units(d["blocks"], arch.blocks, BLOCK)
    assert not bad, (what, "block slots", bad[:8], [(_tag(d["blocks"][s]), _tag(arch.blocks[s]), arch.owner[s]) for s in bad[:4]])
    bad = np.flatnonzero(d["tags"] != arch.tags).tolist()
    assert not bad, (what, "record slot tags", bad[:8], d["tags"][bad[:8]].tolist(), arch.tags[bad[:8]].tolist())
    for a in (0, 1):
        bad = _units(d["arrays"][a], arch.arrays[a], BLOCK)
        assert not bad, (what, f"array {a} positions", bad[:8], [(_tag(d["arrays"][a][s]), _tag(arch.arrays[a][s])) for s in bad[:4]])
    rb, want = d["readback"], arch.readback
    assert rb[:HEADER].tobytes() == want[:HEADER].tobytes(), (what, "readback header (n_held, n_new, n_dropped, n_valid, pad)",
                                                               struct.unpack("<iiqqq", rb[:HEADER].tobytes()), struct.unpack("<iiqqq", want[:HEADER].tobytes()))
    bad = _units(rb[HEADER:], want[HEADER:], ROW)
    assert not bad, (what, "readback rows", bad[:8], [np.flatnonzero(rb[HEADER + r * ROW:HEADER + (r + 1) * ROW] != want[HEADER + r * ROW:HEADER + (r + 1) * ROW])[:4].tolist() for r in bad[:4]])
    got = struct.unpack("<QII", d["counters"].tobytes())
    assert got == struct.unpack("<QII", arch.counters().tobytes()), (what, "counters (n_valid, done, pad)", got)
    return d


def run(eng):
    return Run(eng, check)


# ---- case 1: sizes across the ballot words -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [5, 15])
def test_breed_turnover_at_every_size(eng, mask):
    """1 .. 256 entries, one below, at and one above every multiple of the wave; a generation per size into the arrays 0 and 1
    alternately; n_held and n_dropped are 0 on the device afterwards (the state check)."""
    R = run(eng)
    case1_breed(R, mask)
    assert R.steps >= 12 * 3


@pytest.mark.parametrize("mask", [5, 15])
def test_explore_turnover_across_the_four_ballot_words(eng, mask):
    """One archive grown through every size with the entered members turned over each time, then at 256 entries the new suffix started
    at entry 0, 1, 63, 64, 65, 128, 192, 255, at nobody, between two indices and at m_first 0; the state is the same bytes before and after
    every call (the restatement's state does not move)."""
    R = run(eng)
    case1_explore(R, mask)
    assert len(R.arch.index) == 256


# ---- cases 2 and 3: eviction, slot reuse, capacity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
def test_eviction_and_slot_reuse(eng, mask, kind):
    """200 held, two chunks that dominate every third held entry and add new ones (new entries in freed low slots: slot != position),
    equal points at higher numbers that change nothing."""
    did = case_evict(run(eng), mask, kind)
    assert did[1]["retaken"] == 67 and did[2]["moved"] >= 40


@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
@pytest.mark.parametrize("cap,n_new", [(8, 5), (256, 150)])
def test_truncated_fronts(eng, mask, kind, cap, n_new):
    """More than cap alive: the gather follows what k_pareto_finalize kept, n_dropped stands in both headers, a dropped point never
    reaches a slot."""
    R = run(eng)
    did = case_evict(R, mask, kind, cap=cap, n_new=n_new)
    assert all(len(d["cut"]) > 0 for d in did[1:3]) and R.steps > 4


# ---- case 4: the gather's window -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
@pytest.mark.parametrize("n", WINDOW_N)
def test_the_gathers_window(eng, mask, kind, n):
    """first = 2^40 + 5: the entries with index first and first + n - 1 get pool blocks 0 and n - 1, the entries held from the chunk before
    keep their own blocks although the pool holds others now."""
    did = case_window(run(eng), mask, kind, n)
    assert FAR in did["new"] and FAR + n - 1 in did["new"]


def test_the_gathers_window_at_a_full_launch(eng):
    did = case_window(run(eng), 5, EXPLORE, BIG_N)
    assert FAR + BIG_N - 1 in did["new"]


# ---- case 5: counting ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [5, 15])
@pytest.mark.parametrize("kind", [BREED, EXPLORE])
@pytest.mark.parametrize("n", WINDOW_N)
def test_n_valid_over_the_chunks_of_a_generation(eng, mask, kind, n):
    """Failed and NaN records sprinkled in (records 0 and n - 1 too), -0.0 and infinities valid; the header's n_valid is the sum over the
    generation's chunks, the counters are empty behind the turnover, and a second generation straight behind it counts from zero."""
    sums = case_count(run(eng), mask, kind, n)
    assert len(sums) == 2


def test_n_valid_at_a_full_launch(eng):
    sums = case_count(run(eng), 15, BREED, BIG_N)
    assert sums[0] > BIG_N // 2


@pytest.mark.parametrize("kind", [BREED, EXPLORE])
def test_a_generation_without_a_valid_variant(eng, kind):
    R = run(eng)
    case_empty(R, 5, kind)
    d = eng._debug_breed_fetch()
    assert (d["arrays"][0] == CANARY).all() and (d["arrays"][1] == CANARY).all() and (d["readback"][HEADER:] == CANARY).all() and (d["blocks"] == CANARY).all()


# ---- case 6: nothing else moves --------------------------------------------------------------------------------------------------------
def test_the_contexts_own_archive_is_not_touched(eng):
    from tests.test_gpu_pareto import RECORD_FIELDS, same
    rng = np.random.default_rng(6)
    eng.track_pareto(64, ("emissions", "cost"))
    try:
        for b in range(3):
            p = anti(range(20 * b, 20 * b + 20))
            eng._debug_pareto_fold(np.concatenate([p, below(p)])[rng.permutation(40)], ok(40), 1000 * b)
        before = eng.fetch_pareto()
        assert len(before[1]) == 60
        case_evict(run(eng), 5, BREED)
        case1_explore(run(eng), 15)
        same(eng.fetch_pareto(), before, "a crafted generation", RECORD_FIELDS)
    finally:
        eng.track_pareto(0)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(eng):
    from eirgrid_amd.engine import Engine, Group
    from eirgrid_amd.world import World
    L = N.lib()
    m, st = np.ascontiguousarray(anti(range(4))), ok(4)
    mp, sp = m.ctypes.data_as(N.C.POINTER(N.C.c_double)), st.ctypes.data_as(N.C.POINTER(N.C.c_int32))

    def refused(rc, word):
        assert rc == N.EG_ERR_BAD_ARG and word in L.eg_last_error().decode(), (rc, word, L.eg_last_error())

    R = run(eng)
    R.begin(16, 5)
    R.chunk(m, st, 100)
    for args, word in (((0, 5, 1), "cap"), ((257, 5, 1), "cap"), ((8, 0, 1), "objectives"), ((8, 16, 1), "objectives"), ((8, 5, 0), "mode"), ((8, 5, 3), "mode")):
        refused(L.eg_debug_breed_begin(eng.h, *args), word)
    refused(L.eg_debug_breed_chunk(eng.h, mp, sp, 0, 200), "n = 0")
    refused(L.eg_debug_breed_chunk(eng.h, mp, sp, N.CROSS_MAX_VARIANTS + 1, 200), "EG_CROSS_MAX_VARIANTS")
    refused(L.eg_debug_breed_chunk(eng.h, None, sp, 4, 200), "bad argument")
    refused(L.eg_debug_breed_chunk(eng.h, mp, sp, 4, 2**63 - 2), "2^63")
    for args, word in (((0, 0, 0), "kind"), ((3, 0, 0), "kind"), ((BREED, 2, 0), "next"), ((EXPLORE, -1, 0), "next"), ((EXPLORE, 0, -1), "m_first")):
        refused(L.eg_debug_breed_turnover(eng.h, *args), word)
    check(eng, R.arch, "behind the refusals")      # nothing moved: the chunk's state, its running n_valid, canary elsewhere
    R.turnover(BREED, 0)
    world = World.from_json_dict(json.load(open(WORLD)))
    fresh = Engine(world, device=0)
    g = Group(world, devices=(0, 0))
    try:
        refused(L.eg_debug_breed_chunk(fresh.h, mp, sp, 4, 0), "eg_debug_breed_begin first")
        refused(L.eg_debug_breed_turnover(fresh.h, BREED, 0, 0), "eg_debug_breed_begin first")
        refused(L.eg_debug_breed_fetch(fresh.h, None, None, None, None, None, None, None), "eg_debug_breed_begin first")
        rank = g.ranks[0].h
        refused(L.eg_debug_breed_begin(rank, 8, 5, 1), "eg_group")
        refused(L.eg_debug_breed_chunk(rank, mp, sp, 4, 0), "eg_group")
        refused(L.eg_debug_breed_turnover(rank, BREED, 0, 0), "eg_group")
        refused(L.eg_debug_breed_fetch(rank, None, None, None, None, None, None, None), "eg_group")
    finally:
        g.close(); fresh.close()
