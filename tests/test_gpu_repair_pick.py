"""GPU: k_repair_pick_many (csrc/eg_repair.h) on crafted batches through eg_debug_repair_pick_many — records, yearly rows and constraints
made here, judged on the device by k_plan_constraints (eg_debug_constrain_last_batch), picked segment by segment, and compared byte for
byte with tests/test_repair.py pick_restated fed tests/test_plan_constraints.py judge: the entries and the base blocks."""
import functools

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd._native import EirgridError
from eirgrid_amd.constraints import Constraint
from tests.test_crafted_folds import level_metrics, refine_block
from tests.test_gpu_plan_constraints import SPECIAL, constrained
from tests.test_gpu_refine_many import _base_words
from tests.test_plan_constraints import judge
from tests.test_repair import pick_restated

pytestmark = pytest.mark.gpu

# one thread, two, the wave's edge, the workgroup's edge, a third stride trip; the boundaries 1, 3, 66, 130, 195, 1 218, 2 242, 3 267 lie
# off every multiple of 64
SEGMENTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
FIRST = tuple(int(x) for x in np.concatenate([[0], np.cumsum(SEGMENTS)[:-1]]))
CLEAN = 7.0      # a record whose rows are all CLEAN meets every constraint below


def _constraints(k, rng):
    """k constraints every one of which rows of CLEAN everywhere satisfy — some with slack, some exactly on the bound; constraint 0 is
    "every year of column 5 <= CLEAN + 2"; column 3 only ever meets a bound equal to it"""
    cs = [Constraint(5, "<=", CLEAN + 2.0)]
    for i in range(1, k):
        lo = int(rng.integers(0, 26)); hi = int(rng.integers(lo + 1, 27))
        if i % 5 == 0:
            lo, hi = 0, 26
        col = 3 if i % 7 == 3 else int(rng.integers(0, 21))
        d = 0.0 if col == 3 else float(rng.choice([0.0, 5.5, 23.0]))
        le = rng.random() < 0.5
        if i % 3 == 1:
            cs.append(Constraint(col, "<=" if le else ">=", CLEAN * (hi - lo) + (d if le else -d) * (hi - lo), lo, hi, "sum"))
        else:
            cs.append(Constraint(col, "<=" if le else ">=", CLEAN + (d if le else -d), lo, hi))
    return cs


def _dirty(over):
    """CLEAN rows but for one year of column 5, `over` above constraint 0's bound (NaN: a NaN there)"""
    rows = np.full((26, 21), CLEAN)
    rows[5, 5] = CLEAN + 2.0 + over
    return rows


@functools.lru_cache(maxsize=None)
def _crafted(k):
    """(rows, constraints, status as loaded, metrics, what judge makes of them), 5 316 records in the nine SEGMENTS; by segment:
      0  a clean base alone: feasible
      1  a failed base in front of a clean record: nothing moves
      2  every record a copy of a dirty base, some failed: nothing lies strictly below it — stuck
      3  a base with a NaN excess (V = +inf) among copies of itself, one dirty record with a finite V: it moves there
      4  copies of a very dirty base but two equal mildly dirty records, the later one scoring higher: the tie on V goes to the score
      5  the same with three records equal in V and score, a lower-scoring fourth in front of them: the lowest index of the three
      6  random rows with specials, NaN metrics and failures
      7  copies of the base; the only record below it sits alone in the last stride trip
      8  random rows; clean records spread over the trips, the best-scoring one in the third"""
    rng = np.random.default_rng(7000 + k)
    n = int(np.sum(SEGMENTS))
    cs = _constraints(k, rng)
    rows = rng.normal(0.0, 10.0, (n, 26, 21)).round(1)
    hit = rng.random(rows.shape) < 0.03
    rows[hit] = rng.choice(SPECIAL, int(hit.sum()))
    rows[:, :, 3] = CLEAN
    status = rng.choice(np.array([0, 0, 0, -1, -2], np.int32), n).astype(np.int32)
    level = rng.integers(0, 50, n).astype(np.float64)
    f = FIRST
    status[list(f)] = 0
    rows[f[0]] = CLEAN
    status[f[1]] = -2; rows[f[1] + 1] = CLEAN; status[f[1] + 1] = 0
    rows[f[2]:f[3]] = _dirty(4.0)
    rows[f[3]:f[4]] = _dirty(np.nan); rows[f[3] + 40] = _dirty(1e6); status[f[3] + 40] = 0
    rows[f[4]:f[5]] = _dirty(50.0)
    for j, lv in ((10, 3.0), (20, 8.0)):
        rows[f[4] + j] = _dirty(0.5); status[f[4] + j] = 0; level[f[4] + j] = lv
    rows[f[5]:f[6]] = _dirty(50.0)
    for j, lv in ((5, 2.0), (700, 9.0), (900, 9.0), (1000, 9.0)):
        rows[f[5] + j] = _dirty(0.5); status[f[5] + j] = 0; level[f[5] + j] = lv
    rows[f[7]:f[8]] = _dirty(50.0); rows[f[7] + 1024] = _dirty(0.25); status[f[7] + 1024] = 0
    for j, lv in ((100, 60.0), (1500, 70.0), (2048, 9000.0), (2047, 60.0)):
        rows[f[8] + j] = CLEAN; status[f[8] + j] = 0; level[f[8] + j] = lv
    m = level_metrics(level)
    for s in (6, 8):      # NaN scores in mode 1, a candidate that scores -inf there
        m[f[s] + 3:f[s] + SEGMENTS[s]:11, :2] = (-1.0, np.nan)
        m[f[s] + 10] = (-5.0, -np.inf, 1e10, 1.0); status[f[s] + 10] = 0
    return rows, cs, status, m, judge(rows, status, cs)


def _weights(k, trivial):
    return None if trivial else (10.0 ** np.arange(k) * np.where(np.arange(k) % 2, 3.0, 0.1))[::-1] / 1e12


def _entry(r, status, m, violated, f, n):
    """the entry k_repair_pick_many must leave for a segment whose round pick_restated saw as `r`"""
    e = N.EgDebugRepairEntry()
    w = f + max(r["winner"], 0)
    j = max(r["winner"], 0)
    e.winner, e.n_failed, e.n_feasible, e.base_ok, e.n = r["winner"], r["n_failed"], r["n_feasible"], r["base_ok"], n
    e.edit[0], e.edit[1] = w, ~w & 0xFFFFFFFF
    e.metrics[:] = [float(x) for x in m[w]]
    e.off26, e.offd26 = w % 4097, (w // 3) % 4097
    if r["base_ok"]:
        e.violation, e.score, e.violated = r["V"][j], r["score"][j], int(violated[w])
        e.base_violation, e.base_score, e.base_violated = r["V"][0], r["score"][0], int(violated[f])
    return e


@pytest.mark.parametrize("k, trivial, mode", [(1, True, 1), (1, False, 2), (31, False, 1), (32, True, 2), (32, False, 1)])
def test_crafted_segments_are_picked_as_the_definition_says(engine, k, trivial, mode):
    rows, cs, status, m, (judged, violated, excess) = _crafted(k)
    weights = _weights(k, trivial)
    first, count = np.array(FIRST, np.uint32), np.array(SEGMENTS, np.uint32)
    with constrained(engine, cs):
        engine._debug_load_batch(m, status, 0)
        engine._debug_load_yearly(rows)
        engine._debug_constrain_last_batch()
        entries, bases = engine._debug_repair_pick_many(first, count, mode, weights)
        again, bases_again = engine._debug_repair_pick_many(first, count, mode, weights)      # the pick judges nothing and moves no record
    seen = set()
    for s, (f, n) in enumerate(zip(FIRST, SEGMENTS)):
        r = pick_restated(judged[f:f + n], m[f:f + n], excess[f:f + n], mode, weights)
        want = _entry(r, judged, m, violated, f, n)
        e = entries[s]
        assert (e.winner, e.n_failed, e.n_feasible, e.base_ok, e.n) == (want.winner, want.n_failed, want.n_feasible, want.base_ok, want.n), (s, r["stop"])
        assert bytes(e) == bytes(want), (s, r["stop"], [(name, getattr(e, name), getattr(want, name)) for name, _ in e._fields_ if name not in ("edit", "metrics")])
        assert bytes(again[s]) == bytes(e), s
        w = f + max(r["winner"], 0)
        assert bases[s].tobytes() == (refine_block(w) if r["winner"] > 0 else _base_words(s)).tobytes(), (s, "the base block")      # untouched where winner <= 0
        assert bases_again[s].tobytes() == bases[s].tobytes(), s
        # what the crafted batch is there for
        seen.add(r["stop"])
        V, sc, cand, win = r["V"], r["score"], r["cand"], r["winner"]
        if win > 0:
            tied = [j for j in range(n) if cand[j] and j != win and V[j] == V[win]]
            if any(sc[j] < sc[win] for j in tied):
                seen.add("tie on V, to the score")
            if any(sc[j] == sc[win] and j > win for j in tied):
                seen.add("tie on both, to the index")
            if V[0] == float("inf"):
                seen.add("a base at +inf moves")
            if win >= 2048:
                seen.add("third trip")
    assert seen >= {"feasible", "base_failed", "stuck", None, "tie on V, to the score", "tie on both, to the index", "a base at +inf moves", "third trip"}, seen
    assert (judged == N.EG_EP_INFEASIBLE).any() and (judged[status != 0] == status[status != 0]).all() and {-1, -2} <= set(status.tolist())


@pytest.mark.parametrize("n", [1, 2, 65])
def test_a_launch_of_one_small_segment(engine, n):
    rows, cs, status, m, _ = _crafted(1)
    f = FIRST[4]      # the segment of the tie on V: cut short, the base alone is stuck, with its mildly dirty records it moves
    rows, status, m = rows[f:f + n], status[f:f + n], m[f:f + n]
    judged, violated, excess = judge(rows, status, cs)
    with constrained(engine, cs):
        engine._debug_load_batch(m, status, 0)
        engine._debug_load_yearly(rows)
        engine._debug_constrain_last_batch()
        entries, bases = engine._debug_repair_pick_many([0], [n], 1, [2.5])
    r = pick_restated(judged, m, excess, 1, [2.5])
    assert bytes(entries[0]) == bytes(_entry(r, judged, m, violated, 0, n)) and r["stop"] == ("stuck" if n < 65 else None) and r["winner"] == (0 if n < 65 else 20)
    assert bases[0].tobytes() == (refine_block(20) if n == 65 else _base_words(0)).tobytes()


def test_the_hook_refuses_what_it_cannot_do(engine):
    rows, cs, status, m, _ = _crafted(1)
    first, count = np.array(FIRST, np.uint32), np.array(SEGMENTS, np.uint32)
    with constrained(engine, cs):
        engine._debug_load_batch(m, status, 0)
        with pytest.raises(EirgridError, match="eg_debug_repair_pick_many: the last batch was not judged"):
            engine._debug_repair_pick_many(first, count, 1)
        engine._debug_load_yearly(rows)
        engine._debug_constrain_last_batch()
        for bad in ([0.0], [-1.0], [np.inf], [np.nan]):
            with pytest.raises(EirgridError, match=r"weights\[0\] = .* \(finite and > 0\)"):
                engine._debug_repair_pick_many(first, count, 1, bad)
        with pytest.raises(EirgridError, match="tiling"):
            engine._debug_repair_pick_many(first[::-1].copy(), count, 1)
        with pytest.raises(EirgridError, match="cover"):
            engine._debug_repair_pick_many(first[:-1], count[:-1], 1)
        with pytest.raises(EirgridError, match="bad argument"):
            engine._debug_repair_pick_many(first, count, 3)
        engine._debug_load_batch(m, status, 0)      # a fresh crafted batch is not judged until it is constrained again
        with pytest.raises(EirgridError, match="was not judged"):
            engine._debug_repair_pick_many(first, count, 1)
