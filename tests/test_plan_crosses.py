"""CPU: the host side of plan crosses (include/eirgrid_hip.h eg_evaluate_plan_crosses) — the struct layout, what the validator accepts and
refuses, PlanCross.apply against lists written out by hand and a restatement written out here (`apply_cross`, which the GPU tests
import), the order of cross_pairs, and the host's front filter (engine.pareto_filter) against an O(n^2) restatement (`front_restated`)."""
import ctypes as C
import os

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import Plan, PlanCross, PlanSet, _cross_array, cross_pairs, pareto_filter
from tests.test_plans import _empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def apply_cross(parents, x):
    """Cross x over `parents`, written out once more (not PlanCross.apply: the tests' own restatement): year by year, both lists of a
    year inside the window are parent b's, the others parent a's."""
    run, dfc = [], []
    for y in range(26):
        src = parents[x.b] if x.from_year <= y < x.to_year else parents[x.a]
        run.append(list(src.best_actions[y])); dfc.append(list(src.best_deficit_actions[y]))
    return Plan(run, dfc, parents[x.a].name)


def front_restated(metrics, status, mask):
    """The variants that eg_pareto_track's definitions keep, by the definitions and nothing else, O(n^2): valid = status 0 and no NaN
    among the four metrics; a dominates b = at least as good in every active metric (lower 0 and 2, higher 1 and 3) and better in
    one; equal active metrics = one point, held by the lowest variant.  Ascending variant numbers."""
    metrics = np.asarray(metrics, np.float64).reshape(-1, 4)
    active = [i for i in range(4) if mask >> i & 1]
    better = lambda i, a, b: a < b if i in (0, 2) else a > b
    valid = [j for j in range(len(metrics)) if status[j] == 0 and not any(np.isnan(v) for v in metrics[j])]

    def dominates(a, b):
        return all(not better(i, metrics[b][i], metrics[a][i]) for i in active) and any(better(i, metrics[a][i], metrics[b][i]) for i in active)

    def same(a, b):
        return all(metrics[a][i] == metrics[b][i] for i in active)
    return [j for j in valid if not any(dominates(k, j) for k in valid) and not any(same(k, j) for k in valid if k < j)]


def _parents():
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[6] = [3]; run[7] = [9, 10, 11, 12]; run[25] = [45, 0]
    dfc[0] = [24]; dfc[6] = [24, 60, 21]
    a = Plan(run, dfc, "A")
    run = _empty(); dfc = _empty()
    run[0] = [1]; run[5] = [2, 2]; run[7] = [8]; run[24] = [30, 31, 32]
    dfc[6] = [21]; dfc[7] = [24, 24]; dfc[25] = [60]
    b = Plan(run, dfc, "B")
    return [a, b, Plan(_empty(), _empty(), "empty")]


def _validate(parents, crosses, n=None):
    L = N.lib()
    ps = PlanSet(parents) if parents is not None else None
    arr, k = _cross_array(crosses)
    rc = L.eg_plan_crosses_validate(C.byref(ps.s) if ps is not None else None, arr, k if n is None else n)
    return rc, L.eg_last_error().decode()


# ---------------------------------------------------------------- layout
def test_struct_layout_is_the_headers(built):
    X = N.EgPlanCross
    assert C.sizeof(X) == 6 and (X.a.offset, X.b.offset, X.from_year.offset, X.to_year.offset) == (0, 2, 4, 5)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert "typedef struct { uint16_t a, b; uint8_t from_year, to_year; } eg_plan_cross;" in header
    assert "#define EG_CROSS_MAX_PARENTS 256" in header and "#define EG_CROSS_MAX_VARIANTS 16384" in header
    assert (N.CROSS_MAX_PARENTS, N.CROSS_MAX_VARIANTS) == (256, 16384)
    assert "eg_plan_crosses_validate" in N.EXPORTS and "eg_evaluate_plan_crosses" in N.EXPORTS
    # the library's side of sizeof(eg_plan_cross): it steps through an array as ctypes laid it out, and names the third
    rc, msg = _validate(_parents(), [PlanCross(0, 1, 3, 26), PlanCross(1, 0, 0, 1), PlanCross(1, 2, 9, 8)])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_crosses_validate: cross 2: from_year 9 > to_year 8", msg


# ---------------------------------------------------------------- PlanCross.apply
def test_apply_against_lists_written_out_by_hand():
    ps = _parents()
    a, b = ps[0], ps[1]
    # head of A, tail of B, cut at 2031 (year 6): years 0..5 are A's, 6..25 are B's
    got = PlanCross(0, 1, 6, 26).apply(ps)
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[7] = [8]; run[24] = [30, 31, 32]
    dfc[0] = [24]; dfc[6] = [21]; dfc[7] = [24, 24]; dfc[25] = [60]
    assert (got.best_actions, got.best_deficit_actions) == (run, dfc) and got.name == "A"
    # B's 2031 and 2032 dropped into A: both lists of the two years
    got = PlanCross(0, 1, 6, 8).apply(ps)
    run = [list(l) for l in a.best_actions]; dfc = [list(l) for l in a.best_deficit_actions]
    run[6] = []; run[7] = [8]; dfc[6] = [21]; dfc[7] = [24, 24]
    assert (got.best_actions, got.best_deficit_actions) == (run, dfc)
    # one year transplanted; year 5 is empty in A
    got = PlanCross(0, 1, 5, 6).apply(ps)
    run = [list(l) for l in a.best_actions]
    run[5] = [2, 2]
    assert (got.best_actions, got.best_deficit_actions) == (run, a.best_deficit_actions)
    # the whole plan replaced; the window's last year is 25
    assert PlanCross(0, 1, 0, 26).apply(ps) == b and PlanCross(0, 1, 0, 26).apply(ps).name == "A"
    got = PlanCross(1, 0, 25, 26).apply(ps)
    assert got.best_actions[25] == [45, 0] and got.best_deficit_actions[25] == [] and got.best_actions[:25] == b.best_actions[:25]
    # an empty parent on either side
    assert len(PlanCross(0, 2, 0, 7).apply(ps)) == 6 and PlanCross(2, 0, 7, 8).apply(ps).best_actions[7] == [9, 10, 11, 12]
    assert ps[0] == _parents()[0] and ps[1] == _parents()[1]      # (copies: the parents are left alone)
    got.best_actions[25].append(1)
    assert ps[0].best_actions[25] == [45, 0]


def test_identities_are_parent_a():
    ps = _parents()
    for x in (PlanCross(0, 0, 0, 26), PlanCross(0, 0, 3, 9), PlanCross(0, 1, 0, 0), PlanCross(0, 1, 7, 7), PlanCross(0, 1, 26, 26), PlanCross(1, 1, 0, 0)):
        assert x.apply(ps) == ps[x.a] and apply_cross(ps, x) == ps[x.a], x
        assert _validate(ps, [x])[0] == N.EG_OK


def test_apply_on_random_crosses_is_the_restatement(built):
    rng = np.random.default_rng(8)
    for _ in range(200):
        ps = [Plan([[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 5)))] for _ in range(26)],
                   [[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 3)))] for _ in range(26)], f"p{k}") for k in range(3)]
        to = int(rng.integers(0, 27))
        x = PlanCross(int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, to + 1)), to)
        got = x.apply(ps)
        assert got == apply_cross(ps, x) and got.name == ps[x.a].name, x
        assert len(got) == len(ps[x.a]) - sum(len(l) for l in ps[x.a].best_actions[x.from_year:x.to_year]) + sum(len(l) for l in ps[x.b].best_actions[x.from_year:x.to_year])
        assert _validate(ps, [x])[0] == N.EG_OK


# ---------------------------------------------------------------- cross_pairs
def test_cross_pairs_order_and_count():
    got = cross_pairs(3)
    assert got[:3] == [PlanCross(0, 0, 0, 0), PlanCross(1, 1, 0, 0), PlanCross(2, 2, 0, 0)]
    assert got[3:6] == [PlanCross(0, 1, 1, 26), PlanCross(0, 1, 2, 26), PlanCross(0, 1, 3, 26)]
    assert got[3 + 25] == PlanCross(0, 2, 1, 26) and got[3 + 50] == PlanCross(1, 0, 1, 26) and got[-1] == PlanCross(2, 1, 25, 26)
    assert len(got) == 3 + 3 * 2 * 25 == len(set(got))
    assert [(x.a, x.b, x.from_year) for x in got[3:]] == sorted((x.a, x.b, x.from_year) for x in got[3:])
    assert len(cross_pairs(25)) == 25 + 25 * 24 * 25 == 15025 and len(cross_pairs(1)) == 1
    assert cross_pairs(2, cuts=(10, 3)) == [PlanCross(0, 0, 0, 0), PlanCross(1, 1, 0, 0), PlanCross(0, 1, 10, 26), PlanCross(0, 1, 3, 26),
                                            PlanCross(1, 0, 10, 26), PlanCross(1, 0, 3, 26)]      # (the cuts in the order given)
    assert cross_pairs(4, cuts=()) == [PlanCross(p, p, 0, 0) for p in range(4)]


# ---------------------------------------------------------------- eg_plan_crosses_validate
def test_validate_accepts_every_well_formed_cross(built):
    ps = _parents()
    crosses = [PlanCross(a, b, f, t) for a in range(3) for b in range(3) for t in range(27) for f in range(t + 1)]
    rc, msg = _validate(ps, crosses)
    assert rc == N.EG_OK, msg
    assert _validate(ps, cross_pairs(3))[0] == N.EG_OK
    # two full plans whose windows are equally long: the child holds exactly 4 096 entries
    full = [[60] * 157 for _ in range(26)]
    full[0] = full[0] + [60] * (4096 - 26 * 157)
    assert _validate([Plan(full, full), Plan(full, full)], [PlanCross(0, 1, 3, 9), PlanCross(1, 0, 0, 26)])[0] == N.EG_OK
    assert _validate([_parents()[0]] * 256, [PlanCross(255, 0, 1, 26)])[0] == N.EG_OK
    assert _validate(ps, [PlanCross()] * 16384)[0] == N.EG_OK


@pytest.mark.parametrize("cross, expect", [
    (PlanCross(3, 0, 0, 1), "cross 2: a 3 >= n_plans 3"),
    (PlanCross(0, 3, 0, 1), "cross 2: b 3 >= n_plans 3"),
    (PlanCross(0, 65535, 0, 0), "cross 2: b 65535 >= n_plans 3"),
    (PlanCross(0, 1, 0, 27), "cross 2: to_year 27 (at most 26)"),
    (PlanCross(0, 1, 27, 27), "cross 2: to_year 27 (at most 26)"),
    (PlanCross(0, 1, 5, 4), "cross 2: from_year 5 > to_year 4"),
    (PlanCross(0, 0, 26, 0), "cross 2: from_year 26 > to_year 0"),
])
def test_validate_names_the_cross_and_the_field(built, cross, expect):
    rc, msg = _validate(_parents(), [PlanCross(0, 1, 1, 26), PlanCross(1, 1, 0, 0), cross])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_crosses_validate: " + expect, msg


def test_validate_refuses_an_over_long_child(built):
    # A: 4 000 entries in the first 25 years; B: 212 entries more than A in year 3 — B's year 3 dropped into A makes 4 212
    a_run = [[7] * 160 for _ in range(25)] + [[]]
    b_run = _empty(); b_run[3] = [9] * 372
    a = Plan(a_run, [[24] * 100 for _ in range(26)]); b = Plan(b_run, [[21] * 157 for _ in range(26)])
    ok = [PlanCross(0, 0, 0, 0)] * 7
    rc, msg = _validate([a, b], ok + [PlanCross(0, 1, 3, 4)])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_crosses_validate: cross 7: best_actions would hold 4212 entries (at most 4096)", msg
    rc, msg = _validate([a, b], ok + [PlanCross(0, 1, 3, 4)], 7)      # (the eighth is not looked at)
    assert rc == N.EG_OK, msg
    # the deficit list: B with 4 096 deficit entries takes a year of A's that is one entry longer than its own
    b2 = Plan(b_run, [[21] * 157 for _ in range(25)] + [[21] * 171])      # 4 096 deficit entries
    rc, msg = _validate([a, b2], [PlanCross(1, 0, 0, 26), PlanCross(1, 0, 25, 26), PlanCross(1, 0, 0, 1), PlanCross(0, 1, 0, 1)])
    assert rc == N.EG_OK, msg      # (A's years hold 100: every child is shorter)
    a3 = Plan(a_run, [[24] * 158] + [[24] * 100 for _ in range(25)])
    rc, msg = _validate([a3, b2], [PlanCross(1, 0, 1, 1), PlanCross(1, 0, 0, 1)])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_crosses_validate: cross 1: best_deficit_actions would hold 4097 entries (at most 4096)", msg


def test_validate_refuses_bad_counts_null_crosses_and_bad_parent_sets(built):
    ps = _parents()
    L = N.lib()
    for n in (0, -3, 16385):
        rc, msg = _validate(ps, [PlanCross()], n)
        assert rc == N.EG_ERR_BAD_ARG and msg == f"eg_plan_crosses_validate: n_crosses = {n} (1..16384)", msg
    s = PlanSet(ps)
    assert L.eg_plan_crosses_validate(C.byref(s.s), None, 1) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_crosses_validate: NULL crosses"
    rc, msg = _validate([ps[0]] * 257, [PlanCross()])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_crosses_validate: the set holds 257 plans (at most 256)", msg
    rc, msg = _validate(None, [PlanCross()])
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    rc, msg = _validate([], [PlanCross()])
    assert rc == N.EG_ERR_BAD_ARG and "n_plans" in msg, msg
    bad = _parents(); bad[1].best_actions[5][1] = 61
    rc, msg = _validate(bad, [PlanCross()])
    assert rc == N.EG_ERR_BAD_ARG and "plan 1" in msg and "61 >= 61" in msg, msg


def test_evaluate_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_evaluate_plan_crosses(None, None, None, None, None, 1, 0, 0, 1, None) == N.EG_ERR_BAD_ARG
    assert "eg_evaluate_plan_crosses: bad argument" in L.eg_last_error().decode()


# ---------------------------------------------------------------- the front filter
def _crafted():
    """(metrics [n,4], status [n]): ties, repeated points, a NaN in an active and in a masked metric, failed statuses, infinities, zeros of
    both signs, and points that only a masked objective tells apart"""
    nan, inf = float("nan"), float("inf")
    rows = [
        ((10.0, 0.5, 100.0, 0.9), 0),      # 0
        ((10.0, 0.5, 100.0, 0.9), 0),      # 1: the same point as 0
        ((9.0, 0.5, 100.0, 0.9), 0),       # 2: dominates 0
        ((9.0, 0.4, 90.0, 0.9), 0),        # 3: a trade-off against 2
        ((8.0, 0.9, 50.0, 1.0), -1),       # 4: would dominate everything, but failed
        ((8.5, nan, 95.0, 0.9), 0),        # 5: a NaN
        ((9.0, 0.5, 100.0, 0.95), 0),      # 6: dominates 2 through reliability alone
        ((9.0, 0.4, 90.0, 0.9), 0),        # 7: the same point as 3
        ((-0.0, 0.1, 500.0, 0.1), 0),      # 8
        ((0.0, 0.1, 500.0, 0.1), 0),       # 9: -0.0 equals +0.0: the same point as 8
        ((-inf, 0.0, inf, 0.0), 0),        # 10: best emissions, worst cost
        ((9.0, 0.5, 100.0, 0.95), -2),     # 11: failed
        ((20.0, 0.99, 100.0, 0.2), 0),     # 12: best opinion
        ((9.5, 0.45, 95.0, nan), 0),       # 13: a NaN in reliability: invalid whatever the mask
        ((9.0, 0.5, 90.0, 0.9), 0),        # 14: dominates 2 and 3
        ((9.0, 0.5, 90.0, 0.5), 0),        # 15: 14 with worse reliability
    ]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32)


def _filter(metrics, status, mask, chunk):
    fi, fm = np.zeros(0, np.int64), np.zeros((0, 4))
    for first in range(0, len(status), chunk):
        fi, fm = pareto_filter(fi, fm, np.arange(first, min(first + chunk, len(status))), metrics[first:first + chunk], status[first:first + chunk], mask)
    assert fm.tobytes() == metrics[fi].tobytes()      # (a row's metrics are its variant's, bit for bit)
    return fi.tolist()


def test_front_filter_on_crafted_metrics():
    metrics, status = _crafted()
    assert front_restated(metrics, status, 15) == [6, 8, 10, 12, 14]
    assert front_restated(metrics, status, 0b0111) == [8, 10, 12, 14]      # without reliability 14 dominates 6 and 15 is 14's point
    assert front_restated(metrics, status, 0b0001) == [10]
    assert front_restated(metrics, status, 0b1000) == [6]
    assert front_restated(metrics, status, 0b0100) == [3]                  # 3, 7, 14 and 15 cost 90: one point, held by the lowest
    for mask in range(1, 16):
        want = front_restated(metrics, status, mask)
        for chunk in (1, 3, 5, 16):
            assert _filter(metrics, status, mask, chunk) == want, (mask, chunk)


def test_front_filter_on_random_metrics_with_many_ties():
    rng = np.random.default_rng(4)
    for trial in range(30):
        n = int(rng.integers(1, 120))
        metrics = rng.integers(0, 4, (n, 4)).astype(np.float64)      # few distinct values: many equal points and ties
        metrics[rng.random(n) < 0.05, int(rng.integers(0, 4))] = np.nan
        status = np.where(rng.random(n) < 0.1, -1, 0).astype(np.int32)
        mask = int(rng.integers(1, 16))
        want = front_restated(metrics, status, mask)
        for chunk in (7, n):
            assert _filter(metrics, status, mask, chunk) == want, (trial, mask, chunk)


# ---------------------------------------------------------------- scripts/cross_front.py
def test_the_script_writes_the_front_and_its_plans(built, tmp_path):
    import csv
    import sys
    from eirgrid_amd.engine import CrossFront
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import cross_front as script
    finally:
        sys.path.pop(0)
    ps = _parents()
    crosses = cross_pairs(3)
    rows = [1, 3 + 11, 3 + 25 * 4 + 24]      # B itself, A>B cut at year 12, "empty">A cut at year 25
    assert [crosses[j] for j in rows] == [PlanCross(1, 1, 0, 0), PlanCross(0, 1, 12, 26), PlanCross(2, 0, 25, 26)]
    metrics = np.array([[1.5, 0.25, 1e10, 0.5], [-2.0, 0.75, 3e10 + 1, 1.0], [0.1, 1 / 3, 7.0, 0.0]])
    front = CrossFront(np.array(rows), [crosses[j] for j in rows], metrics, np.array([0.5, -1.25, 2.0]), np.array([True, False, False]), len(crosses), 140)
    d = script.write(str(tmp_path), ps, front)
    assert d == os.path.join(str(tmp_path), "cross")
    got = list(csv.reader(open(os.path.join(d, "index.csv"))))
    assert got[0] == ["variant", "a", "a_name", "b", "b_name", "cut", "net_emissions", "public_opinion", "total_cost", "power_reliability", "score", "is_parent"]
    assert got[1][:6] == ["1", "1", "B", "1", "B", ""] and got[1][-1] == "1"
    assert got[2][:6] == ["14", "0", "A", "1", "B", "2037"] and got[2][-1] == "0" and got[3][:6] == ["127", "2", "empty", "0", "A", "2050"]
    assert [float(v) for v in got[2][6:10]] == metrics[1].tolist() and got[2][8] == "30000000001" and float(got[3][10]) == 2.0
    plans = Plan.load(os.path.join(d, "plans.jsonl"))
    assert [p.name for p in plans] == ["B", "A>B@2037", "empty>A@2050"]
    assert plans == [apply_cross(ps, crosses[j]) for j in rows]
    assert script.years("2026,2050") == [2026, 2050]
    for bad in ("2025", "2051", "x", ""):
        with pytest.raises(Exception):
            script.years(bad)
