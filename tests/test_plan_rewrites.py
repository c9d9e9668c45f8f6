"""CPU: the host side of plan rewrites (include/eirgrid_hip.h eg_evaluate_plan_rewrites) — the struct layouts, what the validator accepts
and refuses, the ActionMap constructors, PlanRewrite.apply against lists written out by hand and a restatement written out here
(`apply_rewrite`, which the GPU tests import), the variants of Engine.technology_report (engine.technology_rewrites), and what
scripts/plan_technologies.py writes."""
import ctypes as C
import os

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionMap, Plan, PlanRewrite, PlanSet, TechnologyRow, _map_array, _rewrite_array, technology_rewrites
from tests.test_plans import _empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = 0xFF


def apply_rewrite(plans, maps, rw):
    """Rewrite rw over `plans` and `maps`, written out once more (not PlanRewrite.apply: the tests' own restatement), entry by entry"""
    src = plans[rw.plan]
    to = maps[rw.map].to
    out = []
    for bit, lists in enumerate((src.best_actions, src.best_deficit_actions)):
        new = []
        for y in range(26):
            year = []
            for e in lists[y]:
                if (rw.lists & (1 << bit)) == 0 or y < rw.from_year or y >= rw.to_year:
                    year.append(e)
                elif to[e] != DROP:
                    year.append(to[e])
            new.append(year)
        out.append(new)
    return Plan(out[0], out[1], src.name)


def _plans():
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[6] = [3]; run[7] = [9, 10, 11, 12]; run[25] = [45, 0]
    dfc[0] = [24]; dfc[6] = [24, 60, 21]
    a = Plan(run, dfc, "A")
    run = _empty(); dfc = _empty()
    run[0] = [1]; run[5] = [2, 2]; run[7] = [8]; run[24] = [30, 31, 32]
    dfc[6] = [21]; dfc[7] = [24, 24]; dfc[25] = [60]
    b = Plan(run, dfc, "B")
    return [a, b, Plan(_empty(), _empty(), "empty")]


def _validate(plans, maps, rewrites, n_maps=None, n=None):
    L = N.lib()
    ps = PlanSet(plans) if plans is not None else None
    marr, m = _map_array(maps)
    arr, k = _rewrite_array(rewrites)
    rc = L.eg_plan_rewrites_validate(C.byref(ps.s) if ps is not None else None, marr, m if n_maps is None else n_maps, arr, k if n is None else n)
    return rc, L.eg_last_error().decode()


def _raw_map(to):
    return N.EgActionMap((C.c_uint8 * 61)(*to))


# ---------------------------------------------------------------- layout
def test_struct_layouts_are_the_headers(built):
    M, R = N.EgActionMap, N.EgPlanRewrite
    assert C.sizeof(M) == 61 and C.sizeof(R) == 8
    assert (R.plan.offset, R.map.offset, R.from_year.offset, R.to_year.offset, R.lists.offset, R.pad.offset) == (0, 2, 4, 5, 6, 7)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert "typedef struct { uint8_t to[EG_N_ACTIONS]; } eg_action_map;" in header
    assert "typedef struct { uint16_t plan, map; uint8_t from_year, to_year, lists, pad; } eg_plan_rewrite;" in header
    assert "#define EG_REWRITE_DROP 0xFF" in header and "#define EG_REWRITE_MAX_MAPS 256" in header and "#define EG_REWRITE_MAX_VARIANTS 16384" in header
    assert (N.REWRITE_DROP, N.REWRITE_MAX_MAPS, N.REWRITE_MAX_VARIANTS) == (255, 256, 16384)
    assert "eg_plan_rewrites_validate" in N.EXPORTS and "eg_evaluate_plan_rewrites" in N.EXPORTS
    # the library's side of the two sizes: it steps through the arrays as ctypes laid them out, and names the third of each
    maps = [ActionMap.identity(), ActionMap.drop_all(), _raw_map([0] * 60 + [99])]
    rc, msg = _validate(_plans(), maps, [PlanRewrite()])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_rewrites_validate: map 2: to[60] = 99 (0..60 or 0xFF drop)", msg
    rc, msg = _validate(_plans(), maps[:2], [PlanRewrite(0, 1, 3, 26), PlanRewrite(1, 0, 0, 1, 3), PlanRewrite(1, 1, 9, 8)])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_rewrites_validate: rewrite 2: from_year 9 > to_year 8", msg


# ---------------------------------------------------------------- ActionMap
def test_the_map_constructors():
    ident = list(range(61))
    assert list(ActionMap.identity().to) == ident
    assert list(ActionMap.drop_all().to) == [DROP] * 61
    want = list(ident); want[7] = DROP; want[60] = DROP
    assert list(ActionMap.drop([60, 7]).to) == want
    want = list(ident); want[3] = 0; want[24] = 36
    assert list(ActionMap.substitute({3: 0, 24: 36}).to) == want
    want = list(ident); want[15:18] = [DROP] * 3
    assert list(ActionMap.drop_technology(5).to) == want      # Nuclear
    want = list(ident); want[3:6] = [0, 1, 2]
    assert list(ActionMap.replace_technology(1, 0).to) == want      # offshore wind built as onshore, tier kept
    for k in range(3):
        assert list(ActionMap.cost_tier(k).to) == [3 * (a // 3) + k for a in range(57)] + [57, 58, 59, 60]
    for bad in ([0] * 60, [0] * 62, [61] + [0] * 60, [-1] + [0] * 60, [254] + [0] * 60):
        with pytest.raises(ValueError):
            ActionMap(tuple(bad))
    with pytest.raises(ValueError):
        ActionMap.cost_tier(3)
    assert bytes(ActionMap.drop([2]).struct().to) == bytes([0, 1, DROP] + ident[3:])
    assert ActionMap.identity() == ActionMap(tuple(ident)) and hash(ActionMap.identity()) == hash(ActionMap(ident))


# ---------------------------------------------------------------- PlanRewrite.apply
def test_apply_against_lists_written_out_by_hand():
    ps = _plans()
    a = ps[0]
    maps = [ActionMap.identity(), ActionMap.drop([12]), ActionMap.substitute({24: 36, 12: 0}), ActionMap.drop_all(), ActionMap.cost_tier(0)]
    # 12 dropped from best_actions in every year: two entries go, the order of the others stays
    got = PlanRewrite(0, 1).apply(ps, maps)
    run = [list(l) for l in a.best_actions]; run[0] = [5, 60]; run[7] = [9, 10, 11]
    assert (got.best_actions, got.best_deficit_actions) == (run, a.best_deficit_actions) and got.name == "A" and len(got) == len(a) - 2
    # ... in the years 1..7 only (to_year is exclusive: year 7 is outside)
    assert PlanRewrite(0, 1, 1, 7).apply(ps, maps) == a
    got = PlanRewrite(0, 1, 1, 8).apply(ps, maps)
    run = [list(l) for l in a.best_actions]; run[7] = [9, 10, 11]
    assert got.best_actions == run
    # a substitution on both lists
    got = PlanRewrite(0, 2, 0, 26, 3).apply(ps, maps)
    run = [list(l) for l in a.best_actions]; run[0] = [5, 0, 60]; run[7] = [9, 10, 11, 0]
    dfc = [list(l) for l in a.best_deficit_actions]; dfc[0] = [36]; dfc[6] = [36, 60, 21]
    assert (got.best_actions, got.best_deficit_actions) == (run, dfc)
    # ... on the deficit list alone
    got = PlanRewrite(0, 2, 0, 26, 2).apply(ps, maps)
    assert (got.best_actions, got.best_deficit_actions) == (a.best_actions, dfc)
    # nothing built from 2032 on (year 7); the deficit list stays
    got = PlanRewrite(0, 3, 7, 26).apply(ps, maps)
    assert got.best_actions == a.best_actions[:7] + [[] for _ in range(19)] and got.best_deficit_actions == a.best_deficit_actions
    # every plant at the first cost tier
    got = PlanRewrite(0, 4).apply(ps, maps)
    run = _empty(); run[0] = [3, 12, 60]; run[6] = [3]; run[7] = [9, 9, 9, 12]; run[25] = [45, 0]
    assert got.best_actions == run
    assert ps[0] == _plans()[0]      # (a copy: the plan is left alone)
    got.best_actions[25].append(1)
    assert ps[0].best_actions[25] == [45, 0]


def test_identities_are_the_plan():
    ps = _plans()
    maps = [ActionMap.identity(), ActionMap.drop_all(), ActionMap.drop([4, 13, 59])]      # (the third drops nothing that occurs)
    for rw in (PlanRewrite(0, 0, 0, 26, 3), PlanRewrite(0, 1, 0, 26, 0), PlanRewrite(1, 1, 9, 9, 3), PlanRewrite(1, 1, 26, 26, 3), PlanRewrite(0, 2, 0, 26, 3),
               PlanRewrite(2, 1, 0, 26, 3), PlanRewrite(0, 1, 1, 6, 1)):
        assert rw.apply(ps, maps) == ps[rw.plan] and apply_rewrite(ps, maps, rw) == ps[rw.plan], rw
        assert _validate(ps, maps, [rw])[0] == N.EG_OK


def _random_map(rng):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return ActionMap.identity()
    if kind == 1:
        return ActionMap.drop(rng.integers(0, 61, int(rng.integers(1, 30))).tolist())
    if kind == 2:
        return ActionMap.cost_tier(int(rng.integers(0, 3)))
    if kind == 3:
        return ActionMap(tuple(int(t) if t < 61 else DROP for t in rng.integers(0, 80, 61)))
    return ActionMap.drop_all()


def test_apply_on_random_rewrites_is_the_restatement(built):
    rng = np.random.default_rng(8)
    for _ in range(200):
        ps = [Plan([[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 5)))] for _ in range(26)],
                   [[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 3)))] for _ in range(26)], f"p{k}") for k in range(3)]
        maps = [_random_map(rng) for _ in range(3)]
        to = int(rng.integers(0, 27))
        rw = PlanRewrite(int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, to + 1)), to, int(rng.integers(0, 4)))
        got = rw.apply(ps, maps)
        assert got == apply_rewrite(ps, maps, rw) and got.name == ps[rw.plan].name, rw
        assert len(got) <= len(ps[rw.plan]) and all(len(g) <= len(l) for g, l in zip(got.best_deficit_actions, ps[rw.plan].best_deficit_actions))
        assert _validate(ps, maps, [rw])[0] == N.EG_OK


# ---------------------------------------------------------------- eg_plan_rewrites_validate
def test_validate_accepts_every_well_formed_rewrite(built):
    ps = _plans()
    maps = [ActionMap.identity(), ActionMap.drop_all(), ActionMap.cost_tier(2)]
    rewrites = [PlanRewrite(p, m, f, t, l) for p in range(3) for m in range(3) for t in range(27) for f in range(t + 1) for l in range(4) if (p + m + f + t + l) % 5 == 0]
    rc, msg = _validate(ps, maps, rewrites)
    assert rc == N.EG_OK, msg
    full = [[60] * 157 for _ in range(26)]
    full[0] = full[0] + [60] * (4096 - 26 * 157)
    assert _validate([Plan(full, full)], maps, [PlanRewrite(0, 1, 3, 9, 3), PlanRewrite(0, 2, 0, 26, 3)])[0] == N.EG_OK
    assert _validate([ps[0]] * 256, [ActionMap.identity()] * 256, [PlanRewrite(255, 255, 1, 26, 3)])[0] == N.EG_OK
    assert _validate(ps, maps, [PlanRewrite()] * 16384)[0] == N.EG_OK


@pytest.mark.parametrize("rewrite, expect", [
    (PlanRewrite(3, 0, 0, 1), "rewrite 2: plan 3 >= n_plans 3"),
    (PlanRewrite(65535, 0, 0, 0), "rewrite 2: plan 65535 >= n_plans 3"),
    (PlanRewrite(0, 2, 0, 1), "rewrite 2: map 2 >= n_maps 2"),
    (PlanRewrite(0, 1, 0, 27), "rewrite 2: to_year 27 (at most 26)"),
    (PlanRewrite(0, 1, 27, 27), "rewrite 2: to_year 27 (at most 26)"),
    (PlanRewrite(0, 1, 5, 4), "rewrite 2: from_year 5 > to_year 4"),
    (PlanRewrite(0, 0, 26, 0), "rewrite 2: from_year 26 > to_year 0"),
    (PlanRewrite(0, 0, 0, 26, 4), "rewrite 2: lists 4 (bit 0 best_actions, bit 1 best_deficit_actions)"),
    (N.EgPlanRewrite(0, 0, 0, 26, 1, 7), "rewrite 2: pad 7 (must be 0)"),
])
def test_validate_names_the_rewrite_and_the_field(built, rewrite, expect):
    rc, msg = _validate(_plans(), [ActionMap.identity(), ActionMap.drop_all()], [PlanRewrite(0, 1, 1, 26), PlanRewrite(1, 1, 0, 0, 3), rewrite])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_rewrites_validate: " + expect, msg


@pytest.mark.parametrize("entry, value", [(17, 200), (0, 61), (60, 254), (3, 64)])
def test_validate_names_the_map_and_the_entry(built, entry, value):
    to = list(range(61)); to[entry] = value
    maps = [ActionMap.identity(), ActionMap.drop_all(), ActionMap.cost_tier(1), _raw_map(to)]
    rc, msg = _validate(_plans(), maps, [PlanRewrite()])      # (a map no rewrite uses is checked all the same)
    assert rc == N.EG_ERR_BAD_ARG and msg == f"eg_plan_rewrites_validate: map 3: to[{entry}] = {value} (0..60 or 0xFF drop)", msg
    assert _validate(_plans(), maps, [PlanRewrite()], n_maps=3)[0] == N.EG_OK      # (the fourth is not looked at)


def test_validate_refuses_bad_counts_null_arrays_and_bad_sets(built):
    ps = _plans()
    maps = [ActionMap.identity()]
    L = N.lib()
    for n in (0, -3, 16385):
        rc, msg = _validate(ps, maps, [PlanRewrite()], n=n)
        assert rc == N.EG_ERR_BAD_ARG and msg == f"eg_plan_rewrites_validate: n_rewrites = {n} (1..16384)", msg
    for n in (0, -1, 257):
        rc, msg = _validate(ps, maps, [PlanRewrite()], n_maps=n)
        assert rc == N.EG_ERR_BAD_ARG and msg == f"eg_plan_rewrites_validate: n_maps = {n} (1..256)", msg
    s = PlanSet(ps)
    marr, _ = _map_array(maps)
    arr, _ = _rewrite_array([PlanRewrite()])
    assert L.eg_plan_rewrites_validate(C.byref(s.s), marr, 1, None, 1) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_rewrites_validate: NULL rewrites"
    assert L.eg_plan_rewrites_validate(C.byref(s.s), None, 1, arr, 1) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_rewrites_validate: NULL maps"
    rc, msg = _validate([ps[0]] * 257, maps, [PlanRewrite()])
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_plan_rewrites_validate: the set holds 257 plans (at most 256)", msg
    rc, msg = _validate(None, maps, [PlanRewrite()])
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    rc, msg = _validate([], maps, [PlanRewrite()])
    assert rc == N.EG_ERR_BAD_ARG and "n_plans" in msg, msg
    bad = _plans(); bad[1].best_actions[5][1] = 61
    rc, msg = _validate(bad, maps, [PlanRewrite()])
    assert rc == N.EG_ERR_BAD_ARG and "plan 1" in msg and "61 >= 61" in msg, msg


def test_evaluate_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_evaluate_plan_rewrites(None, None, None, None, None, 1, None, 1, 0, 0, 1, None) == N.EG_ERR_BAD_ARG
    assert "eg_evaluate_plan_rewrites: bad argument" in L.eg_last_error().decode()


# ---------------------------------------------------------------- the variants of technology_report
def test_technology_rewrites_per_plan_the_plan_then_every_type_it_uses():
    ps = _plans()      # A uses the types 0 (action 0), 1 (3, 5), 3 (9, 10, 11), 4 (12, 12); 45 is an offset and 60 has no type; B 0, 2, 10
    parents, maps, rewrites, rows = technology_rewrites(ps, "keep")
    assert parents == ps and maps[0] == ActionMap.identity()
    assert rows == [(0, -1, 0), (0, 0, 1), (0, 1, 2), (0, 3, 3), (0, 4, 2), (1, -1, 0), (1, 0, 3), (1, 2, 1), (1, 10, 3), (2, -1, 0)]
    for rw, (p, t, removed) in zip(rewrites, rows):
        child = apply_rewrite(parents, maps, rw)
        assert rw.plan == p and child.best_deficit_actions == ps[p].best_deficit_actions and len(child) == len(ps[p]) - removed
        assert all(a // 3 != t for l in child.best_actions for a in l)
    assert len(maps) == 1 + 6 and len({rw.map for rw in rewrites}) == 7      # (types 0, 1, 3, 4, 2, 10: a map each, shared between the plans)
    # substitute: A's deficit list holds type 8 (24) and 7 (21), which best_actions does not use: nothing to substitute, no extra parent
    parents, maps, rewrites, rows2 = technology_rewrites(ps, "substitute")
    assert parents == ps and rows2 == rows
    # ... a plan whose deficit list holds a type best_actions uses: the substituted plan rides as a parent of its own
    run = _empty(); dfc = _empty()
    run[0] = [24, 15]; run[3] = [26]; dfc[0] = [24, 36]; dfc[9] = [25, 15, 60]
    g = Plan(run, dfc, "G")
    parents, maps, rewrites, rows = technology_rewrites([ps[0], g], "substitute", 36)
    assert rows[5:] == [(1, -1, 0), (1, 5, 1), (1, 8, 2)] and len(parents) == 4 and parents[:2] == [ps[0], g]
    kids = [apply_rewrite(parents, maps, rw) for rw in rewrites[5:]]
    assert kids[0] == g and kids[0].name == "G"
    assert kids[1].best_actions[0] == [24] and kids[1].best_deficit_actions[9] == [25, 36, 60] and kids[1].best_deficit_actions[0] == [24, 36]
    assert kids[2].best_actions == [[15]] + _empty()[1:] and kids[2].best_deficit_actions[0] == [36, 36] and kids[2].best_deficit_actions[9] == [36, 15, 60]
    assert all(k.name == "G" for k in kids)
    for bad in ({"deficit": "drop"}, {"substitute_with": 61}, {"substitute_with": -1}):
        with pytest.raises(ValueError):
            technology_rewrites(ps, **bad)


# ---------------------------------------------------------------- scripts/plan_technologies.py
def test_the_script_writes_the_report_and_its_plans(built, tmp_path):
    import csv
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import plan_technologies as script
    finally:
        sys.path.pop(0)
    ps = _plans()[:2]
    parents, maps, rewrites, rows = technology_rewrites(ps, "keep")
    metrics = np.arange(4.0 * len(rows)).reshape(-1, 4) + 0.5
    report = [TechnologyRow(p, t, r, 0, tuple(metrics[j]), float(j), float(j) - (0.0 if p == 0 else 5.0)) for j, (p, t, r) in enumerate(rows)]
    replaced = [(0, 1, 0, PlanRewrite(0, 0).apply(ps, [ActionMap.replace_technology(1, 0)]), TechnologyRow(0, 1, 2, 0, (1.0, 2.0, 3.0, 4.0), 7.0, 7.0))]
    d = script.write(str(tmp_path), ps, report, replaced)
    assert d == os.path.join(str(tmp_path), "technologies")
    got = list(csv.reader(open(os.path.join(d, "index.csv"))))
    assert got[0] == ["plan", "plan_name", "technology", "replaced_by", "removed", "status", "net_emissions", "public_opinion", "total_cost", "power_reliability",
                      "score", "delta"]
    assert got[1][:5] == ["0", "A", "", "", "0"] and got[2][:5] == ["0", "A", "OnshoreWind", "", "1"] and got[3][:5] == ["0", "A", "OffshoreWind", "", "2"]
    assert got[6][:5] == ["1", "B", "", "", "0"] and got[-2][:5] == ["1", "B", "HydroDam", "", "3"]
    assert got[-1][:5] == ["0", "A", "OffshoreWind", "OnshoreWind", "2"] and float(got[-1][10]) == 7.0
    assert [float(v) for v in got[2][6:10]] == metrics[1].tolist() and float(got[7][11]) == 1.0
    plans = Plan.load(os.path.join(d, "plans.jsonl"))
    assert [p.name for p in plans] == ["A", "A-OnshoreWind", "A-OffshoreWind", "A-CommercialSolar", "A-UtilitySolar", "B", "B-OnshoreWind", "B-DomesticSolar",
                                       "B-HydroDam", "A:OffshoreWind>OnshoreWind"]
    assert plans[:-1] == [apply_rewrite(parents, maps, rw) for rw in rewrites] and plans[-1] == replaced[0][3]
    assert script.replacements("1:0,5:12") == [(1, 0), (5, 12)] and script.replacements("OffshoreWind:OnshoreWind") == [(1, 0)]
    for bad in ("1", "15:0", "x:y", "1:1"):
        with pytest.raises(Exception):
            script.replacements(bad)
