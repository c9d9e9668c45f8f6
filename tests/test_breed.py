"""CPU: the host side of eg_breed_plans (include/eirgrid_hip.h) — the struct layouts, every refusal of eg_breed_validate with its message,
BreedFront.lineage against lists written out by hand over two generations, and what scripts/breed_front.py writes and refuses."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import BREED_STOP, BreedFront, BreedGeneration, BreedMember, Plan, PlanCross, PlanSet
from tests.test_plan_crosses import _parents
from tests.test_plans import _empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "breed_front.py")


def _opts(mode=1, objectives=15, cap=256, max_generations=8, cuts=None, launch_variants=0, n_cuts=None):
    arr = np.array(list(cuts) if cuts else [0], np.uint8)
    n = (len(cuts) if cuts else 0) if n_cuts is None else n_cuts
    ptr = arr.ctypes.data_as(C.POINTER(C.c_uint8)) if cuts is not None else None
    return N.EgBreedOpts(mode, objectives, cap, max_generations, n, ptr, launch_variants), arr


def _validate(parents, **kw):
    L = N.lib()
    ps = PlanSet(parents) if parents is not None else None
    bo, keep = _opts(**kw)
    rc = L.eg_breed_validate(C.byref(ps.s) if ps is not None else None, C.byref(bo))
    return rc, L.eg_last_error().decode()


# ---------------------------------------------------------------- layout
def test_struct_layouts_are_the_headers(built):
    O, G, M = N.EgBreedOpts, N.EgBreedGeneration, N.EgBreedMember
    assert C.sizeof(O) == 40 and C.sizeof(G) == 40 and C.sizeof(M) == 56
    assert (O.mode.offset, O.objectives.offset, O.cap.offset, O.max_generations.offset, O.n_cuts.offset, O.cuts.offset, O.launch_variants.offset) == (0, 4, 8, 12, 16, 24, 32)
    assert (G.n_parents.offset, G.n_skipped.offset, G.n_kept.offset, G.n_children_kept.offset, G.n_variants.offset, G.n_valid.offset, G.n_dropped.offset) == \
           (0, 4, 8, 12, 16, 24, 32)
    assert (M.cross.offset, M.variant.offset, M.score.offset, M.metrics.offset) == (0, 8, 16, 24)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "typedef struct { int32_t mode , objectives , cap , max_generations ; int32_t n_cuts; const uint8_t *cuts ; int32_t launch_variants; } eg_breed_opts;" in flat
    assert "typedef struct { int32_t n_parents, n_skipped, n_kept, n_children_kept; int64_t n_variants, n_valid, n_dropped; } eg_breed_generation;" in flat
    assert "typedef struct { eg_plan_cross cross ; int32_t variant; double score, metrics[4]; } eg_breed_member;" in flat
    for k, name in enumerate(("EG_BREED_CONVERGED", "EG_BREED_MAX_GENERATIONS", "EG_BREED_EMPTY")):
        assert f"#define {name} {k}" in header
    assert (N.BREED_CONVERGED, N.BREED_MAX_GENERATIONS, N.BREED_EMPTY) == (0, 1, 2) and BREED_STOP == ("converged", "max_generations", "empty")
    assert "eg_breed_validate" in N.EXPORTS and "eg_breed_plans" in N.EXPORTS
    assert hasattr(N.lib(), "eg_breed_validate") and hasattr(N.lib(), "eg_breed_plans")


# ---------------------------------------------------------------- the validator
def test_validate_accepts_well_formed_options(built):
    ps = _parents()
    for kw in ({}, {"mode": 2, "objectives": 1, "cap": 1, "max_generations": 1, "cuts": (1, 25), "launch_variants": 1}, {"cuts": tuple(range(1, 26)), "launch_variants": 16384},
               {"cuts": (7, 7, 7)}):
        rc, msg = _validate(ps, **kw)
        assert rc == N.EG_OK, (kw, msg)
    assert _validate(ps[:1])[0] == N.EG_OK and _validate([ps[0]] * 256)[0] == N.EG_OK


@pytest.mark.parametrize("kw,expect", [
    ({"mode": 0}, "mode 0 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ({"mode": 3}, "mode 3 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ({"objectives": 0}, "objectives 0 is outside 1..15 (bit i = metric i)"),
    ({"objectives": 16}, "objectives 16 is outside 1..15 (bit i = metric i)"),
    ({"cap": 0}, "cap 0 is outside 1..EG_PARETO_MAX (256)"),
    ({"cap": 257}, "cap 257 is outside 1..EG_PARETO_MAX (256)"),
    ({"max_generations": 0}, "max_generations = 0 (at least 1)"),
    ({"max_generations": -2}, "max_generations = -2 (at least 1)"),
    ({"launch_variants": -1}, "launch_variants = -1 (1..16384; 0: 16384)"),
    ({"launch_variants": 16385}, "launch_variants = 16385 (1..16384; 0: 16384)"),
    ({"cuts": (5, 0)}, "cuts[1] = 0 (a year index 1..25)"),
    ({"cuts": (26,)}, "cuts[0] = 26 (a year index 1..25)"),
    ({"n_cuts": 3}, "NULL cuts with n_cuts = 3"),
    ({"n_cuts": -1}, "n_cuts = -1 (0..25; 0: every cut)"),
    ({"cuts": (5,), "n_cuts": 26}, "n_cuts = 26 (0..25; 0: every cut)"),
])
def test_validate_names_the_field(built, kw, expect):
    rc, msg = _validate(_parents(), **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_breed_validate: " + expect, msg


def test_validate_refuses_bad_parent_sets_and_null_options(built):
    ps = _parents()
    L = N.lib()
    rc, msg = _validate([ps[0]] * 257)
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_breed_validate: the set holds 257 plans (at most 256)", msg
    rc, msg = _validate(None)
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    rc, msg = _validate([])
    assert rc == N.EG_ERR_BAD_ARG and "n_plans" in msg, msg
    bad = _parents(); bad[1].best_actions[5][1] = 61
    rc, msg = _validate(bad)
    assert rc == N.EG_ERR_BAD_ARG and "plan 1" in msg and "61 >= 61" in msg, msg
    s = PlanSet(ps)
    assert L.eg_breed_validate(C.byref(s.s), None) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_breed_validate: NULL options"


def test_breed_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_breed_plans(None, None, None, None, None, 0, 0, None, None, None, None, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_breed_plans: bad argument" in L.eg_last_error().decode()


# ---------------------------------------------------------------- BreedFront.lineage
def _member(x, variant):
    return BreedMember(x, variant, 0.0, (0.0, 0.0, 0.0, 0.0))


def test_lineage_against_lists_written_out_by_hand():
    a, b, e = _parents()      # A, B, "empty" (tests/test_plan_crosses.py)
    # generation 0 keeps B itself, A>B cut at year 6 and empty>A cut at year 7; generation 1 keeps the second of those and its cross with the third at year 1
    g0 = [_member(PlanCross(1, 1, 0, 0), 1), _member(PlanCross(0, 1, 6, 26), 3 + 5), _member(PlanCross(2, 0, 7, 26), 3 + 4 * 25 + 6)]
    g1 = [_member(PlanCross(1, 1, 0, 0), 1), _member(PlanCross(1, 2, 1, 26), 3 + 3 * 25)]
    front = BreedFront([], np.zeros((2, 4)), np.zeros(2), [], [g0, g1], "max_generations")
    p0, p1, p2 = front.lineage([a, b, e])
    assert p0 == [a, b, e] and [p.name for p in p0] == ["A", "B", "empty"]
    assert [p.name for p in p1] == ["B", "A>B@2031", "empty>A@2032"]
    # A>B@2031: A's years 0..5, B's from 6 on
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[7] = [8]; run[24] = [30, 31, 32]
    dfc[0] = [24]; dfc[6] = [21]; dfc[7] = [24, 24]; dfc[25] = [60]
    ab = Plan(run, dfc)
    # empty>A@2032: nothing before year 7, A's from 7 on
    run = _empty(); dfc = _empty()
    run[7] = [9, 10, 11, 12]; run[25] = [45, 0]
    ea = Plan(run, dfc)
    assert p1 == [b, ab, ea]
    # generation 1: the second plan again, and its year 0 followed by empty>A@2032's years from 1 on
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[7] = [9, 10, 11, 12]; run[25] = [45, 0]
    dfc[0] = [24]
    assert p2 == [ab, Plan(run, dfc)]
    assert [p.name for p in p2] == ["A>B@2031", "A>B@2031>empty>A@2032@2026"]
    # a plan without a name goes by its position; a generation that kept nothing ends the lineage
    anon = [Plan(a.best_actions, a.best_deficit_actions), b]
    front = BreedFront([], np.zeros((0, 4)), np.zeros(0), [], [[_member(PlanCross(0, 1, 3, 26), 2)], []], "empty")
    line = front.lineage(anon)
    assert len(line) == 2 and [p.name for p in line[1]] == ["0>B@2028"]


# ---------------------------------------------------------------- scripts/breed_front.py
def test_the_script_writes_its_three_files(built, tmp_path):
    import csv
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import breed_front as script
    finally:
        sys.path.pop(0)
    a, b, e = _parents()
    kept = [_member(PlanCross(1, 1, 0, 0), 1), _member(PlanCross(0, 1, 12, 26), 3 + 11)]
    metrics = np.array([[1.5, 0.25, 1e10, 0.5], [-2.0, 0.75, 3e10 + 1, 1.0]])
    front = BreedFront([], metrics, np.array([0.5, -1.25]), [BreedGeneration(3, 0, 2, 1, 153, 140, 0)], [kept], "max_generations")
    front.plans = front.lineage([a, b, e])[-1]
    d = script.write(str(tmp_path), front)
    assert d == os.path.join(str(tmp_path), "breed") and sorted(os.listdir(d)) == ["generations.csv", "index.csv", "plans.jsonl"]
    got = list(csv.reader(open(os.path.join(d, "index.csv"))))
    assert got[0] == ["plan", "name", "variant", "a", "b", "cut", "net_emissions", "public_opinion", "total_cost", "power_reliability", "score"]
    assert got[1][:6] == ["0", "B", "1", "1", "1", ""] and got[2][:6] == ["1", "A>B@2037", "14", "0", "1", "2037"]
    assert [float(v) for v in got[2][6:10]] == metrics[1].tolist() and got[2][8] == "30000000001" and float(got[2][10]) == -1.25
    gens = list(csv.reader(open(os.path.join(d, "generations.csv"))))
    assert gens == [["generation", "n_parents", "n_skipped", "n_variants", "n_valid", "n_kept", "n_children_kept", "n_dropped", "stop"],
                    ["0", "3", "0", "153", "140", "2", "1", "0", "max_generations"]]
    plans = Plan.load(os.path.join(d, "plans.jsonl"))
    assert plans == front.plans and [p.name for p in plans] == ["B", "A>B@2037"]


@pytest.mark.parametrize("args,expect", [
    (["--cuts", "2025"], "argument --cuts: a comma-separated list of at most 25 years 2026..2050"),
    (["--cuts", "2030,x"], "argument --cuts: a comma-separated list of at most 25 years 2026..2050"),
    (["--generations", "0"], "argument --generations: a number of generations 1..1024"),
    (["--cap", "257"], "argument --cap: a population size 1..256"),
    (["--cap", "none"], "argument --cap: a population size 1..256"),
    ([], None),
])
def test_the_script_refuses_bad_arguments(tmp_path, args, expect):
    base = ["--world", "synthetic", "--plans", str(tmp_path / "none.jsonl"), "--seed", "1", "--out", str(tmp_path / "out")] if expect else ["--world", "synthetic"]
    run = subprocess.run([sys.executable, SCRIPT] + base + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 2, run.stdout + run.stderr
    assert (expect or "the following arguments are required: --plans, --seed, --out") in run.stderr, run.stderr
    assert not os.path.exists(tmp_path / "out")


def test_the_script_refuses_more_than_256_plans(built, tmp_path):
    a = _parents()[0]
    path = str(tmp_path / "many.jsonl")
    Plan.save(path, [Plan(a.best_actions, a.best_deficit_actions, f"p{k}") for k in range(257)])
    run = subprocess.run([sys.executable, SCRIPT, "--world", "synthetic", "--plans", path, "--seed", "1", "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "--plans holds 257 plans (at most 256)" in run.stderr, run.stdout + run.stderr
