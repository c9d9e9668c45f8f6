"""CPU: the host side of eg_explore_plans (include/eirgrid_hip.h) — the struct layouts, every refusal of eg_explore_validate with its
message, eg_explore_neighbourhood against the enumerations of engine.py, ExploreFront.lineage against lists written out by hand, and
what scripts/explore_front.py refuses."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import EXPLORE_STOP, ExploreFront, ExploreMember, Plan, PlanEdit, PlanMove, PlanSet, refine_edits, refine_moves
from tests.test_plan_crosses import _parents
from tests.test_plans import _empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "explore_front.py")


def _opts(mode=1, objectives=15, cap=256, max_generations=8, replace_with=None, append_with=None, max_shift=0, launch_variants=0, max_variants=0,
          n_replace=None, n_append=None):
    rep = np.array(list(replace_with) if replace_with else [0], np.uint8)
    app = np.array(list(append_with) if append_with else [0], np.uint8)
    ptr = lambda arr, given: arr.ctypes.data_as(C.POINTER(C.c_uint8)) if given is not None else None
    xo = N.EgExploreOpts(mode, objectives, cap, max_generations, (len(replace_with) if replace_with else 0) if n_replace is None else n_replace,
                         ptr(rep, replace_with), (len(append_with) if append_with else 0) if n_append is None else n_append, ptr(app, append_with),
                         max_shift, launch_variants, max_variants)
    return xo, (rep, app)


def _validate(starts, **kw):
    L = N.lib()
    ps = PlanSet(starts) if starts is not None else None
    xo, keep = _opts(**kw)
    rc = L.eg_explore_validate(C.byref(ps.s) if ps is not None else None, C.byref(xo))
    return rc, L.eg_last_error().decode()


# ---------------------------------------------------------------- layout
def test_struct_layouts_are_the_headers(built):
    O, G, M = N.EgExploreOpts, N.EgExploreGeneration, N.EgExploreMember
    assert C.sizeof(O) == 64 and C.sizeof(G) == 40 and C.sizeof(M) == 88
    assert (O.mode.offset, O.objectives.offset, O.cap.offset, O.max_generations.offset, O.n_replace.offset, O.replace_with.offset, O.n_append.offset,
            O.append_with.offset, O.max_shift.offset, O.launch_variants.offset, O.max_variants.offset) == (0, 4, 8, 12, 16, 24, 32, 40, 48, 52, 56)
    assert (G.n_frontier.offset, G.n_held.offset, G.n_new.offset, G.n_variants.offset, G.n_valid.offset, G.n_dropped.offset) == (0, 4, 8, 16, 24, 32)
    assert (M.parent.offset, M.is_move.offset, M.edit.offset, M.move.offset, M.number.offset, M.score.offset, M.metrics.offset) == (0, 8, 12, 24, 40, 48, 56)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("typedef struct { int32_t mode , objectives , cap , max_generations ; int32_t n_replace; const uint8_t *replace_with; int32_t n_append; "
            "const uint8_t *append_with; int32_t max_shift , launch_variants; int64_t max_variants ; } eg_explore_opts;") in flat
    assert "typedef struct { int32_t n_frontier, n_held, n_new, pad; int64_t n_variants, n_valid, n_dropped; } eg_explore_generation;" in flat
    assert "typedef struct { int64_t parent ; int32_t is_move; eg_plan_edit edit; eg_plan_move move; int64_t number; double score, metrics[4]; } eg_explore_member;" in flat
    for k, name in enumerate(("EG_EXPLORE_EXPLORED", "EG_EXPLORE_MAX_GENERATIONS", "EG_EXPLORE_EMPTY", "EG_EXPLORE_BUDGET")):
        assert f"#define {name} {k}" in header
    assert (N.EXPLORE_EXPLORED, N.EXPLORE_MAX_GENERATIONS, N.EXPLORE_EMPTY, N.EXPLORE_BUDGET) == (0, 1, 2, 3)
    assert EXPLORE_STOP == ("explored", "max_generations", "empty", "budget")
    for name in ("eg_explore_validate", "eg_explore_neighbourhood", "eg_explore_plans"):
        assert name in N.EXPORTS and hasattr(N.lib(), name)


# ---------------------------------------------------------------- the validator
def test_validate_accepts_well_formed_options(built):
    ps = _parents()
    for kw in ({}, {"mode": 2, "objectives": 1, "cap": 1, "max_generations": 1, "replace_with": (0, 60), "append_with": (60,), "max_shift": 25, "launch_variants": 1,
                    "max_variants": 1}, {"launch_variants": 16384, "max_variants": 2**40}, {"replace_with": (7, 7, 7)}):
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
    ({"n_replace": -1}, "n_replace = -1"),
    ({"n_append": -3}, "n_append = -3"),
    ({"n_replace": 2}, "NULL replace_with with n_replace = 2"),
    ({"n_append": 1}, "NULL append_with with n_append = 1"),
    ({"replace_with": (5, 61)}, "replace_with[1]: action 61 >= 61"),
    ({"append_with": (255,)}, "append_with[0]: action 255 >= 61"),
    ({"max_shift": -1}, "max_shift = -1 (0..25 years; 0: no moves)"),
    ({"max_shift": 26}, "max_shift = 26 (0..25 years; 0: no moves)"),
    ({"launch_variants": -1}, "launch_variants = -1 (1..16384; 0: 16384)"),
    ({"launch_variants": 16385}, "launch_variants = 16385 (1..16384; 0: 16384)"),
    ({"max_variants": -1}, "max_variants = -1 (0: no budget)"),
])
def test_validate_names_the_field(built, kw, expect):
    rc, msg = _validate(_parents(), **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_explore_validate: " + expect, msg


def test_validate_refuses_bad_start_sets_and_null_options(built):
    ps = _parents()
    L = N.lib()
    rc, msg = _validate([ps[0]] * 257)
    assert rc == N.EG_ERR_BAD_ARG and msg == "eg_explore_validate: the set holds 257 plans (at most 256)", msg
    rc, msg = _validate(None)
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    rc, msg = _validate([])
    assert rc == N.EG_ERR_BAD_ARG and "n_plans" in msg, msg
    bad = _parents(); bad[1].best_actions[5][1] = 61
    rc, msg = _validate(bad)
    assert rc == N.EG_ERR_BAD_ARG and "plan 1" in msg and "61 >= 61" in msg, msg
    s = PlanSet(ps)
    assert L.eg_explore_validate(C.byref(s.s), None) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_explore_validate: NULL options"


def test_explore_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_explore_plans(None, None, None, None, None, 0, 0, None, None, None, None, None, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_explore_plans: bad argument" in L.eg_last_error().decode()
    s = PlanSet(_parents())
    xo, keep = _opts()
    assert L.eg_explore_neighbourhood(C.byref(s.s), C.byref(xo), None) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_explore_neighbourhood: NULL sizes"
    xo, keep = _opts(max_shift=26)
    sizes = (C.c_int64 * 3)()
    assert L.eg_explore_neighbourhood(C.byref(s.s), C.byref(xo), sizes) == N.EG_ERR_BAD_ARG and "max_shift = 26" in L.eg_last_error().decode()


# ---------------------------------------------------------------- the neighbourhood
def _full():
    """best_actions at the 4 096-entry capacity (no appends), a few deficit entries"""
    rng = np.random.default_rng(5)
    run = [[int(a) for a in rng.integers(0, 61, 150)] for _ in range(26)]
    run[13] = []
    run[3] += [int(a) for a in rng.integers(0, 61, 4096 - 25 * 150)]
    dfc = _empty(); dfc[0] = [24, 21]; dfc[25] = [60]
    plan = Plan(run, dfc, "full")
    assert len(plan) == 4096
    return plan


@pytest.mark.parametrize("kw", [{}, {"replace_with": (3, 17)}, {"append_with": (9, 9, 60)}, {"replace_with": (1,), "append_with": (2, 3), "max_shift": 1},
                                {"max_shift": 25}, {"replace_with": (4, 5, 6), "append_with": (7,), "max_shift": 25}])
def test_neighbourhood_sizes_are_the_enumerations(built, kw):
    a, b, empty = _parents()
    one = Plan([[17]] + _empty()[1:], _empty(), "one entry")
    last = Plan(_empty()[:25] + [[3]], _empty(), "one entry in the last year")
    starts = [a, b, empty, one, last, _full()]
    xo, keep = _opts(**kw)
    s = PlanSet(starts)
    sizes = (C.c_int64 * len(starts))()
    assert N.lib().eg_explore_neighbourhood(C.byref(s.s), C.byref(xo), sizes) == N.EG_OK, N.lib().eg_last_error().decode()
    want = [len(refine_edits(p, kw.get("replace_with"), kw.get("append_with"))) - 1 + len(refine_moves(p, kw.get("max_shift", 0))) for p in starts]
    assert list(sizes) == want, (kw, list(sizes), want)
    n_app = 26 * len(kw.get("append_with", ()))
    assert want[2] == n_app      # the empty plan: appends only
    shifts = min(kw.get("max_shift", 0), 25)
    assert want[3] == 1 + len(kw.get("replace_with", ())) + n_app + shifts == want[4]      # one entry: a delete, its replaces, the appends, the moves one way
    assert want[5] == 4096 + 3 + 4096 * len(kw.get("replace_with", ())) + len(refine_moves(starts[5], kw.get("max_shift", 0)))      # a full list: no appends


# ---------------------------------------------------------------- ExploreFront.lineage
def _member(parent, edit, number):
    return ExploreMember(parent, edit, number, 0.0, (0.0, 0.0, 0.0, 0.0))


def test_lineage_against_lists_written_out_by_hand():
    a, b, e = _parents()      # A, B, "empty" (tests/test_plan_crosses.py)
    # generation 0 holds B of the start plans, and A without its entry 2031.0, and "empty" with action 9 appended to 2040; generation 1 the
    # second of those with its entry 2032.3 moved to 2034, generation 2 that one with its deficit entry 2031.1 replaced... by a delete
    rows = [[_member(-1, PlanEdit(), 1)],
            [_member(0, PlanEdit("delete", 0, 6, 0), 40), _member(2, PlanEdit("insert", 0, 15, 0, 9), 77)],
            [_member(40, PlanMove(0, 7, 3, 9, 0), 130)],
            [_member(130, PlanEdit("delete", 1, 6, 1), 200)]]
    front = ExploreFront([], np.array([1, 77, 200]), np.zeros((3, 4)), np.zeros(3), [], rows, "explored")
    l0, l1, l2, l3 = front.lineage([a, b, e])
    assert sorted(l0) == [0, 1, 2] and [l0[k] for k in range(3)] == [a, b, e] and [l0[k].name for k in range(3)] == ["A", "B", "empty"]
    assert sorted(l1) == [0, 1, 2, 40, 77] and sorted(l2) == [0, 1, 2, 40, 77, 130] and sorted(l3) == [0, 1, 2, 40, 77, 130, 200]
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[7] = [9, 10, 11, 12]; run[25] = [45, 0]
    dfc[0] = [24]; dfc[6] = [24, 60, 21]
    assert l1[40] == Plan(run, dfc) and l1[40].name == "A-2031.0"
    run15 = _empty(); run15[15] = [9]
    assert l1[77] == Plan(run15, _empty()) and l1[77].name == "empty+2040=9"
    run[7] = [9, 10, 11]; run[9] = [12]
    assert l2[130] == Plan(run, dfc) and l2[130].name == "A-2031.0:2032.3>2034"
    dfc[6] = [24, 21]
    assert l3[200] == Plan(run, dfc) and l3[200].name == "A-2031.0:2032.3>2034-d2031.1"
    assert l3[40] == l1[40] and l2[77] == l1[77]      # (what is known stays)
    assert ExploreFront([], np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros(0), [], [], "empty").lineage([a, b]) == []


# ---------------------------------------------------------------- the script's arguments
@pytest.mark.parametrize("args,expect", [
    (["--replace", "3,61"], "a comma-separated list of canonical action indices 0..60"),
    (["--append", "x"], "a comma-separated list of canonical action indices 0..60"),
    (["--shift", "26"], "a number of years 0..25"),
    (["--cap", "0"], "a front size 1..256"),
    (["--generations", "0"], "a number of generations 1..1024"),
    (["--budget", "-1"], "a number of variants 0.."),
])
def test_the_script_refuses_bad_arguments(args, expect):
    run = subprocess.run([sys.executable, SCRIPT, "--world", "synthetic", "--plans", "none.jsonl", "--seed", "1", "--out", "none"] + args,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and expect in run.stderr, run.stderr


def test_the_script_has_help():
    run = subprocess.run([sys.executable, SCRIPT, "--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "--shift" in run.stdout and "--budget" in run.stdout and "--replace" in run.stdout, run.stderr
