"""CPU: the option checks the plan-search validators share (csrc/eg_plan_host.cpp: check_mode, check_objectives, check_cap,
check_launch_variants, validate_front_opts, validate_action_lists) seen through each of the five validators that run them —
eg_breed_validate, eg_explore_validate, eg_refine_validate, eg_refine_plans_validate, eg_refine_plans_moves_validate.  Every refusal is
pinned with its FULL text, prefix included: the texts are the ones the library gave before the checks were shared, written out here, so
a validator that picks up another one's wording or prefix fails.  One one-entry plan serves every case."""
import ctypes as C

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import Plan, PlanSet

_U8P = C.POINTER(C.c_uint8)
ONE = Plan([[17]] + [[] for _ in range(25)], [[] for _ in range(26)], "one entry")
VALIDATORS = ("eg_breed_validate", "eg_explore_validate", "eg_refine_validate", "eg_refine_plans_validate", "eg_refine_plans_moves_validate")


def _list(values):
    """(count, pointer, what keeps the pointer alive) of an action list; None: no list, count 0; an int: that count with a NULL list"""
    if values is None:
        return 0, None, None
    if isinstance(values, int):
        return values, None, None
    arr = np.array(values, np.uint8)
    return len(values), arr.ctypes.data_as(_U8P), arr


def _validate(validator, n_plans=1, mode=1, objectives=15, cap=256, max_generations=8, launch_variants=0, replace_with=None, append_with=None):
    """rc and message of `validator` over n_plans copies of ONE; the options a validator does not have are not passed to it"""
    L = N.lib()
    ps = PlanSet([ONE] * n_plans)
    n_rep, rep, keep_rep = _list(replace_with)
    n_app, app, keep_app = _list(append_with)
    if validator == "eg_breed_validate":
        opts = N.EgBreedOpts(mode, objectives, cap, max_generations, 0, None, launch_variants)
        rc = L.eg_breed_validate(C.byref(ps.s), C.byref(opts))
    elif validator == "eg_explore_validate":
        opts = N.EgExploreOpts(mode, objectives, cap, max_generations, n_rep, rep, n_app, app, 0, launch_variants, 0)
        rc = L.eg_explore_validate(C.byref(ps.s), C.byref(opts))
    else:
        opts = N.EgRefineOpts(mode, 4, n_rep, rep, n_app, app)
        if validator == "eg_refine_plans_moves_validate":
            mo = N.EgRefineMoveOpts(1)
            rc = L.eg_refine_plans_moves_validate(C.byref(ps.s), C.byref(opts), C.byref(mo))
        else:
            rc = getattr(L, validator)(C.byref(ps.s), C.byref(opts))
    return rc, L.eg_last_error().decode()


def test_every_validator_accepts_the_defaults(built):
    for v in VALIDATORS:
        rc, msg = _validate(v)
        assert rc == N.EG_OK, (v, msg)
        rc, msg = _validate(v, replace_with=[0, 60], append_with=[60])
        assert rc == N.EG_OK, (v, msg)


FRONT = [      # the archive options: eg_breed_validate and eg_explore_validate have them, with one wording
    ({"mode": 0}, "mode 0 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ({"mode": 3}, "mode 3 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ({"objectives": 0}, "objectives 0 is outside 1..15 (bit i = metric i)"),
    ({"objectives": 16}, "objectives 16 is outside 1..15 (bit i = metric i)"),
    ({"cap": 0}, "cap 0 is outside 1..EG_PARETO_MAX (256)"),
    ({"cap": 257}, "cap 257 is outside 1..EG_PARETO_MAX (256)"),
    ({"max_generations": 0}, "max_generations = 0 (at least 1)"),
    ({"max_generations": -7}, "max_generations = -7 (at least 1)"),
    ({"launch_variants": -1}, "launch_variants = -1 (1..16384; 0: 16384)"),
    ({"launch_variants": 16385}, "launch_variants = 16385 (1..16384; 0: 16384)"),
    ({"n_plans": 257}, "the set holds 257 plans (at most 256)"),
    # (the order of the checks: the set before the options, mode before objectives before cap before max_generations before launch_variants)
    ({"n_plans": 257, "mode": 0}, "the set holds 257 plans (at most 256)"),
    ({"mode": 0, "objectives": 0, "cap": 0}, "mode 0 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ({"objectives": 0, "cap": 0, "max_generations": 0}, "objectives 0 is outside 1..15 (bit i = metric i)"),
    ({"cap": 0, "max_generations": 0, "launch_variants": -1}, "cap 0 is outside 1..EG_PARETO_MAX (256)"),
    ({"max_generations": 0, "launch_variants": -1}, "max_generations = 0 (at least 1)"),
]


@pytest.mark.parametrize("validator", ["eg_breed_validate", "eg_explore_validate"])
@pytest.mark.parametrize("kw,expect", FRONT)
def test_archive_options(built, validator, kw, expect):
    rc, msg = _validate(validator, **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg == validator + ": " + expect, msg


LISTS = [      # replace_with / append_with: eg_explore_validate and the three refinement validators have them, with one wording
    ({"replace_with": -1}, "n_replace = -1"),
    ({"append_with": -3}, "n_append = -3"),
    ({"replace_with": 2}, "NULL replace_with with n_replace = 2"),
    ({"append_with": 1}, "NULL append_with with n_append = 1"),
    ({"replace_with": [5, 61]}, "replace_with[1]: action 61 >= 61"),
    ({"append_with": [255]}, "append_with[0]: action 255 >= 61"),
    ({"replace_with": [61], "append_with": [61]}, "replace_with[0]: action 61 >= 61"),      # (replace_with is checked first)
    ({"replace_with": [3], "append_with": 4}, "NULL append_with with n_append = 4"),
]


@pytest.mark.parametrize("validator", ["eg_explore_validate", "eg_refine_validate", "eg_refine_plans_validate", "eg_refine_plans_moves_validate"])
@pytest.mark.parametrize("kw,expect", LISTS)
def test_action_lists(built, validator, kw, expect):
    rc, msg = _validate(validator, **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg == validator + ": " + expect, msg


@pytest.mark.parametrize("validator,kw,expect", [
    # the refinement validators word a bad mode their own way, and check it before the lists
    ("eg_refine_validate", {"mode": 0}, "eg_refine_validate: mode 0 (1: optimization_mode None, 2: cost_only)"),
    ("eg_refine_plans_validate", {"mode": 3}, "eg_refine_plans_validate: mode 3 (1: optimization_mode None, 2: cost_only)"),
    ("eg_refine_plans_moves_validate", {"mode": -1}, "eg_refine_plans_moves_validate: mode -1 (1: optimization_mode None, 2: cost_only)"),
    ("eg_refine_plans_validate", {"mode": 0, "replace_with": [61]}, "eg_refine_plans_validate: mode 0 (1: optimization_mode None, 2: cost_only)"),
    # ... and an oversized set each in its own words, before the options
    ("eg_refine_validate", {"n_plans": 2}, "eg_refine_validate: the base holds 2 plans (exactly 1)"),
    ("eg_refine_validate", {"n_plans": 257, "mode": 0}, "eg_refine_validate: the base holds 257 plans (exactly 1)"),
    ("eg_refine_plans_validate", {"n_plans": 257}, "eg_refine_plans_validate: the set holds 257 plans (at most 256)"),
    ("eg_refine_plans_validate", {"n_plans": 257, "mode": 0}, "eg_refine_plans_validate: the set holds 257 plans (at most 256)"),
    ("eg_refine_plans_moves_validate", {"n_plans": 257}, "eg_refine_plans_moves_validate: the set holds 257 plans (at most 256)"),
    ("eg_refine_plans_moves_validate", {"n_plans": 257, "append_with": 1}, "eg_refine_plans_moves_validate: the set holds 257 plans (at most 256)"),
    # eg_explore_validate: the lists between max_generations and launch_variants
    ("eg_explore_validate", {"max_generations": 0, "replace_with": [61]}, "eg_explore_validate: max_generations = 0 (at least 1)"),
    ("eg_explore_validate", {"replace_with": [61], "launch_variants": -1}, "eg_explore_validate: replace_with[0]: action 61 >= 61"),
])
def test_each_validator_keeps_its_own_words_and_order(built, validator, kw, expect):
    rc, msg = _validate(validator, **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg == expect, msg
