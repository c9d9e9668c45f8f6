"""CPU: the host side of refining many plans in one call (include/eirgrid_hip.h eg_refine_plans) — the new constants and signatures, what
eg_refine_plans_validate accepts and refuses (every message about a plan names it), the argument check in front of any device, and that
scripts/refine_front.py explains itself without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import Plan, PlanSet, _refine_opts
from tests.test_plan_edits import _base
from tests.test_plans import _empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_native_agree_on_the_new_symbols(built):
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    L = N.lib()
    for name in ("eg_refine_plans_validate", "eg_refine_plans", "eg_debug_refine_pick_many"):
        assert name in N.EXPORTS and hasattr(L, name), name
        assert len(re.findall(rf"^int32_t {name}\(", header, flags=re.M)) == 1, name
    assert re.search(r"#define EG_REFINE_MAX_PLANS 256\b", header) and re.search(r"#define EG_PARETO_MAX 256\b", header)
    assert N.REFINE_MAX_PLANS == 256
    # the signatures: eg_refine_plan's, with arrays where it has scalars
    assert L.eg_refine_plans.argtypes == L.eg_refine_plan.argtypes and L.eg_refine_plans.restype == C.c_int32
    assert L.eg_refine_plans_validate.argtypes == L.eg_refine_validate.argtypes
    assert len(L.eg_debug_refine_pick_many.argtypes) == 7
    assert re.search(r"int32_t eg_refine_plans\(eg_ctx \*, const eg_policy_snapshot \*, const eg_opts \*, const eg_plan_set \*bases /\* 1\.\.EG_REFINE_MAX_PLANS \*/,", header)
    assert re.search(r"int32_t eg_debug_refine_pick_many\(eg_ctx \*, int32_t mode, const uint32_t \*seg_first, const uint32_t \*seg_count, int32_t n_segs,", header)
    assert "EIRGRID_REFINE_LAUNCH_VARIANTS" in header


def _validate(plans, **kw):
    L = N.lib()
    args = dict(mode=1, max_rounds=4, replace_with=None, append_with=None); args.update(kw)
    ro, keep = _refine_opts(**args)
    ps = PlanSet(plans) if plans is not None else None
    rc = L.eg_refine_plans_validate(C.byref(ps.s) if ps is not None else None, C.byref(ro))
    return rc, L.eg_last_error().decode()


def test_validate_accepts_one_plan_and_a_whole_front(built):
    assert _validate([_base()])[0] == N.EG_OK
    rc, msg = _validate([_base() for _ in range(256)], mode=2, replace_with=[0, 60], append_with=[12])
    assert rc == N.EG_OK, msg
    assert _validate([Plan(_empty(), _empty()), _base()], append_with=[3])[0] == N.EG_OK


def test_validate_refuses_bad_sets(built):
    rc, msg = _validate([])
    assert rc == N.EG_ERR_BAD_ARG and "n_plans = 0 (at least 1)" in msg, msg
    rc, msg = _validate([_base() for _ in range(257)])
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_refine_plans_validate: ") and "257 plans (at most 256)" in msg, msg
    rc, msg = _validate(None)
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    L = N.lib()
    ps = PlanSet([_base()])
    assert L.eg_refine_plans_validate(C.byref(ps.s), None) == N.EG_ERR_BAD_ARG and "NULL options" in L.eg_last_error().decode()


@pytest.mark.parametrize("kw, expect", [
    (dict(mode=0), "mode 0 (1: optimization_mode None, 2: cost_only)"),
    (dict(mode=3), "mode 3 ("),
    (dict(max_rounds=0), "max_rounds = 0 (at least 1)"),
    (dict(max_rounds=-2), "max_rounds = -2 (at least 1)"),
    (dict(replace_with=[3, 61]), "replace_with[1]: action 61 >= 61"),
    (dict(append_with=[200]), "append_with[0]: action 200 >= 61"),
])
def test_validate_names_the_option(built, kw, expect):
    rc, msg = _validate([_base(), _base()], **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_refine_plans_validate: ") and expect in msg, msg


def test_validate_names_the_plan(built):
    bad = _base(); bad.best_actions[0][1] = 61
    rc, msg = _validate([_base(), _base(), bad])
    assert rc == N.EG_ERR_BAD_ARG and "plan 2" in msg and "best_actions year 2025 entry 1: 61 >= 61" in msg, msg
    # tests/test_refine.py's `big` plan: 1 + 4 000 + 26 + 4 * 4 000 = 20 027 variants in round 0 with four replace actions
    big = Plan([[60] * 160 for _ in range(25)] + [[]], [[24] for _ in range(26)])
    rc, msg = _validate([_base(), big], replace_with=[0, 3, 6, 9])
    assert rc == N.EG_ERR_BAD_ARG and "plan 1: round 0 enumerates 20027 variants (at most 16384)" in msg, msg
    assert _validate([_base(), big], replace_with=[0, 3, 6])[0] == N.EG_OK
    rc, msg = _validate([big, _base()], replace_with=[0, 3, 6, 9])
    assert rc == N.EG_ERR_BAD_ARG and "plan 0: round 0 enumerates 20027" in msg, msg


def test_refine_plans_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_refine_plans(None, None, None, None, None, 0, 0, None, None, None, None, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_refine_plans: bad argument" in L.eg_last_error().decode()
    assert L.eg_debug_refine_pick_many(None, 1, None, None, 0, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_debug_refine_pick_many: bad argument" in L.eg_last_error().decode()


def test_the_front_script_explains_itself_without_a_gpu(built):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "refine_front.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for flag in ("--world", "--plans", "--policy", "--seed", "--rounds", "--replace", "--append", "--cost-only", "--out"):
        assert flag in out.stdout, flag
