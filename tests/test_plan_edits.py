"""CPU: the host side of plan edits (include/eirgrid_hip.h eg_evaluate_plan_edits) — what eg_plan_edits_validate accepts and refuses, the
canonical edit order of a sensitivity run, the CLI flags and the exported symbols."""
import ctypes as C
import os
import subprocess

import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import Plan, PlanEdit, PlanSet, _edit_array, sensitivity_edits
from tests.test_plans import _empty, _line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def _base():
    run = _empty(); dfc = _empty()
    run[0] = [5, 12, 60]; run[6] = [3]; run[25] = [45, 0]
    dfc[0] = [24]; dfc[6] = [24, 60]
    return Plan(run, dfc, "base")


def _validate(base_set, edits, n=None):
    L = N.lib()
    arr, k = _edit_array(edits)
    rc = L.eg_plan_edits_validate(C.byref(base_set.s) if base_set is not None else None, arr, k if n is None else n)
    return rc, L.eg_last_error().decode()


def test_struct_layout_is_the_headers(built):
    assert C.sizeof(N.EgPlanEdit) == 12 and N.EgPlanEdit.pos.offset == 4 and N.EgPlanEdit.action.offset == 8


def test_validate_accepts_every_well_formed_edit(built):
    base = _base()
    ps = PlanSet([base])
    edits = [PlanEdit()]
    for which, lists in enumerate((base.best_actions, base.best_deficit_actions)):
        for y, l in enumerate(lists):
            edits += [PlanEdit("delete", which, y, i) for i in range(len(l))]
            edits += [PlanEdit("replace", which, y, i, a) for i in range(len(l)) for a in (0, 24, 60)]
            edits += [PlanEdit("insert", which, y, i, a) for i in range(len(l) + 1) for a in (0, 60)]      # (pos == len: append; empty years too)
    edits.append(PlanEdit("none", 7, 99, 12345, 200))      # (none: the other fields are not read)
    rc, msg = _validate(ps, edits)
    assert rc == N.EG_OK, msg
    full = Plan([[60] * 157 for _ in range(26)], _empty())      # 4 082 entries: 14 inserts would still fit, each on its own
    rc, msg = _validate(PlanSet([full]), [PlanEdit("insert", 0, 25, 157, 3)])
    assert rc == N.EG_OK, msg


@pytest.mark.parametrize("edit, expect", [
    (PlanEdit("delete", 0, 0, 3), "edit 2: pos 3 outside best_actions year 2025 (3 entries)"),
    (PlanEdit("replace", 1, 6, 2, 24), "edit 2: pos 2 outside best_deficit_actions year 2031 (2 entries)"),
    (PlanEdit("insert", 0, 6, 2, 24), "edit 2: pos 2 outside best_actions year 2031 (1 entries)"),
    (PlanEdit("delete", 0, 3, 0), "edit 2: pos 0 outside best_actions year 2028 (0 entries)"),
    (PlanEdit("replace", 0, 0, 0, 61), "edit 2: action 61 >= 61"),
    (PlanEdit("insert", 1, 0, 0, 200), "edit 2: action 200 >= 61"),
    (PlanEdit("delete", 0, 26, 0), "edit 2: year 26"),
    (PlanEdit("delete", 2, 0, 0), "edit 2: list 2"),
])
def test_validate_names_the_edit_and_the_field(built, edit, expect):
    rc, msg = _validate(PlanSet([_base()]), [PlanEdit(), PlanEdit("delete", 0, 0, 0), edit])
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_plan_edits_validate: ") and expect in msg, msg


def test_validate_refuses_unknown_kinds_overlong_lists_and_bad_bases(built):
    ps = PlanSet([_base()])
    arr, _ = _edit_array([PlanEdit(), PlanEdit()])
    arr[1].kind = 4
    L = N.lib()
    assert L.eg_plan_edits_validate(C.byref(ps.s), arr, 2) == N.EG_ERR_BAD_ARG
    assert "edit 1: kind 4" in L.eg_last_error().decode()
    cap = [[60] * 157 for _ in range(26)]
    cap[0] += [60] * (4096 - 26 * 157)
    rc, msg = _validate(PlanSet([Plan(cap, [[24] * 4096] + _empty()[1:])]), [PlanEdit("replace", 0, 0, 0, 1), PlanEdit("delete", 1, 0, 4095), PlanEdit("insert", 0, 25, 157, 3)])
    assert rc == N.EG_ERR_BAD_ARG and "edit 2: the insert makes best_actions 4097 entries (at most 4096)" in msg, msg
    rc, msg = _validate(PlanSet([Plan(cap, [[24] * 4096] + _empty()[1:])]), [PlanEdit("insert", 1, 3, 0, 24)])
    assert rc == N.EG_ERR_BAD_ARG and "edit 0: the insert makes best_deficit_actions 4097 entries" in msg, msg
    rc, msg = _validate(ps, [], 0)
    assert rc == N.EG_ERR_BAD_ARG and "n_edits = 0 (at least 1)" in msg, msg
    rc, msg = _validate(ps, [PlanEdit()], -3)
    assert rc == N.EG_ERR_BAD_ARG and "n_edits = -3" in msg, msg
    rc, msg = _validate(PlanSet([_base(), _base()]), [PlanEdit()])
    assert rc == N.EG_ERR_BAD_ARG and "the base holds 2 plans (exactly 1)" in msg, msg
    rc, msg = _validate(None, [PlanEdit()])
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    bad = _base(); bad.best_actions[0][1] = 61
    rc, msg = _validate(PlanSet([bad]), [PlanEdit()])
    assert rc == N.EG_ERR_BAD_ARG and "best_actions year 2025 entry 1: 61 >= 61" in msg, msg
    assert L.eg_plan_edits_validate(C.byref(ps.s), None, 1) == N.EG_ERR_BAD_ARG and "NULL edits" in L.eg_last_error().decode()


def test_edits_apply_in_python_as_documented():
    base = _base()
    assert PlanEdit().apply(base) == base
    assert PlanEdit("delete", 0, 0, 1).apply(base).best_actions[0] == [5, 60]
    assert PlanEdit("replace", 1, 6, 1, 3).apply(base).best_deficit_actions[6] == [24, 3]
    assert PlanEdit("insert", 0, 25, 2, 9).apply(base).best_actions[25] == [45, 0, 9]
    assert PlanEdit("insert", 0, 25, 0, 9).apply(base).best_actions[25] == [9, 45, 0]
    assert base == _base()      # (a copy: the base is left alone)


def test_sensitivity_order_is_canonical():
    base = _base()
    e = sensitivity_edits(base, replace_with=[12, 60])
    assert e[0] == PlanEdit()
    assert e[1:7] == [PlanEdit("delete", 0, 0, 0), PlanEdit("delete", 0, 0, 1), PlanEdit("delete", 0, 0, 2), PlanEdit("delete", 0, 6, 0),
                      PlanEdit("delete", 0, 25, 0), PlanEdit("delete", 0, 25, 1)]
    assert e[7:10] == [PlanEdit("delete", 1, 0, 0), PlanEdit("delete", 1, 6, 0), PlanEdit("delete", 1, 6, 1)]
    assert e[10:14] == [PlanEdit("replace", 0, 0, 0, 12), PlanEdit("replace", 0, 0, 0, 60), PlanEdit("replace", 0, 0, 1, 12), PlanEdit("replace", 0, 0, 1, 60)]
    assert len(e) == 1 + 6 + 3 + 2 * 6
    assert len(sensitivity_edits(base)) == 10


def test_help_lists_the_sensitivity_flags(built):
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert "--sensitivity <FILE>" in out.stdout and "--sensitivity-replace <a,b,...>" in out.stdout and "--evaluate-policy <CKPT>" in out.stdout


def test_cli_refusals_need_no_device(built, tmp_path):
    path = tmp_path / "plans.jsonl"
    path.write_text(_line([[5, 12]] + _empty()[1:], _empty(), "ok") + "\n")
    base = [CLI, "--world", WORLD, "-c", str(tmp_path / "ck")]
    out = subprocess.run(base + ["--sensitivity", str(path), "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--sensitivity runs on one device" in out.stderr, out.stdout + out.stderr
    out = subprocess.run(base + ["--sensitivity-replace", "3,4"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--sensitivity-replace needs --sensitivity" in out.stderr
    out = subprocess.run(base + ["--sensitivity", str(path), "--sensitivity-replace", "3,61"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "canonical actions 0..60" in out.stderr
    out = subprocess.run(base + ["--sensitivity", str(path), "--evaluate", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "separate runs" in out.stderr
    broken = tmp_path / "broken.jsonl"
    broken.write_text('{"best_actions": {}}' + "\n")
    out = subprocess.run(base + ["--sensitivity", str(broken)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and 'line 1: missing "best_deficit_actions"' in out.stderr, out.stdout + out.stderr
    assert "World:" not in out.stdout and not (tmp_path / "ck").exists()


def test_cli_without_a_device_fails_as_evaluate_does(built, tmp_path):
    have_device = N.lib().eg_device_count() > 0      # (with a device both runs succeed: the outcome is --evaluate's either way)
    path = tmp_path / "plans.jsonl"
    path.write_text(_line([[5, 12]] + _empty()[1:], _empty(), "ok") + "\n")
    outs = []
    for flag in ("--evaluate", "--sensitivity"):
        ck = tmp_path / flag.strip("-")
        out = subprocess.run([CLI, "--world", WORLD, "-c", str(ck), flag, str(path)], capture_output=True, text=True, timeout=300)
        outs.append((out.returncode, out.stderr.strip()))
        if have_device:
            assert out.returncode == 0 and ck.exists(), out.stdout + out.stderr
        else:
            assert out.returncode == 1 and out.stderr.startswith("eg_create: "), out.stdout + out.stderr
            assert not ck.exists()
    assert outs[0] == outs[1]


def test_library_exports_the_plan_edit_symbols(built):
    L = N.lib()
    for name in ("eg_plan_edits_validate", "eg_evaluate_plan_edits", "eg_debug_fetch_plan_block"):
        assert hasattr(L, name) and name in N.EXPORTS, name


def test_fetch_plan_block_refuses_without_a_plan_batch(built):
    L = N.lib()
    assert L.eg_debug_fetch_plan_block(None, 0, None) == N.EG_ERR_BAD_ARG and "bad argument" in L.eg_last_error().decode()
    assert "eg_debug_fetch_plan_block" in N.EXPORTS and N.PLAN_BLOCK_BYTES == 8832
