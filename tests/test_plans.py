"""CPU: the host side of plan evaluation (include/eirgrid_hip.h eg_evaluate_plans) — eg_plans_load on checkpoints and JSON Lines,
the refusals of eg_plans_validate / eg_plans_load, the CLI flags and the exported symbols."""
import ctypes as C
import json
import os
import subprocess

import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, Plan, PlanSet
from tests.test_checkpoint import _trained_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def _action(a):
    """SerializableAction of canonical index a (the checkpoint writer's form, csrc/eg_checkpoint.cpp Writer::action)."""
    types = ["OnshoreWind", "OffshoreWind", "DomesticSolar", "CommercialSolar", "UtilitySolar", "Nuclear", "CoalPlant",
             "GasCombinedCycle", "GasPeaker", "Biomass", "HydroDam", "PumpedStorage", "BatteryStorage", "TidalGenerator", "WaveEnergy"]
    d = dict(action_type="DoNothing", generator_type=None, generator_id=None, operation_percentage=None, offset_type=None, cost_multiplier=None)
    if a < 45:
        d.update(action_type="AddGenerator", generator_type=types[a // 3], cost_multiplier=[100, 120, 150][a % 3])
    elif a < 57:
        d.update(action_type="AddCarbonOffset", offset_type=["Forest", "Wetland", "ActiveCapture", "CarbonCredit"][(a - 45) // 3],
                 cost_multiplier=[100, 120, 150][(a - 45) % 3])
    elif a < 60:
        d.update(action_type=["UpgradeEfficiency", "AdjustOperation", "CloseGenerator"][a - 57], generator_id="")
        if a == 58:
            d["operation_percentage"] = 0
    return d


def _line(run, dfc, name=None):
    d = {"best_actions": {str(2025 + y): [_action(a) for a in l] for y, l in enumerate(run)},
         "best_deficit_actions": {str(2025 + y): [_action(a) for a in l] for y, l in enumerate(dfc)}}
    if name is not None:
        d["name"] = name
    return json.dumps(d)


def _empty():
    return [[] for _ in range(26)]


def _load_error(path):
    L = N.lib()
    ps = L.eg_plans_load(str(path).encode())
    assert not ps
    return L.eg_last_error().decode()


def test_load_round_trips_a_checkpoint(tmp_path, world):
    pol = _trained_policy(world)
    assert pol.get("has_best_actions") == 1 and sum(len(l) for l in pol.lists(0)) > 0
    path = tmp_path / "best_weights.json"
    pol.save_to_file(path)
    plans = Plan.load(path)
    assert len(plans) == 1
    assert plans[0].best_actions == pol.lists(0) and plans[0].best_deficit_actions == pol.lists(1)
    assert plans[0] == Plan.from_policy(pol)
    fresh = tmp_path / "fresh.json"
    ActionWeights().save_to_file(fresh)      # best_actions: null -> an empty plan
    assert Plan.load(fresh)[0] == Plan(_empty(), _empty())


def test_jsonl_loads_with_names(tmp_path, built):
    plans = [(_empty(), _empty(), "nothing"), ([[0, 3, 60]] + _empty()[1:], [[24]] + _empty()[1:], "offshore 2025"),
             (_empty()[:5] + [[45] * 7] + _empty()[6:], _empty(), None)]
    path = tmp_path / "plans.jsonl"
    path.write_text("\n".join(_line(*p) for p in plans[:2]) + "\n\n" + _line(*plans[2]) + "\n")
    got = Plan.load(path)
    assert [p.name for p in got] == ["nothing", "offshore 2025", ""]
    every = tmp_path / "every.jsonl"      # every canonical action survives the schema
    every.write_text(_line([list(range(61))] + _empty()[1:], _empty()[:25] + [[60, 24]]) + "\n")
    assert Plan.load(every)[0].best_actions[0] == list(range(61))
    for p, (run, dfc, _) in zip(got, plans):
        assert p.best_actions == run and p.best_deficit_actions == dfc


def test_malformed_files_name_the_line_and_field(tmp_path, built):
    good = _line(_empty(), _empty(), "ok")
    d = json.loads(good)
    unknown = json.loads(good); unknown["best_actions"]["2030"] = [{"action_type": "AddGenerator", "generator_type": "Fusion", "cost_multiplier": 100}]
    too_long = json.loads(good); too_long["best_deficit_actions"]["2025"] = [_action(24)] * 4097
    no_key = {k: v for k, v in d.items() if k != "best_actions"}
    bad_year = json.loads(good); bad_year["best_actions"]["1999"] = []
    lines = [good, json.dumps(unknown), "{not json", json.dumps(too_long), json.dumps(no_key), json.dumps(bad_year), good]
    path = tmp_path / "bad.jsonl"
    path.write_text("\n".join(lines) + "\n")
    msg = _load_error(path)
    assert "line 1" not in msg and "line 7" not in msg, msg
    assert 'line 2: best_actions["2030"] entry 0: unknown action' in msg, msg
    assert "line 3:" in msg, msg
    assert "line 4: best_deficit_actions: 4097 entries (at most 4096)" in msg, msg
    assert 'line 5: missing "best_actions"' in msg, msg
    assert 'line 6: best_actions: year "1999"' in msg, msg
    empty = tmp_path / "empty.jsonl"
    empty.write_text("\n\n")
    assert "no plans" in _load_error(empty)
    assert "cannot open" in _load_error(tmp_path / "missing.jsonl")


def _set(plans):
    return PlanSet(plans)


@pytest.mark.parametrize("case, expect", [
    ("entry", "plan 1 (\"b\"): best_actions year 2026 entry 1: 61 >= 61"),
    ("deficit_entry", "plan 0 (\"a\"): best_deficit_actions year 2025 entry 0: 200 >= 61"),
    ("too_long", "plan 1 (\"b\"): best_actions: 4097 entries (at most 4096)"),
    ("counts_more", "plan 1 (\"b\"): the best_actions counts add up to more than best_actions_len"),
    ("counts_fewer", "the best_deficit_actions counts add up to 1 entries, best_deficit_actions_len = 2"),
    ("negative", "plan 0 (\"a\"): best_actions year 2027: count -1 < 0"),
    ("zero", "n_plans = 0"),
    ("null_counts", "NULL best_count"),
    ("null_actions", "NULL best_actions"),
    ("null_set", "NULL plan set"),
])
def test_validate_refuses_malformed_sets(built, case, expect):
    a = Plan([[5]] + _empty()[1:], [[24]] + _empty()[1:], "a")
    b = Plan(_empty()[:1] + [[0, 60]] + _empty()[2:], _empty(), "b")
    if case == "entry":
        b.best_actions[1][1] = 61
    if case == "deficit_entry":
        a.best_deficit_actions[0][0] = 200
    if case == "too_long":
        b.best_actions[3] = [12] * 4095      # + the two of 2026
    ps = _set([a, b])
    s = ps.s
    if case == "counts_more":
        s.best_actions_len = 2
    if case == "counts_fewer":
        s.best_deficit_actions_len = 2
    if case == "negative":
        ps.count[0, 2] = -1
    if case == "zero":
        s.n_plans = 0
    if case == "null_counts":
        s.best_count = None
    if case == "null_actions":
        s.best_actions = None
    L = N.lib()
    rc = L.eg_plans_validate(None if case == "null_set" else C.byref(s))
    assert rc == N.EG_ERR_BAD_ARG
    msg = L.eg_last_error().decode()
    assert expect in msg, msg
    ok = _set([Plan([[5]] + _empty()[1:], [[24]] + _empty()[1:], "a"), Plan(_empty(), _empty())])
    assert L.eg_plans_validate(C.byref(ok.s)) == N.EG_OK


def test_help_lists_the_evaluate_flags(built):
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert "--evaluate <FILE>" in out.stdout and "--evaluate-policy <CKPT>" in out.stdout


def test_cli_refuses_invalid_plans_before_any_device(built, tmp_path):
    path = tmp_path / "plans.jsonl"
    path.write_text(_line(_empty(), _empty(), "ok") + "\n" + '{"best_actions": {}}' + "\n")
    out = subprocess.run([CLI, "--world", WORLD, "-c", str(tmp_path / "ck"), "--evaluate", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1, out.stdout + out.stderr
    assert 'line 2: missing "best_deficit_actions"' in out.stderr
    assert "World:" not in out.stdout and not (tmp_path / "ck").exists()
    out = subprocess.run([CLI, "--world", WORLD, "--evaluate-policy", str(path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--evaluate-policy needs --evaluate" in out.stderr


def test_library_exports_the_plan_symbols(built):
    L = N.lib()
    for name in ("eg_evaluate_plans", "eg_plans_validate", "eg_plans_load", "eg_plans_free"):
        assert hasattr(L, name) and name in N.EXPORTS, name
