"""CPU: the host side of greedy plan refinement (include/eirgrid_hip.h eg_refine_plan) — struct layouts, what eg_refine_validate accepts
and refuses, the order of a round's variants, the CLI flags, eg_plans_save, and the definition itself restated in Python over the tabled
oracle (`refine_restated`, which the GPU tests import): the small inputs on which the tie rule and both stop reasons are reached."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ActionWeights, HostTables, Plan, PlanEdit, PlanSet, _refine_opts, rank_score, refine_edits, sensitivity_edits
from oracle import api as O
from tests.helpers import oracle_weights_like
from tests.test_gpu_replay_hoist import _full_script
from tests.test_plan_edits import _base
from tests.test_plans import _empty, _line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")
SEED = 1234


# ---------------------------------------------------------------- the definition, restated
def apply_edit(plan, e):
    """Edit e applied to a copy of `plan` (the test's own restatement, not PlanEdit.apply)."""
    run = [list(l) for l in plan.best_actions]; dfc = [list(l) for l in plan.best_deficit_actions]
    l = (run, dfc)[e.list][e.year]
    if e.kind == "delete":
        l.pop(e.pos)
    elif e.kind == "replace":
        l[e.pos] = e.action
    elif e.kind == "insert":
        l[e.pos:e.pos] = [e.action]
    else:
        assert e.kind == "none"
    return Plan(run, dfc, plan.name)


def round_edits(plan, replace_with=(), append_with=()):
    """The variants of one round, written out once more: none, deletes of list 0 in (year, pos) order, deletes of list 1, replaces,
    then per year and append action an insert behind the year's last entry — unless list 0 is full."""
    edits = [PlanEdit()]
    for which, lists in enumerate((plan.best_actions, plan.best_deficit_actions)):
        for y in range(26):
            edits += [PlanEdit("delete", which, y, i) for i in range(len(lists[y]))]
    for y in range(26):
        for i in range(len(plan.best_actions[y])):
            edits += [PlanEdit("replace", 0, y, i, int(a)) for a in replace_with]
    if sum(len(l) for l in plan.best_actions) < 4096:
        for y in range(26):
            edits += [PlanEdit("insert", 0, y, len(plan.best_actions[y]), int(a)) for a in append_with]
    return edits


class OracleEvaluator:
    """evaluate(plan, edits) -> (status [n], metrics [n,4]) by the tabled oracle: every variant the replay of the edited plan at global
    index `index` of `seed` under `pol`.  Results are kept by plan, so two modes over the same trajectory evaluate it once."""

    def __init__(self, world, pol, seed=SEED, index=0):
        self.tb = O.OracleTables(HostTables(world), len(world.existing_x))
        self.pol, self.seed, self.index = pol, seed, index
        self.ow = oracle_weights_like(pol)
        self.ow.set("has_best", 1); self.ow.set("has_best_actions", 1); self.ow.set("has_best_deficit_actions", 1)
        self.seen = {}
        self.last = None      # (plan key, EpisodeOut) of the last episode run: the caller's replay of the refined plan

    def one(self, plan):
        key = (repr(plan.best_actions), repr(plan.best_deficit_actions))
        if key not in self.seen:
            for y in range(26):
                self.ow.set_list(0, y, plan.best_actions[y]); self.ow.set_list(1, y, plan.best_deficit_actions[y])
            st, ref = O.run_episode_tabled(self.tb, self.ow, self.seed + self.index, replay=True)
            self.seen[key] = (st, np.array(ref.metrics, np.float64))
            self.last = (key, ref)
        return self.seen[key]

    def record(self, plan):
        """the oracle's whole record of `plan`'s replay"""
        key = (repr(plan.best_actions), repr(plan.best_deficit_actions))
        if self.last is None or self.last[0] != key:
            self.seen.pop(key, None)
            self.one(plan)
        return self.last[1]

    def __call__(self, plan, edits):
        rows = [self.one(apply_edit(plan, e)) for e in edits]
        return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows]).reshape(len(rows), 4)


def refine_restated(evaluate, base, mode=1, max_rounds=64, replace_with=(), append_with=()):
    """include/eirgrid_hip.h eg_refine_plan, literally.  `evaluate(plan, edits)` gives the variants' status and metrics.  Returns
    (refined plan, steps, stop reason, start score, per round the number of variants tied at the round's maximum); a step is
    (edit, variant, n_variants, n_failed, score, metrics)."""
    plan, steps, ties, start = base, [], [], float("nan")
    while True:
        edits = round_edits(plan, replace_with, append_with)
        assert len(edits) <= N.REFINE_MAX_VARIANTS
        status, metrics = evaluate(plan, edits)
        score = np.array([rank_score(metrics[j], mode == 2) if status[j] == N.EG_EP_OK else np.nan for j in range(len(edits))])
        cand = (status == N.EG_EP_OK) & ~np.isnan(score)
        if not steps and cand[0]:
            start = float(score[0])
        if not cand[0]:
            return plan, steps, "base_failed", start, ties
        top = np.nanmax(np.where(cand, score, np.nan))
        winner = int(np.flatnonzero(cand & (score == top))[0])      # ties to the lowest variant
        ties.append(int((cand & (score == top)).sum()))
        if winner == 0:
            return plan, steps, "local_optimum", start, ties
        steps.append((edits[winner], winner, len(edits), int((~cand).sum()), float(score[winner]), metrics[winner].copy()))
        plan = apply_edit(plan, edits[winner])
        if len(steps) == max_rounds:
            return plan, steps, "max_rounds", start, ties


def short_policy():
    return _full_script(np.random.default_rng(7), 1, [0, 4, 12, 7], offsets_per_year=1)


def long_policy():
    return _full_script(np.random.default_rng(5), 9, [0, 4, 12, 7, 5, 1, 13, 2], offsets_per_year=1)


# what the tabled oracle gives for the four cases (the runs below check it; the GPU tests compare the device with the same runs)
CASES = {
    "short, mode 1": dict(policy=short_policy, mode=1, max_rounds=8, replace_with=(12,)),
    "short, mode 2": dict(policy=short_policy, mode=2, max_rounds=8, replace_with=(12,)),
    "long, mode 1": dict(policy=long_policy, mode=1, max_rounds=4, replace_with=()),
    "long, mode 2": dict(policy=long_policy, mode=2, max_rounds=4, replace_with=()),
}
_runs = {}
_evaluators = {}


def oracle_run(world, name):
    """(policy, base, evaluator, refine_restated's result) of a case, computed once per session"""
    if name not in _runs:
        case = CASES[name]
        key = case["policy"].__name__
        if key not in _evaluators:
            pol = case["policy"]()
            _evaluators[key] = (pol, OracleEvaluator(world, pol))
        pol, ev = _evaluators[key]
        base = Plan.from_policy(pol)
        _runs[name] = (pol, base, ev, refine_restated(ev, base, case["mode"], case["max_rounds"], case["replace_with"]))
    return _runs[name]


# ---------------------------------------------------------------- layouts, exports, validation
def test_struct_layouts_are_the_headers(built):
    assert C.sizeof(N.EgRefineOpts) == 40
    assert (N.EgRefineOpts.max_rounds.offset, N.EgRefineOpts.n_replace.offset, N.EgRefineOpts.replace_with.offset, N.EgRefineOpts.n_append.offset,
            N.EgRefineOpts.append_with.offset) == (4, 8, 16, 24, 32)
    assert C.sizeof(N.EgRefineStep) == 64
    assert (N.EgRefineStep.variant.offset, N.EgRefineStep.n_variants.offset, N.EgRefineStep.n_failed.offset, N.EgRefineStep.score.offset,
            N.EgRefineStep.metrics.offset) == (12, 16, 20, 24, 32)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert re.search(r"typedef struct \{ int32_t mode /\* 1 \| 2 \*/, max_rounds; int32_t n_replace; const uint8_t \*replace_with;\s+int32_t n_append; "
                     r"const uint8_t \*append_with; \} eg_refine_opts;", header)
    assert "typedef struct { eg_plan_edit edit; int32_t variant, n_variants, n_failed; double score; double metrics[4]; } eg_refine_step;" in header
    for name, value in (("EG_REFINE_LOCAL_OPTIMUM", 0), ("EG_REFINE_MAX_ROUNDS", 1), ("EG_REFINE_BASE_FAILED", 2), ("EG_REFINE_MAX_VARIANTS", 16384)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (N.REFINE_LOCAL_OPTIMUM, N.REFINE_MAX_ROUNDS, N.REFINE_BASE_FAILED, N.REFINE_MAX_VARIANTS) == (0, 1, 2, 16384)


def test_header_and_exports_agree_on_the_new_symbols(built):
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    L = N.lib()
    for name in ("eg_refine_validate", "eg_refine_plan", "eg_plans_save"):
        assert re.search(rf"\b{name}\(", header) and name in N.EXPORTS and hasattr(L, name), name
        assert len(re.findall(rf"^int32_t {name}\(", header, flags=re.M)) == 1, name


def _validate(base_set, **kw):
    L = N.lib()
    args = dict(mode=1, max_rounds=4, replace_with=None, append_with=None); args.update(kw)
    ro, keep = _refine_opts(**args)
    rc = L.eg_refine_validate(C.byref(base_set.s) if base_set is not None else None, C.byref(ro))
    return rc, L.eg_last_error().decode()


def test_validate_accepts_what_the_definition_allows(built):
    ps = PlanSet([_base()])
    for kw in (dict(), dict(mode=2, max_rounds=1), dict(replace_with=[0, 60], append_with=[12]), dict(max_rounds=10**6)):
        rc, msg = _validate(ps, **kw)
        assert rc == N.EG_OK, (kw, msg)
    assert _validate(PlanSet([Plan(_empty(), _empty())]), append_with=[3])[0] == N.EG_OK      # (an empty plan can still grow)


@pytest.mark.parametrize("kw, expect", [
    (dict(mode=0), "mode 0 (1: optimization_mode None, 2: cost_only)"),
    (dict(mode=3), "mode 3 ("),
    (dict(max_rounds=0), "max_rounds = 0 (at least 1)"),
    (dict(max_rounds=-2), "max_rounds = -2 (at least 1)"),
    (dict(replace_with=[3, 61]), "replace_with[1]: action 61 >= 61"),
    (dict(append_with=[200]), "append_with[0]: action 200 >= 61"),
])
def test_validate_names_the_field(built, kw, expect):
    rc, msg = _validate(PlanSet([_base()]), **kw)
    assert rc == N.EG_ERR_BAD_ARG and msg.startswith("eg_refine_validate: ") and expect in msg, msg


def test_validate_refuses_null_lists_bad_bases_and_oversized_rounds(built):
    L = N.lib()
    ps = PlanSet([_base()])
    for field, n_field in (("replace_with", "n_replace"), ("append_with", "n_append")):
        ro, keep = _refine_opts(1, 4, None, None)
        setattr(ro, n_field, 2)
        assert L.eg_refine_validate(C.byref(ps.s), C.byref(ro)) == N.EG_ERR_BAD_ARG
        assert f"NULL {field} with {n_field} = 2" in L.eg_last_error().decode()
        setattr(ro, n_field, -1)
        assert L.eg_refine_validate(C.byref(ps.s), C.byref(ro)) == N.EG_ERR_BAD_ARG and f"{n_field} = -1" in L.eg_last_error().decode()
    assert L.eg_refine_validate(C.byref(ps.s), None) == N.EG_ERR_BAD_ARG and "NULL options" in L.eg_last_error().decode()
    rc, msg = _validate(PlanSet([_base(), _base()]))
    assert rc == N.EG_ERR_BAD_ARG and "the base holds 2 plans (exactly 1)" in msg, msg
    rc, msg = _validate(None)
    assert rc == N.EG_ERR_BAD_ARG and "NULL plan set" in msg, msg
    bad = _base(); bad.best_actions[0][1] = 61
    rc, msg = _validate(PlanSet([bad]))
    assert rc == N.EG_ERR_BAD_ARG and "best_actions year 2025 entry 1: 61 >= 61" in msg, msg
    # 1 + 4 000 + 26 + 4 * 4 000 = 20 027 variants in round 0; with three replaces 16 027: the largest batch the plan paths are tested at is 16 384
    big = Plan([[60] * 160 for _ in range(25)] + [[]], [[24] for _ in range(26)])
    rc, msg = _validate(PlanSet([big]), replace_with=[0, 3, 6, 9])
    assert rc == N.EG_ERR_BAD_ARG and "round 0 enumerates 20027 variants (at most 16384)" in msg, msg
    assert _validate(PlanSet([big]), replace_with=[0, 3, 6])[0] == N.EG_OK


def test_refine_plan_checks_its_arguments_before_any_device(built):
    L = N.lib()
    assert L.eg_refine_plan(None, None, None, None, None, 0, 0, None, None, None, None, None, None) == N.EG_ERR_BAD_ARG
    assert "eg_refine_plan: bad argument" in L.eg_last_error().decode()


# ---------------------------------------------------------------- the order of a round
def test_round_order_is_the_sensitivity_order_then_the_appends():
    base = _base()
    assert refine_edits(base) == sensitivity_edits(base)
    e = refine_edits(base, replace_with=[12, 60], append_with=[7, 3])
    head = sensitivity_edits(base, replace_with=[12, 60])
    assert e[:len(head)] == head and len(e) == len(head) + 26 * 2
    tail = e[len(head):]
    assert tail[:4] == [PlanEdit("insert", 0, 0, 3, 7), PlanEdit("insert", 0, 0, 3, 3), PlanEdit("insert", 0, 1, 0, 7), PlanEdit("insert", 0, 1, 0, 3)]
    assert tail[12:14] == [PlanEdit("insert", 0, 6, 1, 7), PlanEdit("insert", 0, 6, 1, 3)]      # (behind the year's one entry)
    assert tail[-2:] == [PlanEdit("insert", 0, 25, 2, 7), PlanEdit("insert", 0, 25, 2, 3)]
    assert [t.year for t in tail] == [y for y in range(26) for _ in range(2)]
    assert e == round_edits(base, [12, 60], [7, 3])      # the restatement's enumeration is the library's
    full = [[60] * 157 for _ in range(26)]
    full[0] += [60] * (4096 - 26 * 157)
    assert refine_edits(Plan(full, _empty()), append_with=[7]) == sensitivity_edits(Plan(full, _empty()))      # 4 096 entries: no appends
    full[0].pop()
    assert len(refine_edits(Plan(full, _empty()), append_with=[7])) == 1 + 4095 + 26
    assert round_edits(Plan(full, _empty()), (), [7]) == refine_edits(Plan(full, _empty()), append_with=[7])


# ---------------------------------------------------------------- CLI and files
def test_help_lists_the_refine_flags(built):
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for flag in ("--refine <FILE>", "--refine-rounds <N>", "--refine-replace <a,b,...>", "--refine-append <a,b,...>"):
        assert flag in out.stdout, flag


def test_cli_refusals_need_no_device(built, tmp_path):
    one = tmp_path / "one.jsonl"
    one.write_text(_line([[5, 12]] + _empty()[1:], _empty(), "ok") + "\n")
    two = tmp_path / "two.jsonl"
    two.write_text(_line([[5, 12]] + _empty()[1:], _empty(), "a") + "\n" + _line(_empty(), _empty(), "b") + "\n")
    base = [CLI, "--world", WORLD, "-c", str(tmp_path / "ck")]
    for extra, expect in ((["--refine", str(one), "--gpus", "2"], "--refine runs on one device"),
                          (["--refine", str(two)], "--refine needs a file with one plan"),
                          (["--refine", str(one), "--evaluate", str(one)], "separate runs"),
                          (["--refine", str(one), "--sensitivity", str(one)], "separate runs"),
                          (["--refine-rounds", "3"], "need --refine"),
                          (["--refine-replace", "3,4"], "need --refine"),
                          (["--refine-append", "3"], "need --refine"),
                          (["--refine", str(one), "--refine-replace", "3,61"], "--refine-replace needs a comma-separated list of canonical actions 0..60"),
                          (["--refine", str(one), "--refine-append", "61"], "--refine-append needs a comma-separated list of canonical actions 0..60"),
                          (["--refine", str(one), "--refine-rounds", "0"], "--refine-rounds needs a number")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and expect in out.stderr, (extra, out.stdout + out.stderr)
        assert "World:" not in out.stdout and not (tmp_path / "ck").exists()


def test_saved_plans_round_trip_through_eg_plans_load(built, tmp_path):
    rng = np.random.default_rng(1)
    plans = [Plan([[int(a) for a in rng.integers(0, 61, int(rng.integers(0, 9)))] for _ in range(26)],
                  [[int(a) for a in rng.choice([24, 21, 36, 0, 60], int(rng.integers(0, 4)))] for _ in range(26)], name) for name in ("refined", 'a "quoted", name', "")]
    plans.append(Plan([list(range(61))] + _empty()[1:], _empty(), "every action"))
    plans.append(Plan(_empty(), _empty(), "empty"))
    path = tmp_path / "refined.jsonl"
    Plan.save(path, plans)
    text = path.read_text()
    assert text.count("\n") == len(plans) and text.endswith("\n")      # JSON Lines: a plan a line
    back = Plan.load(path)
    assert back == plans and [p.name for p in back] == [p.name for p in plans]
    Plan.save(path, plans[:1])      # one plan: a file --refine and --evaluate both accept
    assert Plan.load(path) == plans[:1]
    L = N.lib()
    assert L.eg_plans_save(None, str(path).encode()) == N.EG_ERR_BAD_ARG and "NULL plan set" in L.eg_last_error().decode()


# ---------------------------------------------------------------- the definition over the tabled oracle
def test_short_base_cost_only_resolves_a_tie_and_stops_at_the_optimum(world):
    pol, base, ev, (plan, steps, stop, start, ties) = oracle_run(world, "short, mode 2")
    assert len(base) == 67 and sum(len(l) for l in base.best_deficit_actions) == 104
    assert [s[2] for s in steps] == [239]
    # twenty variants at the maximum: the lowest wins; then 230 of the 238 variants, the base among them, tied at the maximum: the base wins
    assert [s[1] for s in steps] == [1] and ties == [20, 230]
    assert stop == "local_optimum" and steps[0][4] == 2.0 and start < 2.0
    assert all(s[3] == 0 for s in steps)
    assert plan == apply_edit(base, steps[0][0])


def test_short_base_improves_strictly_for_eight_rounds(world):
    pol, base, ev, (plan, steps, stop, start, ties) = oracle_run(world, "short, mode 1")
    assert stop == "max_rounds" and len(steps) == 8
    scores = [start] + [s[4] for s in steps]
    assert all(b > a for a, b in zip(scores, scores[1:])), scores
    assert ties[5] == 2 and ties[7] == 2 and all(t == 1 for k, t in enumerate(ties) if k not in (5, 7)), ties
    assert all(s[3] == 0 and s[2] == 239 for s in steps)      # (every winner a replace: 239 variants in every round)


@pytest.mark.parametrize("mode", [1, 2])
def test_long_base_takes_the_four_deletes(world, mode):
    pol, base, ev, (plan, steps, stop, start, ties) = oracle_run(world, f"long, mode {mode}")
    assert len(base) == 272 and sum(len(l) for l in base.best_deficit_actions) == 104
    assert stop == "max_rounds" and [s[1] for s in steps] == [18, 77, 102, 105]
    assert [s[2] for s in steps] == [377, 376, 375, 374]
    assert all(s[0].kind == "delete" and s[0].list == 0 for s in steps) and _deleted_actions(base, steps) == [17] * 4      # (nuclear plants at 150 %)
    scores = [start] + [s[4] for s in steps]
    assert all(b > a for a, b in zip(scores, scores[1:])), scores
    want = {1: (1.4472, 1.4533, 1.4591, 1.4651, 1.4711), 2: (1.3814,)}[mode]
    assert [round(v, 4) for v in scores[:len(want)]] == list(want), scores
    if mode == 2:
        assert round(scores[-1], 4) == 1.4091, scores
    assert all(s[3] == 0 for s in steps)


def _deleted_actions(base, steps):
    plan, out = base, []
    for s in steps:
        e = s[0]
        out.append((plan.best_actions, plan.best_deficit_actions)[e.list][e.year][e.pos])
        plan = apply_edit(plan, e)
    return out
