"""What repairing plans costs: ONE Engine.repair_plans call over P infeasible plans (include/eirgrid_hip.h eg_repair_plans: the rounds of
all plans stepped together, the pick on the device) against the only way to do it without the call — a host loop per plan and round over
evaluate_plan_edits / evaluate_plan_moves under the constraints, fetch_feasibility and a numpy pick by the header's definition.

    python scripts/repair_probe.py [--plans 16] [--rounds 4] [--shift 1] [--reps 5]

The two bases tests/test_refine.py pins with the tabled oracle: `short` (67 + 104 entries, replace_with=[12]) and `long` (272 + 104 entries),
seed 1234, index 0, mode 2, under a reserve on the balance equal to the base's own minimum.  The P starting plans are the base with one
entry deleted, taken from the deletes that dip under the reserve (cycled when there are fewer than P); append_with holds the deleted
actions, so a repair exists.  One process, one build: per base a warm-up of both forms, then --reps INTERLEAVED repeats (the call, the
loop, the call, ...), each the wall time between two synchronisations.  Reports the medians, the spread, the ratio of the medians and the
variants of round 0, and checks that both forms returned the same trajectories.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(walls):
    return {"median_ms": float(np.median(walls)), "min_ms": float(min(walls)), "max_ms": float(max(walls)), "all_ms": [round(w, 3) for w in walls]}


def host_loop(eng, pol, plan, seed, mode, rounds, hood):
    """eg_repair_plans for one plan on the host: (plan, [(variant, V)], stop)"""
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import rank_score, refine_edits, refine_moves
    steps = []
    while True:
        edits = refine_edits(plan, hood["replace_with"], hood["append_with"])
        moves = refine_moves(plan, hood["max_shift"]) if hood["max_shift"] else []
        res = eng.evaluate_plan_edits(pol, plan, edits, seed, 0, same_index=True)
        status, metrics, excess = res.status.copy(), res.metrics.copy(), eng.fetch_feasibility()[1]
        if moves:
            res = eng.evaluate_plan_moves(pol, plan, moves, seed, 0, same_index=True)
            status, metrics, excess = np.concatenate([status, res.status]), np.concatenate([metrics, res.metrics]), np.concatenate([excess, eng.fetch_feasibility()[1]])
        score = np.array([rank_score(m, mode == 2) for m in metrics])
        cand = ((status == N.EG_EP_OK) | (status == N.EG_EP_INFEASIBLE)) & ~np.isnan(score)
        with np.errstate(invalid="ignore"):
            t = np.where(np.isnan(excess), np.inf, np.where(excess > 0.0, 1.0 * excess, 0.0))
        V = np.zeros(len(status))
        for i in range(t.shape[1]):      # in constraint order, one rounding per addition
            V = V + t[:, i]
        if not cand[0]:
            return plan, steps, "base_failed"
        if V[0] == 0.0:
            return plan, steps, "feasible"
        below = np.flatnonzero(cand & (V < V[0]))
        if not len(below):
            return plan, steps, "stuck"
        w = int(min(below, key=lambda j: (V[j], -score[j], j)))
        plan = (edits + moves)[w].apply(plan)
        steps.append((w, float(V[w])))
        if V[w] == 0.0:
            return plan, steps, "feasible"
        if len(steps) == rounds:
            return plan, steps, "max_rounds"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--shift", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.constraints import Constraint
    from eirgrid_amd.engine import Engine, Plan, refine_edits, refine_moves
    from tests.test_refine import long_policy, short_policy
    eng = Engine(synthetic_world(), device=0)
    out = {"plans": a.plans, "rounds": a.rounds, "shift": a.shift, "reps": a.reps}
    for name, pol, replace in (("short", short_policy(), [12]), ("long", long_policy(), None)):
        base = Plan.from_policy(pol)
        edits = refine_edits(base)
        free = eng.evaluate_plan_edits(pol, base, edits, a.seed, 0, same_index=True)
        lows = free.yearly[:, :, 4].min(axis=1)
        dips = [j for j in range(1, len(edits)) if edits[j].list == 0 and lows[j] < lows[0]]
        if not dips:
            out[name] = "no delete dips under the base's reserve"
            continue
        picked = [dips[p % len(dips)] for p in range(a.plans)]
        starts = [edits[j].apply(base) for j in picked]
        plans = [Plan(q.best_actions, q.best_deficit_actions, f"{name} {p}") for p, q in enumerate(starts)]
        deleted = sorted({base.best_actions[edits[j].year][edits[j].pos] for j in picked})
        hood = dict(replace_with=replace, append_with=deleted, max_shift=a.shift)
        eng.set_constraints([Constraint("balance", ">=", float(lows[0]))])

        def one_call():
            return [([(s.variant, s.violation) for s in r[1]], r[2]) for r in eng.repair_plans(pol, plans, a.seed, 0, 2, a.rounds, **hood)]

        def loop():
            return [host_loop(eng, pol, p, a.seed, 2, a.rounds, hood)[1:] for p in plans]

        same = one_call() == loop(); eng.sync()      # warm-up: pools and buffers sized
        walls = {"one_call": [], "host_loop": []}
        for _ in range(a.reps):
            for form, call in (("one_call", one_call), ("host_loop", loop)):
                eng.sync()
                t0 = time.perf_counter()
                got = call()
                eng.sync()
                walls[form].append(1e3 * (time.perf_counter() - t0))
        eng.clear_constraints()
        row = {form: summary(w) for form, w in walls.items()}
        row.update(same_trajectories=bool(same), stops=sorted({g[1] for g in got}), steps=[len(g[0]) for g in got],
                   variants_round_0=len(refine_edits(plans[0], replace, deleted)) + (len(refine_moves(plans[0], a.shift)) if a.shift else 0),
                   distinct_starts=len(dips), host_loop_over_one_call=row["host_loop"]["median_ms"] / row["one_call"]["median_ms"])
        out[name] = row
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
