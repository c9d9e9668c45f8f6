"""What G generations of a Pareto local search over plan edits cost end to end on the device (include/eirgrid_hip.h eg_explore_plans: the
archive lives on the device across the generations, the members that entered become the next frontier in k_breed_gather /
k_explore_turnover, one readback per generation) against the host loop that was the only way before it: per generation every frontier
member's neighbourhood through Engine.evaluate_plan_edits / evaluate_plan_moves (the base uploaded whole, 36 bytes per variant read
back), the front filtered in numpy with pareto_filter, every new member built on the host with PlanEdit.apply / PlanMove.apply.

    python scripts/explore_probe.py [--front 16] [--generations 3] [--shift 1] [--reps 5]

The start plans are the Pareto front of a short training run on tests/golden/world_v1.json (a few steps of 1 024 episodes with an archive
of --front entries); the neighbourhood is the deletes and the moves of up to --shift years.  Both forms run in one process on one build:
a warm-up of each, then --reps INTERLEAVED repeats (device, host, device, ...), each the wall time of the whole call.  The host loop has
no capacity rule: as long as the cap of 256 is never filled (dropped = 0) both forms must arrive at the same front, and the script checks
that (same_population; null once something was dropped).  Reports the medians, the spread and the ratio of the medians.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def summary(walls):
    return {"median_ms": float(np.median(walls)), "min_ms": float(min(walls)), "max_ms": float(max(walls)), "all_ms": [round(w, 3) for w in walls]}


def host_loop(eng, pol, starts, seed, generations, max_shift, mask=15):
    """the parent commit's way; returns (the front's plans in ascending number, variants evaluated)"""
    from eirgrid_amd.engine import PlanEdit, pareto_filter, refine_edits, refine_moves
    n = len(starts)
    plans = {p: s for p, s in enumerate(starts)}
    fi, fm = np.zeros(0, np.int64), np.zeros((0, 4))
    frontier, number = list(range(n)), 0
    for g in range(generations):
        gen_first, variants, metrics, status, nones = number, ([None] * n if g == 0 else []), [], [], []
        for k in frontier:
            edits, moves = refine_edits(plans[k])[1:], refine_moves(plans[k], max_shift)
            if g == 0 or edits:
                cnt = len(edits) + (g == 0)
                res = eng.evaluate_plan_edits(pol, plans[k], ([PlanEdit()] if g == 0 else []) + edits, seed, 0, True, write_yearly=False)
                m, s = res.metrics[:cnt], res.status[:cnt]
                if g == 0:
                    nones.append((m[0], s[0])); m, s = m[1:], s[1:]
                metrics.append(m); status.append(s)
            if moves:
                res = eng.evaluate_plan_moves(pol, plans[k], moves, seed, 0, True, write_yearly=False)
                metrics.append(res.metrics[:len(moves)]); status.append(res.status[:len(moves)])
            variants += [(k, e) for e in edits + moves]
        metrics = np.concatenate([np.array([m for m, _ in nones]).reshape(-1, 4)] + metrics).reshape(-1, 4)
        status = np.concatenate([np.array([s for _, s in nones], np.int32)] + status)
        number += len(variants)
        fi, fm = pareto_filter(fi, fm, np.arange(gen_first, number), metrics, status, mask)
        frontier = [int(k) for k in fi if k >= gen_first + (n if g == 0 else 0)]
        for k in frontier:
            parent, edit = variants[k - gen_first]
            plans[k] = edit.apply(plans[parent])
        if not frontier:
            break
    return [plans[int(k)] for k in fi], number


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--front", type=int, default=16, help="entries of the training run's Pareto archive: the start plans (at most)")
    ap.add_argument("--steps", type=int, default=4, help="training steps of 1 024 episodes")
    ap.add_argument("--generations", type=int, default=3)
    ap.add_argument("--shift", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    a = ap.parse_args()
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    eng = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    try:
        eng.push(ActionWeights())
        eng.track_pareto(a.front)
        for step in range(a.steps):
            eng.device_step(a.seed, 1024 * step, 1024, 10, a.seed + step)
        res, index = eng.fetch_pareto()[:2]
        starts = [Plan.from_result(res, e, f"episode {int(index[e])}") for e in range(len(index))]
        pol = ActionWeights()

        def device():
            return eng.explore_front(pol, starts, a.seed, 0, generations=a.generations, cap=256, max_shift=a.shift)

        def host():
            return host_loop(eng, pol, starts, a.seed, a.generations, a.shift)
        front = device(); pop, total = host()      # warm-up: pools and buffers sized
        dropped = front.generations[-1].n_dropped
        same = (front.plans == pop and sum(g.n_variants for g in front.generations) == total) if dropped == 0 else None
        walls = {"device": [], "host": []}
        for _ in range(a.reps):
            for form, call in (("device", device), ("host", host)):
                eng.sync()
                t0 = time.perf_counter()
                call()
                eng.sync()
                walls[form].append(1e3 * (time.perf_counter() - t0))
        out = {"starts": len(starts), "generations": [[g.n_frontier, g.n_variants, g.n_held, g.n_new] for g in front.generations], "stop": front.stop_reason,
               "variants": sum(g.n_variants for g in front.generations), "dropped": dropped, "same_population": same, "reps": a.reps,
               "device": summary(walls["device"]), "host": summary(walls["host"])}
        out["host_over_device"] = out["host"]["median_ms"] / out["device"]["median_ms"]
        print(json.dumps(out))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
