"""What refining many plans costs: ONE eg_refine_plans call over P plans (include/eirgrid_hip.h; the rounds of all plans stepped together)
against the loop of P eg_refine_plan calls over the same plans — the path a caller had before, whose code the new call does not touch.

    python scripts/refine_many_probe.py [--plans 16,64] [--rounds 4] [--reps 5]

P copies of each of the two bases tests/test_refine.py pins with the tabled oracle: `short` (67 + 104 entries, replace_with=[12]: 239
variants a round) and `long` (272 + 104 entries, deletes only: 377 variants), seed 1234, index 0, mode 1 (both improve for at least four
rounds, so every plan runs all --rounds).  One process, one build: per base and P a warm-up of both forms, then --reps INTERLEAVED repeats
(the one call, the loop, the one call, ...), each the wall time between two synchronisations.  Reports the medians, the spread (min ..
max) and the ratio of the medians, and checks that both forms returned the same trajectories.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", default="16,64", help="comma-separated numbers of plans")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import Engine, Plan
    from tests.test_refine import long_policy, short_policy
    eng = Engine(synthetic_world(), device=0)
    out = {"rounds": a.rounds, "reps": a.reps}
    for name, pol, replace in (("short", short_policy(), [12]), ("long", long_policy(), None)):
        base = Plan.from_policy(pol)
        for P in [int(p) for p in a.plans.split(",")]:
            plans = [Plan(base.best_actions, base.best_deficit_actions, f"{name} {p}") for p in range(P)]

            def one_call():
                return [[s.score for s in r[1]] for r in eng.refine_plans(pol, plans, a.seed, 0, 1, a.rounds, replace_with=replace)]

            def loop():
                return [[s.score for s in eng.refine_plan(pol, p, a.seed, 0, 1, a.rounds, replace_with=replace)[1]] for p in plans]

            same = one_call() == loop(); eng.sync()      # warm-up: pools and buffers sized
            walls = {"one_call": [], "loop": []}
            for _ in range(a.reps):
                for form, call in (("one_call", one_call), ("loop", loop)):
                    eng.sync()
                    t0 = time.perf_counter()
                    scores = call()
                    eng.sync()
                    walls[form].append(1e3 * (time.perf_counter() - t0))
            row = {form: summary(w) for form, w in walls.items()}
            row.update(same_trajectories=bool(same), steps_per_plan=len(scores[0]), variants_round_0=1 + len(base) * (2 if replace else 1) + sum(len(l) for l in base.best_deficit_actions),
                       loop_over_one_call=row["loop"]["median_ms"] / row["one_call"]["median_ms"])
            out[f"{name} x{P}"] = row
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
