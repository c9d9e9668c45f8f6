"""Which entries of a plan would be better placed in another year: every plan of a file with each of its best_actions entries moved up to
N years earlier and later.

    python scripts/plan_timing.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --shift 2 --out run1

Engine.plan_timing (include/eirgrid_hip.h eg_evaluate_plan_moves) evaluates a plan and all its moves in one batch, every variant at
global index 0 of the seed, and this script writes
    DIR/timing/index.csv   a row per plan and move — row `move` 0 of a plan is the plan itself —: the plan's position and name, where the
                           entry was (year, pos, the action) and where it went (to_year, to_pos), the record's status, the four
                           metrics and the score as %.17g, and their differences from the plan's own row (nan where either failed)
--world takes a world as World.to_json_dict writes it, or the word `synthetic`; without --policy the plans are evaluated under a fresh
policy.  The `eirgrid-hip` binary has no flag for this yet."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")


def g17(x):
    return "%.17g" % x


def write(out_dir, bases, timings):
    """index.csv from one Engine.plan_timing result per plan; returns the directory."""
    d = os.path.join(out_dir, "timing")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "name", "move", "year", "pos", "action", "to_year", "to_pos", "status") + METRICS + ("score",) +
                   tuple("d_" + m for m in METRICS[:3]) + ("d_score",))
        for p, t in enumerate(timings):
            for j, m in enumerate(t.moves):
                where = ["", "", "", "", ""] if j == 0 or m is None else [2025 + m.year, m.pos, bases[p].best_actions[m.year][m.pos], 2025 + m.to_year, m.to_pos]
                w.writerow([p, bases[p].name, j] + where + [int(t.status[j])] + [g17(v) for v in t.metrics[j]] + [g17(t.score[j])] +
                           [g17(v) for v in t.d_metrics[j][:3]] + [g17(t.d_score[j])])
    return d


def main():
    ap = argparse.ArgumentParser(description="Every plan of a file with each best_actions entry moved to the years around it: DIR/timing/index.csv")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--shift", type=int, default=1, help="years an entry is moved earlier and later at most (default 1)")
    ap.add_argument("--cost-only", action="store_true", help="score by the cost-only score")
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, apply_constraints
    add_constraint_arguments(ap)
    from eirgrid_amd.streams import add_stream_arguments, apply_streams
    add_stream_arguments(ap)
    a = ap.parse_args()
    if not 1 <= a.shift <= 25:
        ap.error("--shift takes 1..25 years")
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    world = synthetic_world() if a.world == "synthetic" else World.from_json_dict(json.load(open(a.world)))
    bases = Plan.load(a.plans)
    policy = ActionWeights.load_from_file(a.policy) if a.policy else ActionWeights()
    eng = Engine(world, device=0)
    try:
        apply_constraints(eng, a)      # --constraint: every plan batch below is judged under them
        apply_streams(eng, a)          # --streams R [--tail K]: ... over R draw streams, and ranked by committed outcomes
        timings = [eng.plan_timing(policy, base, a.seed, 2 if a.cost_only else 1, a.shift) for base in bases]
    finally:
        eng.close()
    d = write(a.out, bases, timings)
    print(f"{len(bases)} plans, {sum(len(t.moves) - 1 for t in timings)} moves -> {d}")


if __name__ == "__main__":
    main()
