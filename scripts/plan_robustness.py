"""How much of a plan's score is the luck of one draw stream: every plan of a file judged over R streams.

    python scripts/plan_robustness.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --streams 16 --tail 4 \\
        --constraint "net_co2 <= 0 @2040" --out run1

A replay reads no seeded draw only while its two lists last; a plan whose best_deficit_actions runs short falls back to sampled draws
and its outcome depends on the seed.  Under Engine.set_streams (include/eirgrid_hip.h eg_plan_streams_set) the plans are evaluated as
`eirgrid-hip --evaluate` evaluates them — plan j the replay episode at global index j of the seed — R times, stream r at index j + r,
and reduced on the device.  This script writes
    DIR/robustness/index.csv   a row per plan, from its eg_ensemble_row: position and name, the committed status (0: every stream ended
                               well; -4: a constraint is violated in some stream), the nominal score (stream 0: what one evaluation
                               reports) and the committed score (of the mean of the K worst streams), the smallest, mean and largest
                               stream score, the worst stream, in how many streams the plan ended well, was infeasible or failed, and
                               the nominal and the committed metrics, as %.17g
--tail K commits the mean of the K worst streams (default R, the mean outcome); --cost-only orders and scores by the cost-only score.
--world takes a world as World.to_json_dict writes it, or the word `synthetic`; without --policy the plans are evaluated under a fresh
policy."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "opinion", "cost", "reliability")


def write(out_dir, plans, ens, n_streams, cost_only):
    """index.csv from Engine.fetch_ensemble's rows; returns the directory"""
    from eirgrid_amd.engine import rank_score
    d = os.path.join(out_dir, "robustness")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["plan", "name", "status", "nominal_score", "committed_score", "score_min", "score_mean", "score_max", "worst_stream", "n_ok", "n_infeasible",
                    "n_failed"] + [f"nominal_{m}" for m in METRICS] + [f"committed_{m}" for m in METRICS])
        for p, plan in enumerate(plans):
            scores = [rank_score(ens.nominal[p], cost_only), rank_score(ens.committed[p], cost_only), ens.score_min[p], ens.score_sum[p] / n_streams, ens.score_max[p]]
            w.writerow([p, plan.name, int(ens.status[p])] + ["%.17g" % s for s in scores] +
                       [int(ens.worst_stream[p]), int(ens.n_ok[p]), int(ens.n_infeasible[p]), int(ens.n_failed[p])] +
                       ["%.17g" % v for v in ens.nominal[p]] + ["%.17g" % v for v in ens.committed[p]])
    return d


def main():
    ap = argparse.ArgumentParser(description="Judge the plans of a file over R draw streams: index.csv under DIR/robustness/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--cost-only", action="store_true", help="order the streams and score by the cost-only score")
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, apply_constraints
    from eirgrid_amd.streams import add_stream_arguments, apply_streams
    add_constraint_arguments(ap)
    add_stream_arguments(ap)
    a = ap.parse_args()
    if a.streams < 2:
        ap.error("--streams R with R >= 2 is needed")
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    world = synthetic_world() if a.world == "synthetic" else World.from_json_dict(json.load(open(a.world)))
    plans = Plan.load(a.plans)
    policy = ActionWeights.load_from_file(a.policy) if a.policy else ActionWeights()
    eng = Engine(world, device=0)
    try:
        apply_constraints(eng, a)      # --constraint: every stream is judged under them
        apply_streams(eng, a)
        eng.evaluate_plans(policy, plans, a.seed, 0)
        ens = eng.fetch_ensemble()
    finally:
        eng.close()
    d = write(a.out, plans, ens, a.streams, a.cost_only)
    spread = float((ens.score_max - ens.score_min).max()) if len(plans) else 0.0
    print(f"{len(plans)} plans over {a.streams} streams ({int((ens.n_ok == a.streams).sum())} ended well in every stream; the largest score spread is {spread:.6g}) -> {d}")


if __name__ == "__main__":
    main()
