"""Which plans of a file meet which constraints on their yearly rows, and by how much.

    python scripts/plan_feasibility.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 \\
        --constraint "net_co2 <= 0 @2040" --constraint "sum(net_co2) <= 4e8" --constraint "balance >= 500" --out run1

Engine.plan_feasibility (include/eirgrid_hip.h eg_plan_constraints_set, eg_fetch_plan_feasibility) evaluates the plans as
`eirgrid-hip --evaluate` does — plan j the replay episode at global index j of the seed — judges the constraints on the device and this
script writes
    DIR/feasibility/index.csv   a row per plan: its position and name, its status (0 feasible, -4 infeasible, another negative number: the
                                plan failed on its own and was not judged), the violated constraints (their specs, joined by "; ") and
                                one `excess` column per constraint, as %.17g: <= 0 is satisfied and its negative is the slack, nan violates
--streams R [--tail K] judges every plan over R draw streams (Engine.set_streams): the status is then infeasible as soon as one stream
violates a constraint, the violated constraints and the excess columns are those of the first stream.
--world takes a world as World.to_json_dict writes it, or the word `synthetic`; without --policy the plans are evaluated under a fresh
policy."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write(out_dir, plans, constraints, status, violated, excess):
    """index.csv from Engine.plan_feasibility's result; returns the directory"""
    d = os.path.join(out_dir, "feasibility")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["plan", "name", "status", "violated"] + [f"excess {c}" for c in constraints])
        for p, plan in enumerate(plans):
            w.writerow([p, plan.name, int(status[p]), "; ".join(str(c) for c in violated[p])] + ["%.17g" % v for v in excess[p]])
    return d


def main():
    ap = argparse.ArgumentParser(description="Judge the plans of a file against constraints on their yearly rows: index.csv under DIR/feasibility/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, constraint_list
    add_constraint_arguments(ap)
    from eirgrid_amd.streams import add_stream_arguments, apply_streams
    add_stream_arguments(ap)
    a = ap.parse_args()
    if not a.constraint:
        ap.error("at least one --constraint is needed")
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    constraints = constraint_list(a.constraint)
    world = synthetic_world() if a.world == "synthetic" else World.from_json_dict(json.load(open(a.world)))
    plans = Plan.load(a.plans)
    policy = ActionWeights.load_from_file(a.policy) if a.policy else ActionWeights()
    eng = Engine(world, device=0)
    try:
        apply_streams(eng, a)      # --streams R [--tail K]: a plan is infeasible as soon as one stream violates; the excess columns stay stream 0's
        status, violated, excess = eng.plan_feasibility(policy, plans, a.seed, 0, constraints=constraints)
    finally:
        eng.close()
    d = write(a.out, plans, constraints, status, violated, excess)
    print(f"{int((status == 0).sum())} of {len(plans)} plans meet the {len(constraints)} constraints -> {d}")


if __name__ == "__main__":
    main()
