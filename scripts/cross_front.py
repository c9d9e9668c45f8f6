"""Cross every pair of plans of a file: a Pareto front (scripts/pareto_front.py plans.jsonl), the scenarios of --top-k, any JSON Lines file of
up to 256 plans — each plan's first years followed by another's last years, for every pair and every cut year — and keep what no
other variant dominates.

    python scripts/cross_front.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --out run1
    python scripts/cross_front.py --world W --plans FILE --policy CKPT --seed S --cuts 2030,2035,2040 --cost-only --out DIR

Engine.cross_front (include/eirgrid_hip.h eg_evaluate_plan_crosses) evaluates the plans themselves and all their one-cut children, every
variant at global index 0 of the seed, 16 384 a batch, and filters them with the Pareto archive's definitions; this script writes
    DIR/cross/index.csv     a row per front entry, in variant order: the variant's number, the two parents' positions and names, the cut
                            year (the first year taken from parent b; empty for a plan of the file itself), the four metrics and the
                            score as %.17g, and is_parent
    DIR/cross/plans.jsonl   the front's plans (eg_plans_save), a child named `A>B@2037` after its parents and its cut, a plan of the file
                            by its own name: `eirgrid-hip --evaluate` and scripts/refine_front.py read it
--cuts takes the years 2026..2050 a child may switch parents at (default: all 25).  --world takes a world as World.to_json_dict writes
it, or the word `synthetic`; without --policy the plans are evaluated under a fresh policy.  The `eirgrid-hip` binary has no flag for
this yet."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")


def years(text):
    try:
        out = [int(part) for part in text.split(",")]
    except ValueError:
        out = [0]
    if not out or any(not 2026 <= y <= 2050 for y in out):
        raise argparse.ArgumentTypeError("a comma-separated list of years 2026..2050")
    return out


def g17(x):
    return "%.17g" % x


def child_name(parents, x):
    """a front entry's name: a plan of the file keeps its own, a child is `A>B@year`, the year being the first one taken from B (a plan
    without a name goes by its position in the file)"""
    name = lambda p: parents[p].name or str(p)
    if x.a == x.b or x.from_year == x.to_year:
        return parents[x.a].name
    return f"{name(x.a)}>{name(x.b)}@{2025 + x.from_year}"


def write(out_dir, parents, front):
    """index.csv and plans.jsonl from Engine.cross_front's result; returns the directory."""
    from eirgrid_amd.engine import Plan
    d = os.path.join(out_dir, "cross")
    os.makedirs(d, exist_ok=True)
    plans = []
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("variant", "a", "a_name", "b", "b_name", "cut") + METRICS + ("score", "is_parent"))
        for j, x in enumerate(front.crosses):
            own = bool(front.is_parent[j])
            w.writerow([int(front.variant[j]), x.a, parents[x.a].name, x.b, parents[x.b].name, "" if own else 2025 + x.from_year] +
                       [g17(v) for v in front.metrics[j]] + [g17(front.score[j]), int(own)])
            child = x.apply(parents)
            plans.append(Plan(child.best_actions, child.best_deficit_actions, child_name(parents, x)))
    Plan.save(os.path.join(d, "plans.jsonl"), plans)
    return d


def main():
    ap = argparse.ArgumentParser(description="The non-dominated plans among a file's plans and their one-cut crossovers: index.csv and plans.jsonl under DIR/cross/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of 1..256 plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--cuts", type=years, default=list(range(2026, 2051)), help="years a child may switch parents at, e.g. 2030,2035 (default: 2026..2050)")
    ap.add_argument("--cost-only", action="store_true", help="score by the cost-only score")
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, apply_constraints
    add_constraint_arguments(ap)
    from eirgrid_amd.streams import add_stream_arguments, apply_streams
    add_stream_arguments(ap)
    a = ap.parse_args()
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    world = synthetic_world() if a.world == "synthetic" else World.from_json_dict(json.load(open(a.world)))
    parents = Plan.load(a.plans)
    if len(parents) > 256:
        ap.error(f"--plans holds {len(parents)} plans (at most 256)")
    policy = ActionWeights.load_from_file(a.policy) if a.policy else ActionWeights()
    eng = Engine(world, device=0)
    try:
        apply_constraints(eng, a)      # --constraint: every plan batch below is judged under them
        apply_streams(eng, a)          # --streams R [--tail K]: ... over R draw streams, and ranked by committed outcomes
        front = eng.cross_front(policy, parents, a.seed, 0, cost_only=a.cost_only, cuts=[y - 2025 for y in a.cuts])
    finally:
        eng.close()
    d = write(a.out, parents, front)
    print(f"{len(parents)} plans, {front.n_variants} variants ({front.n_valid} valid): a front of {len(front.variant)} "
          f"({int(front.is_parent.sum())} of them plans of the file) -> {d}")


if __name__ == "__main__":
    main()
