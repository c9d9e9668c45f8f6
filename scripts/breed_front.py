"""Breed a front: generations of scripts/cross_front.py without leaving the device.  From the plans of a file (a Pareto front, the
scenarios of --top-k, any JSON Lines file of up to 256 plans) every generation crosses every pair of the population at every cut year,
keeps what no other variant dominates — at most --cap plans — and makes those the next population.

    python scripts/breed_front.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --out run1
    python scripts/breed_front.py --world W --plans FILE --policy CKPT --seed S --generations 4 --cap 64 --cuts 2030,2035,2040 --cost-only --out DIR

Engine.breed_front (include/eirgrid_hip.h eg_breed_plans) evaluates every variant at global index 0 of the seed, 16 384 a launch, selects
with the Pareto archive's definitions on the device and stops when a generation keeps exactly its parents, after --generations
generations (default 8), or when nothing was valid; this script writes
    DIR/breed/index.csv        a row per plan of the final population, in order: its position, its name, its variant number in the last
                               generation with the two parents' positions in that generation's population and the cut year (empty for a
                               plan that was carried over), the four metrics and the score as %.17g
    DIR/breed/generations.csv  a row per generation that ran: the population it started from, the crosses skipped because a child would
                               outgrow a list, the variants evaluated and valid, what was kept (and how many of those are children) and
                               dropped for want of room; the last row carries the stop reason
    DIR/breed/plans.jsonl      the final population (eg_plans_save), a child named `A>B@2037` after its parents and its cut, a plan that was
                               carried over by its own name: `eirgrid-hip --evaluate`, scripts/refine_front.py and scripts/cross_front.py
                               read it
--cuts takes the years 2026..2050 a child may switch parents at (default: all 25).  --world takes a world as World.to_json_dict writes
it, or the word `synthetic`; without --policy the plans are evaluated under a fresh policy.  The `eirgrid-hip` binary has no flag for
this."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")
ROW = ("n_parents", "n_skipped", "n_variants", "n_valid", "n_kept", "n_children_kept", "n_dropped")


def years(text):
    try:
        out = [int(part) for part in text.split(",")]
    except ValueError:
        out = [0]
    if not out or len(out) > 25 or any(not 2026 <= y <= 2050 for y in out):
        raise argparse.ArgumentTypeError("a comma-separated list of at most 25 years 2026..2050")
    return out


def count(lo, hi, what):
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            v = lo - 1
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError(f"{what} {lo}..{hi}")
        return v
    return parse


def g17(x):
    return "%.17g" % x


def write(out_dir, front):
    """index.csv, generations.csv and plans.jsonl from Engine.breed_front's result; returns the directory."""
    from eirgrid_amd.engine import Plan
    d = os.path.join(out_dir, "breed")
    os.makedirs(d, exist_ok=True)
    last = front.members[-1] if front.members and front.members[-1] else [None] * len(front.plans)
    n_parents = front.generations[-1].n_parents if front.generations else len(front.plans)
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "name", "variant", "a", "b", "cut") + METRICS + ("score",))
        for r, (plan, m) in enumerate(zip(front.plans, last)):
            if m is None:      # (nothing was valid: the plans of the file, unscored)
                w.writerow([r, plan.name, "", "", "", ""] + [""] * 5)
                continue
            own = m.variant < n_parents
            w.writerow([r, plan.name, m.variant, m.cross.a, m.cross.b, "" if own else 2025 + m.cross.from_year] + [g17(v) for v in front.metrics[r]] +
                       [g17(front.score[r])])
    with open(os.path.join(d, "generations.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("generation",) + ROW + ("stop",))
        for g, row in enumerate(front.generations):
            w.writerow([g] + [getattr(row, k) for k in ROW] + [front.stop_reason if g == len(front.generations) - 1 else ""])
    Plan.save(os.path.join(d, "plans.jsonl"), front.plans)
    return d


def main():
    ap = argparse.ArgumentParser(description="Generations of one-cut crossovers with Pareto selection: index.csv, generations.csv and plans.jsonl under DIR/breed/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of 1..256 plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--generations", type=count(1, 1024, "a number of generations"), default=8, help="generations at most, 1..1024 (default 8)")
    ap.add_argument("--cap", type=count(1, 256, "a population size"), default=256, help="plans a generation keeps at most, 1..256 (default 256)")
    ap.add_argument("--cuts", type=years, default=list(range(2026, 2051)), help="years a child may switch parents at, e.g. 2030,2035 (default: 2026..2050)")
    ap.add_argument("--cost-only", action="store_true", help="score by the cost-only score")
    ap.add_argument("--keep", choices=("score", "spread"), default="score",
                    help="what stays when the front outgrows --cap: the best-scoring points, or a spread-out subset (default score)")
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
        front = eng.breed_front(policy, parents, a.seed, 0, cost_only=a.cost_only, cuts=[y - 2025 for y in a.cuts], generations=a.generations, cap=a.cap, keep=a.keep)
    finally:
        eng.close()
    d = write(a.out, front)
    kept = sum(g.n_children_kept for g in front.generations)
    print(f"{len(parents)} plans, {len(front.generations)} generations ({front.stop_reason}), {sum(g.n_variants for g in front.generations)} variants, "
          f"{kept} children kept on the way: a population of {len(front.plans)} -> {d}")


if __name__ == "__main__":
    main()
