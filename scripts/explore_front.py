"""Explore a front: a Pareto local search over one-entry edits and moves without leaving the device.  From the plans of a file (a Pareto
front, a bred population, any JSON Lines file of up to 256 plans) generation 0 evaluates the plans and every one-entry neighbour of
each — an entry deleted, replaced (--replace), appended to a year (--append), moved by up to --shift years —; every later generation
the neighbours of the plans that entered the front in the one before.  What no other variant dominates is kept, at most --cap plans,
in ONE archive that lives through the run: the trade-offs of the front stay apart, where scripts/refine_front.py pulls every plan
toward the same scalar optimum.

    python scripts/explore_front.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --out run1
    python scripts/explore_front.py --world W --plans FILE --policy CKPT --seed S --generations 4 --cap 64 --replace 3,17 --append 9 --shift 2
                                    --budget 2000000 --cost-only --out DIR

Engine.explore_front (include/eirgrid_hip.h eg_explore_plans) evaluates every variant at global index 0 of the seed, 16 384 a launch,
selects with the Pareto archive's definitions on the device and stops when no plan of the front is left unexplored, after --generations
generations (default 8), when the next generation would take the run beyond --budget variants (default: no budget), or when nothing
was valid; this script writes
    DIR/explore/index.csv        a row per plan of the final front, in ascending number: its position, its name, its number, the number
                                 of the plan it was made from (empty for a plan of the file), the four metrics and the score as %.17g
    DIR/explore/generations.csv  a row per generation that ran: the plans whose neighbours it evaluated, the variants evaluated and
                                 valid, what the front held after it, how many of those entered in it, and what was dropped for want
                                 of room so far; the last row carries the stop reason
    DIR/explore/plans.jsonl      the final front (eg_plans_save), a neighbour named after its base and its edit (`A-2031.2`,
                                 `A~2031.2=17`, `A+2040=9`, `A:2031.2>2033`), a plan of the file by its own name: `eirgrid-hip --evaluate`,
                                 scripts/breed_front.py and scripts/refine_front.py read it
--world takes a world as World.to_json_dict writes it, or the word `synthetic`; without --policy the plans are evaluated under a fresh
policy.  The `eirgrid-hip` binary has no flag for this."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")
ROW = ("n_frontier", "n_variants", "n_valid", "n_held", "n_new", "n_dropped")


def actions(text):
    try:
        out = [int(part) for part in text.split(",")]
    except ValueError:
        out = [-1]
    if not out or any(not 0 <= a <= 60 for a in out):
        raise argparse.ArgumentTypeError("a comma-separated list of canonical action indices 0..60")
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
    """index.csv, generations.csv and plans.jsonl from Engine.explore_front's result; returns the directory."""
    from eirgrid_amd.engine import Plan
    d = os.path.join(out_dir, "explore")
    os.makedirs(d, exist_ok=True)
    parent = {m.number: m.parent for row in front.members for m in row}
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "name", "number", "parent") + METRICS + ("score",))
        for r, plan in enumerate(front.plans):
            if front.records is None:      # (nothing was valid: the plans of the file, unscored)
                w.writerow([r, plan.name, "", ""] + [""] * 5)
                continue
            k = int(front.numbers[r])
            w.writerow([r, plan.name, k, "" if parent[k] < 0 else parent[k]] + [g17(v) for v in front.metrics[r]] + [g17(front.score[r])])
    with open(os.path.join(d, "generations.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("generation",) + ROW + ("stop",))
        for g, row in enumerate(front.generations):
            w.writerow([g] + [getattr(row, k) for k in ROW] + [front.stop_reason if g == len(front.generations) - 1 else ""])
    Plan.save(os.path.join(d, "plans.jsonl"), front.plans)
    return d


def main():
    ap = argparse.ArgumentParser(description="A Pareto local search over one-entry edits and moves: index.csv, generations.csv and plans.jsonl under DIR/explore/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of 1..256 plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--generations", type=count(1, 1024, "a number of generations"), default=8, help="generations at most, 1..1024 (default 8)")
    ap.add_argument("--cap", type=count(1, 256, "a front size"), default=256, help="plans the front holds at most, 1..256 (default 256)")
    ap.add_argument("--replace", type=actions, default=[], help="actions every best_actions entry is replaced by, e.g. 3,17 (default: none)")
    ap.add_argument("--append", type=actions, default=[], help="actions appended to every year's best_actions list (default: none)")
    ap.add_argument("--shift", type=count(0, 25, "a number of years"), default=0, help="years an entry may be moved by, 0..25 (default 0: no moves)")
    ap.add_argument("--budget", type=count(0, 2**62, "a number of variants"), default=0, help="variants the run may evaluate at most (default 0: no budget)")
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
    starts = Plan.load(a.plans)
    if len(starts) > 256:
        ap.error(f"--plans holds {len(starts)} plans (at most 256)")
    policy = ActionWeights.load_from_file(a.policy) if a.policy else ActionWeights()
    eng = Engine(world, device=0)
    try:
        apply_constraints(eng, a)      # --constraint: every plan batch below is judged under them
        apply_streams(eng, a)          # --streams R [--tail K]: ... over R draw streams, and ranked by committed outcomes
        front = eng.explore_front(policy, starts, a.seed, 0, cost_only=a.cost_only, generations=a.generations, cap=a.cap, replace_with=a.replace,
                                  append_with=a.append, max_shift=a.shift, max_variants=a.budget, keep=a.keep)
    finally:
        eng.close()
    d = write(a.out, front)
    print(f"{len(starts)} plans, {len(front.generations)} generations ({front.stop_reason}), {sum(g.n_variants for g in front.generations)} variants, "
          f"{sum(g.n_new for g in front.generations)} neighbours entered on the way: a front of {len(front.plans)} -> {d}")


if __name__ == "__main__":
    main()
