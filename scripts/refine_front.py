"""Refine every plan of a file in one call: a Pareto front (scripts/pareto_front.py plans.jsonl), the scenarios of --top-k, any JSON Lines
file of up to 256 plans.

    python scripts/refine_front.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --out run1
    python scripts/refine_front.py --world W --plans FILE --policy CKPT --seed S --rounds 8 --replace 12,14 --append 14 --cost-only --out DIR

Engine.refine_plans (include/eirgrid_hip.h eg_refine_plans) steps the rounds of all plans together — per plan exactly what
`eirgrid-hip --refine` gives for that plan alone, as iteration 0 of the seed — and this script writes
    DIR/refine/index.csv          a row per plan: its position and name, the stop reason, the steps taken, the start and the final score and
                                  the refined plan's four metrics, as %.17g (nan where the base plan failed)
    DIR/refine/trajectories.csv   the columns of the CLI's refine/trajectory.csv behind a leading `plan` column (the plan's position in
                                  the file): per plan the start row, then a row per applied edit
    DIR/refine/refined.jsonl      all refined plans in the file's order, names kept (eg_plans_save): `eirgrid-hip --evaluate` reads it
With --shift N (Engine.refine_plans max_shift, eg_refine_plans_moves) a round also tries every best_actions entry N years earlier and
later at most; trajectories.csv then has kind `move` for such a step — list, year and pos say where the entry was, action what it is — and
two more columns at the end of every row, to_year and to_pos (empty where the row is no move).  Without --shift the three files are what
they have always been.
--world takes a world as World.to_json_dict writes it, or the word `synthetic`; without --policy the plans are evaluated under a fresh
policy."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")


def actions(text):
    try:
        out = [int(part) for part in text.split(",")]
    except ValueError:
        out = [-1]
    if not out or any(not 0 <= a <= 60 for a in out):
        raise argparse.ArgumentTypeError("a comma-separated list of canonical actions 0..60")
    return out


def g17(x):
    return "%.17g" % x


def write(out_dir, bases, results, shift=False):
    """The three files from Engine.refine_plans' result; returns the directory.  shift: the run tried moves (two more columns)."""
    from eirgrid_amd.engine import Plan, PlanMove
    d = os.path.join(out_dir, "refine")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "name", "stop", "steps", "start_score", "final_score") + METRICS)
        for p, (plan, steps, stop, start, rec) in enumerate(results):
            final = steps[-1].score if steps else start
            metrics = [g17(v) for v in rec.metrics[0]] if rec is not None else ["nan"] * 4
            w.writerow([p, bases[p].name, stop, len(steps), g17(start), g17(final)] + metrics)
    with open(os.path.join(d, "trajectories.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "round", "kind", "list", "year", "pos", "action", "variant", "n_variants", "n_failed", "score") + METRICS +
                   (("to_year", "to_pos") if shift else ()))
        for p, (plan, steps, stop, start, rec) in enumerate(results):
            w.writerow([p, "start", "none", "", "", "", "", 0, "", "", g17(start), "", "", "", ""] + (["", ""] if shift else []))
            at = bases[p]      # the plan of the round, for the action a move carries
            for r, s in enumerate(steps):
                e = s.edit
                move = isinstance(e, PlanMove)
                kind = "move" if move else e.kind
                action = (at.best_actions, at.best_deficit_actions)[e.list][e.year][e.pos] if move else ("" if kind == "delete" else e.action)
                w.writerow([p, r, kind, ("best_actions", "best_deficit_actions")[e.list], 2025 + e.year, e.pos, action,
                            s.variant, s.n_variants, s.n_failed, g17(s.score)] + [g17(v) for v in s.metrics] +
                           (([2025 + e.to_year, e.to_pos] if move else ["", ""]) if shift else []))
                if shift:
                    at = e.apply(at)
    Plan.save(os.path.join(d, "refined.jsonl"), [r[0] for r in results])
    return d


def main():
    ap = argparse.ArgumentParser(description="Refine every plan of a file in one call: index.csv, trajectories.csv and refined.jsonl under DIR/refine/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of 1..256 plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--rounds", type=int, default=64, help="steps a plan takes at most (default 64)")
    ap.add_argument("--replace", type=actions, default=[], help="actions every best_actions entry is replaced by, e.g. 12,14")
    ap.add_argument("--append", type=actions, default=[], help="actions appended to every year's best_actions list")
    ap.add_argument("--cost-only", action="store_true", help="rank by the cost-only score")
    ap.add_argument("--shift", type=int, default=0, help="also try every best_actions entry up to N years earlier and later (default 0: no moves)")
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, apply_constraints
    add_constraint_arguments(ap)
    from eirgrid_amd.streams import add_stream_arguments, apply_streams
    add_stream_arguments(ap)
    a = ap.parse_args()
    if a.rounds < 1:
        ap.error("--rounds must be at least 1")
    if not 0 <= a.shift <= 25:
        ap.error("--shift takes 0..25 years")
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
        results = eng.refine_plans(policy, bases, a.seed, 0, 2 if a.cost_only else 1, a.rounds, replace_with=a.replace, append_with=a.append, max_shift=a.shift)
    finally:
        eng.close()
    d = write(a.out, bases, results, shift=a.shift > 0)
    moved = sum(1 for r in results if r[1])
    print(f"refined {len(results)} plans ({moved} moved, {sum(len(r[1]) for r in results)} steps in all) -> {d}")


if __name__ == "__main__":
    main()
