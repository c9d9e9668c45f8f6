"""Repair every plan of a file under plan constraints: the smallest run of one-entry changes that makes each plan legal, and what it costs.

    python scripts/repair_plans.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 \\
        --constraint "net_co2 <= 0 @2040" --constraint "balance >= 500" --out run1
    python scripts/repair_plans.py --world W --plans FILE --seed S --policy CKPT --constraint SPEC --weight 1,0.001 --rounds 16 \\
        --replace 12,14 --append 14 --shift 1 --cost-only --then-refine --out DIR

Engine.repair_plans (include/eirgrid_hip.h eg_repair_plans) descends, per plan, on the violation measure V of the constraints — the sum of
the weighted positive excesses — through the neighbourhood of Engine.refine_plans (--replace, --append, --shift), all plans stepped
together on the device, as iteration 0 of the seed.  It writes
    DIR/repair/index.csv          a row per plan: its position and name, the stop reason (feasible | max_rounds | base_failed | stuck), the
                                  steps taken, the start and the final V, the returned plan's score and four metrics, as %.17g (nan where
                                  the base plan failed), and the constraints it still violates, `;`-separated
    DIR/repair/trajectories.csv   per plan the start row, then a row per applied step: kind (delete | replace | insert | move), list,
                                  year, pos, action, variant, n_variants, n_failed, n_feasible, the violated mask, V, score, the four
                                  metrics, and to_year / to_pos (empty where the row is no move)
    DIR/repair/repaired.jsonl     all plans as the descent left them, in the file's order, names kept (eg_plans_save): the front scripts
                                  and `eirgrid-hip --evaluate` read it
--weight gives one weight per --constraint, in their order (default 1 each).  --then-refine hands the plans that ended `feasible` to
Engine.refine_plans under the same constraints and neighbourhood and writes DIR/refine/ as scripts/refine_front.py does: the cheapest
legal plan near each repaired one.
--world takes a world as World.to_json_dict writes it, or the word `synthetic`; without --policy the plans are evaluated under a fresh
policy."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")


def floats(text):
    try:
        out = [float(part) for part in text.split(",")]
    except ValueError:
        out = []
    if not out or any(not (0.0 < w < float("inf")) for w in out):
        raise argparse.ArgumentTypeError("a comma-separated list of finite weights > 0")
    return out


def write(out_dir, bases, results, constraints, cost_only):
    """The three files from Engine.repair_plans' result; returns the directory."""
    from eirgrid_amd.constraints import record_violates
    from eirgrid_amd.engine import Plan, PlanMove, rank_score
    from refine_front import g17
    d = os.path.join(out_dir, "repair")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "name", "stop", "steps", "start_violation", "final_violation", "score") + METRICS + ("violated",))
        for p, (plan, steps, stop, start, final, rec) in enumerate(results):
            metrics = [g17(v) for v in rec.metrics[0]] if rec is not None else ["nan"] * 4
            score = g17(rank_score(rec.metrics[0], cost_only)) if rec is not None else "nan"
            still = ";".join(str(c) for c in constraints if rec is not None and record_violates(c, rec, 0))
            w.writerow([p, bases[p].name, stop, len(steps), g17(start), g17(final), score] + metrics + [still])
    with open(os.path.join(d, "trajectories.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "round", "kind", "list", "year", "pos", "action", "variant", "n_variants", "n_failed", "n_feasible", "violated", "violation", "score") +
                   METRICS + ("to_year", "to_pos"))
        for p, (plan, steps, stop, start, final, rec) in enumerate(results):
            w.writerow([p, "start", "none", "", "", "", "", 0, "", "", "", "", g17(start), "", "", "", "", "", "", ""])
            at = bases[p]      # the plan of the round, for the action a move carries
            for r, s in enumerate(steps):
                e = s.edit
                move = isinstance(e, PlanMove)
                kind = "move" if move else e.kind
                action = (at.best_actions, at.best_deficit_actions)[e.list][e.year][e.pos] if move else ("" if kind == "delete" else e.action)
                w.writerow([p, r, kind, ("best_actions", "best_deficit_actions")[e.list], 2025 + e.year, e.pos, action, s.variant, s.n_variants, s.n_failed,
                            s.n_feasible, "0x%08x" % s.violated, g17(s.violation), g17(s.score)] + [g17(v) for v in s.metrics] +
                           ([2025 + e.to_year, e.to_pos] if move else ["", ""]))
                at = e.apply(at)
    Plan.save(os.path.join(d, "repaired.jsonl"), [r[0] for r in results])
    return d


def main():
    from refine_front import actions, write as write_refined
    ap = argparse.ArgumentParser(description="Repair every plan of a file under plan constraints: index.csv, trajectories.csv and repaired.jsonl under DIR/repair/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of 1..256 plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--weight", type=floats, default=None, metavar="x,...", help="one weight per --constraint, in their order (default: 1 each)")
    ap.add_argument("--rounds", type=int, default=64, help="steps a plan takes at most (default 64)")
    ap.add_argument("--replace", type=actions, default=[], help="actions every best_actions entry is replaced by, e.g. 12,14")
    ap.add_argument("--append", type=actions, default=[], help="actions appended to every year's best_actions list")
    ap.add_argument("--shift", type=int, default=0, help="also try every best_actions entry up to N years earlier and later (default 0: no moves)")
    ap.add_argument("--cost-only", action="store_true", help="break ties on the violation by the cost-only score")
    ap.add_argument("--then-refine", action="store_true", help="refine the plans that ended feasible under the same constraints (DIR/refine/)")
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, apply_constraints
    add_constraint_arguments(ap)
    a = ap.parse_args()
    if not a.constraint:
        ap.error("at least one --constraint is needed: a repair descends on their violation")
    if a.weight is not None and len(a.weight) != len(a.constraint):
        ap.error(f"--weight gives {len(a.weight)} weights for {len(a.constraint)} constraints")
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
    mode = 2 if a.cost_only else 1
    hood = dict(replace_with=a.replace, append_with=a.append, max_shift=a.shift)
    eng = Engine(world, device=0)
    refined = None
    try:
        constraints = apply_constraints(eng, a)
        results = eng.repair_plans(policy, bases, a.seed, 0, mode, a.rounds, violation_weights=a.weight, **hood)
        legal = [r[0] for r in results if r[2] == "feasible"]
        if a.then_refine and legal:
            refined = eng.refine_plans(policy, legal, a.seed, 0, mode, a.rounds, **hood)
    finally:
        eng.close()
    d = write(a.out, bases, results, constraints, a.cost_only)
    stops = [r[2] for r in results]
    print(f"repaired {len(results)} plans ({stops.count('feasible')} feasible, {stops.count('stuck')} stuck, {stops.count('max_rounds')} out of rounds, "
          f"{stops.count('base_failed')} failed; {sum(len(r[1]) for r in results)} steps in all) -> {d}")
    if refined is not None:
        d2 = write_refined(a.out, legal, refined, shift=a.shift > 0)
        print(f"refined the {len(legal)} feasible plans ({sum(len(r[1]) for r in refined)} steps in all) -> {d2}")


if __name__ == "__main__":
    main()
