"""What is a technology worth to a plan?  For every plan of a file — a Pareto front (scripts/pareto_front.py plans.jsonl), the scenarios of
--top-k, any JSON Lines file of plans — the plan itself and the plan WITHOUT each generator type its best_actions uses, and with --replace
the plan with one type built as another.

    python scripts/plan_technologies.py --world tests/golden/world_v1.json --plans run1/pareto/plans.jsonl --seed 1 --out run1
    python scripts/plan_technologies.py --world W --plans FILE --policy CKPT --seed S --cost-only --deficit keep --replace 1:0,Nuclear:GasCombinedCycle --out DIR

Engine.technology_report (include/eirgrid_hip.h eg_evaluate_plan_rewrites) evaluates every variant at global index 0 of the seed, 16 384 a
batch, the variants' plan blocks written on the device from an action map each; this script writes
    DIR/technologies/index.csv     a row per plan and technology, the plan itself first (technology empty): the plan's position and name,
                                   the type taken out, what replaced it (--replace rows, behind the others), the best_actions entries
                                   that removed or changed, the status, the four metrics, the score and the score minus the plan's own
                                   as %.17g
    DIR/technologies/plans.jsonl   the rows' plans (eg_plans_save) in the rows' order, named `NAME-Nuclear` and
                                   `NAME:OffshoreWind>OnshoreWind`, a plan of the file by its own name: `eirgrid-hip --evaluate`,
                                   scripts/refine_front.py, cross_front.py, breed_front.py and explore_front.py read it
--deficit says what happens to the type in best_deficit_actions: `substitute` (default) builds battery storage at 100 % in its place —
a deficit list that runs short is refilled by seeded draws from the fallback distribution, gas peakers among them, so dropping there
does not take a technology out —, `keep` leaves that list alone.  --replace takes pairs t:u of generator type indices 0..14 or names;
both lists change, the cost tier is kept.  --world takes a world as World.to_json_dict writes it, or the word `synthetic`; without
--policy the plans are evaluated under a fresh policy.  The `eirgrid-hip` binary has no flag for this yet."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("net_emissions", "public_opinion", "total_cost", "power_reliability")


def replacements(text):
    from eirgrid_amd.world import GENERATOR_TYPE_NAMES as NAMES
    def one(word):
        return NAMES.index(word) if word in NAMES else int(word)
    try:
        out = [tuple(one(w) for w in part.split(":")) for part in text.split(",")]
    except ValueError:
        out = [()]
    if any(len(p) != 2 or not all(0 <= t < len(NAMES) for t in p) or p[0] == p[1] for p in out):
        raise argparse.ArgumentTypeError("a comma-separated list of pairs t:u of different generator types (0..14 or their names)")
    return out


def g17(x):
    return "%.17g" % x


def write(out_dir, plans, report, replaced=(), deficit="substitute", substitute_with=36):
    """index.csv and plans.jsonl from Engine.technology_report's rows and the --replace variants [(plan, t, u, child, row)]; returns the
    directory."""
    from eirgrid_amd.engine import Plan, technology_rewrites
    from eirgrid_amd.world import GENERATOR_TYPE_NAMES as NAMES
    d = os.path.join(out_dir, "technologies")
    os.makedirs(d, exist_ok=True)
    parents, maps, rewrites, rows = technology_rewrites(plans, deficit, substitute_with)
    assert [(r.plan, r.type, r.removed) for r in report] == rows, "the report is not this file's"
    name = lambda p: plans[p].name or str(p)
    out = []
    with open(os.path.join(d, "index.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(("plan", "plan_name", "technology", "replaced_by", "removed", "status") + METRICS + ("score", "delta"))
        line = lambda r, tech, by: [r.plan, plans[r.plan].name, tech, by, r.removed, r.status] + [g17(v) for v in r.metrics] + [g17(r.score), g17(r.delta)]
        for r, rw in zip(report, rewrites):
            w.writerow(line(r, "" if r.type < 0 else NAMES[r.type], ""))
            child = rw.apply(parents, maps)
            out.append(Plan(child.best_actions, child.best_deficit_actions, plans[r.plan].name if r.type < 0 else f"{name(r.plan)}-{NAMES[r.type]}"))
        for p, t, u, child, r in replaced:
            w.writerow(line(r, NAMES[t], NAMES[u]))
            out.append(Plan(child.best_actions, child.best_deficit_actions, f"{name(p)}:{NAMES[t]}>{NAMES[u]}"))
    Plan.save(os.path.join(d, "plans.jsonl"), out)
    return d


def main():
    ap = argparse.ArgumentParser(description="Every plan of a file without each technology it uses: index.csv and plans.jsonl under DIR/technologies/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("--plans", required=True, help="a file of plans (JSON Lines in the checkpoint schema, or one checkpoint)")
    ap.add_argument("--policy", help="a policy checkpoint to evaluate the plans under (default: a fresh policy)")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--cost-only", action="store_true", help="score by the cost-only score")
    ap.add_argument("--deficit", choices=("substitute", "keep"), default="substitute", help="the type in best_deficit_actions: battery storage in its place, or left alone")
    ap.add_argument("--replace", type=replacements, default=[], help="pairs t:u, e.g. 1:0,Nuclear:GasCombinedCycle: type t built as type u")
    ap.add_argument("--out", required=True, help="output directory")
    from eirgrid_amd.constraints import add_constraint_arguments, apply_constraints
    add_constraint_arguments(ap)
    from eirgrid_amd.streams import add_stream_arguments, apply_streams
    add_stream_arguments(ap)
    a = ap.parse_args()
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionMap, ActionWeights, Engine, Plan, PlanRewrite, TechnologyRow, rank_score
    from eirgrid_amd.world import World
    world = synthetic_world() if a.world == "synthetic" else World.from_json_dict(json.load(open(a.world)))
    plans = Plan.load(a.plans)
    policy = ActionWeights.load_from_file(a.policy) if a.policy else ActionWeights()
    eng = Engine(world, device=0)
    try:
        apply_constraints(eng, a)      # --constraint: every plan batch below is judged under them
        apply_streams(eng, a)          # --streams R [--tail K]: ... over R draw streams, and ranked by committed outcomes
        report = eng.technology_report(policy, plans, a.seed, 0, cost_only=a.cost_only, deficit=a.deficit)
        own = {r.plan: r.score for r in report if r.type < 0}
        replaced = []
        maps = [ActionMap.replace_technology(t, u) for t, u in a.replace]
        for first in range(0, len(plans) if maps else 0, 256):      # (a set holds at most 256 plans)
            some = plans[first:first + 256]
            rewrites = [PlanRewrite(p, m, 0, 26, 3) for p in range(len(some)) for m in range(len(maps))]
            for lo in range(0, len(rewrites), 16384):
                res = eng.evaluate_plan_rewrites(policy, some, maps, rewrites[lo:lo + 16384], a.seed, 0, write_yearly=False)
                for j, rw in enumerate(rewrites[lo:lo + 16384]):
                    t, u = a.replace[rw.map]
                    score = rank_score(res.metrics[j], a.cost_only)
                    changed = sum(1 for l in some[rw.plan].best_actions for e in l if e // 3 == t)
                    row = TechnologyRow(first + rw.plan, t, changed, int(res.status[j]), tuple(float(v) for v in res.metrics[j]), score, score - own[first + rw.plan])
                    replaced.append((first + rw.plan, t, u, rw.apply(some, maps), row))
    finally:
        eng.close()
    d = write(a.out, plans, report, replaced, a.deficit)
    print(f"{len(plans)} plans, {len(report) + len(replaced)} variants -> {d}")


if __name__ == "__main__":
    main()
