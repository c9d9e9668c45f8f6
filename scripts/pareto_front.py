"""The trade-off curve of a training run: every non-dominated outcome it simulated, with the plan that produced it.

    python scripts/pareto_front.py --world tests/golden/world_v1.json -n 65536 --batch 16384 --seed 1 --out run1
    python scripts/pareto_front.py --world W -n N --batch B --seed S --objectives e,c --cap 64 --cost-only --out DIR

Runs the device-resident training loop (Engine.device_step, every 10th episode a replay of the best strategy) from a fresh policy with
the Pareto archive on (include/eirgrid_hip.h eg_pareto_track) and writes
    DIR/pareto/index.csv      global index, the four metrics and the rank score of every entry, in ascending global index, as %.17g
    DIR/pareto/plans.jsonl    every entry's run_log / def_log per year as a plan (eg_plans_save) named by its global index: the lists
                              update_best_strategy would install, so `eirgrid-hip --evaluate` and scripts/refine_front.py read them back
                              (`--refine` takes a file with ONE plan)
--world takes a world as World.to_json_dict writes it, or the word `synthetic`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LETTERS = {"e": "emissions", "o": "opinion", "c": "cost", "r": "reliability"}
REPLAY_PERIOD = 10


def objectives(text):
    names = []
    for part in text.split(","):
        part = part.strip().lower()
        name = LETTERS.get(part, part)
        if name not in LETTERS.values() or name in names:
            raise argparse.ArgumentTypeError(f"--objectives: {part!r} is not one of e,o,c,r (each at most once)")
        names.append(name)
    return tuple(names)


def run(eng, n, batch, seed, cap, names, cost_only, keep="score"):
    """The loop: batches of `batch` episodes (the last one shorter) at global indices 0 .. n - 1; returns Engine.fetch_pareto()."""
    from eirgrid_amd.engine import ActionWeights
    eng.push(ActionWeights())
    eng.track_pareto(cap, names, cost_only=cost_only, keep=keep)
    first = 0
    while first < n:
        k = min(batch, n - first)
        eng.device_step(seed, first, k, REPLAY_PERIOD, seed + first)
        first += k
    return eng.fetch_pareto()


def write(out_dir, rows, index, scores):
    from eirgrid_amd.engine import Plan
    d = os.path.join(out_dir, "pareto")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "index.csv"), "w") as f:
        f.write("global_index,final_net_emissions,average_public_opinion,total_cost,power_reliability,rank_score\n")
        for r in range(len(index)):
            f.write(",".join([str(int(index[r]))] + ["%.17g" % x for x in rows.metrics[r]] + ["%.17g" % scores[r]]) + "\n")
    path = os.path.join(d, "plans.jsonl")
    if len(index):
        Plan.save(path, [Plan.from_result(rows, r, name=f"episode {int(index[r])}") for r in range(len(index))])
    else:
        open(path, "w").close()
    return d


def main():
    ap = argparse.ArgumentParser(description="The Pareto front of a training run: index.csv and plans.jsonl under DIR/pareto/")
    ap.add_argument("--world", required=True, help="a world JSON file (World.to_json_dict), or `synthetic`")
    ap.add_argument("-n", type=int, required=True, help="episodes to run")
    ap.add_argument("--batch", type=int, required=True, help="episodes per batch")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--cap", type=int, default=256, help="entries the archive holds at most, 1..256 (default 256)")
    ap.add_argument("--objectives", type=objectives, default=tuple(LETTERS.values()),
                    help="comma-separated subset of e,o,c,r: emissions, opinion, cost, reliability (default all four)")
    ap.add_argument("--cost-only", action="store_true", help="rank by the cost-only score when the front outgrows --cap")
    ap.add_argument("--keep", choices=("score", "spread"), default="score",
                    help="what stays when the front outgrows --cap: the best-scoring points, or a spread-out subset (default score)")
    ap.add_argument("--out", required=True, help="output directory")
    a = ap.parse_args()
    if a.n < 1 or a.batch < 1 or not 1 <= a.cap <= 256:
        ap.error("-n and --batch must be at least 1, --cap within 1..256")
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import Engine
    from eirgrid_amd.world import World
    world = synthetic_world() if a.world == "synthetic" else World.from_json_dict(json.load(open(a.world)))
    eng = Engine(world, device=0)
    try:
        rows, index, scores, dropped = run(eng, a.n, a.batch, a.seed, a.cap, a.objectives, a.cost_only, a.keep)
    finally:
        eng.close()
    d = write(a.out, rows, index, scores)
    print(f"{len(index)} non-dominated outcomes of {a.n} episodes over ({', '.join(a.objectives)}) -> {d}"
          + (f"; {dropped} dropped at cap {a.cap}: the archive is no longer the exact front" if dropped else ""))


if __name__ == "__main__":
    main()
