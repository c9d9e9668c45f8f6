"""What G generations of crossing a front cost end to end on the device (include/eirgrid_hip.h eg_breed_plans: the survivors' plan blocks
become the next parents in k_breed_gather / k_breed_turnover, one readback per generation) against the host loop that was the only way
before it: Engine.cross_front per generation (36 bytes per variant read back, the front filtered in numpy), every survivor built on the
host with PlanCross.apply and uploaded whole as the next generation's parents.

    python scripts/breed_probe.py [--front 16] [--generations 3] [--cuts 2030,2038,2045] [--reps 3]

The parents are the Pareto front of a short training run on tests/golden/world_v1.json (a few steps of 1 024 episodes with an archive of
--front entries).  Both forms run in one process on one build: a warm-up of each, then --reps INTERLEAVED repeats (device, host, device,
...), each the wall time of the whole call.  The host loop has no capacity rule: as long as no generation fills the cap of 256 (dropped = 0)
both forms must arrive at the same population, and the script checks that (same_population; null once something was dropped).  Reports
the medians, the spread and the ratio of the medians.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def summary(walls):
    return {"median_ms": float(np.median(walls)), "min_ms": float(min(walls)), "max_ms": float(max(walls)), "all_ms": [round(w, 3) for w in walls]}


def host_loop(eng, pol, parents, seed, cuts, generations):
    """the parent commit's way: cross_front a generation, the survivors rebuilt on the host; returns (population, variants evaluated)"""
    pop, total = list(parents), 0
    for _ in range(generations):
        front = eng.cross_front(pol, pop, seed, 0, cuts=cuts)
        total += front.n_variants
        if len(front.variant) == 0:
            break
        nxt = [x.apply(pop) for x in front.crosses]
        done = len(nxt) == len(pop) and bool(front.is_parent.all())
        pop = nxt
        if done:
            break
    return pop, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--front", type=int, default=16, help="entries of the training run's Pareto archive: the parents (at most)")
    ap.add_argument("--steps", type=int, default=4, help="training steps of 1 024 episodes")
    ap.add_argument("--generations", type=int, default=3)
    ap.add_argument("--cuts", default="2030,2038,2045")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    a = ap.parse_args()
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    from eirgrid_amd.world import World
    cuts = [int(y) - 2025 for y in a.cuts.split(",")]
    eng = Engine(World.from_json_dict(json.load(open(WORLD))), device=0)
    try:
        eng.push(ActionWeights())
        eng.track_pareto(a.front)
        for step in range(a.steps):
            eng.device_step(a.seed, 1024 * step, 1024, 10, a.seed + step)
        res, index = eng.fetch_pareto()[:2]
        parents = [Plan.from_result(res, e, f"episode {int(index[e])}") for e in range(len(index))]
        pol = ActionWeights()

        def device():
            return eng.breed_front(pol, parents, a.seed, 0, cuts=cuts, generations=a.generations, cap=256)

        def host():
            return host_loop(eng, pol, parents, a.seed, cuts, a.generations)
        front = device(); pop, total = host()      # warm-up: pools and buffers sized
        dropped = sum(g.n_dropped for g in front.generations)
        same = (front.plans == pop and sum(g.n_variants for g in front.generations) == total) if dropped == 0 else None
        walls = {"device": [], "host": []}
        for _ in range(a.reps):
            for form, call in (("device", device), ("host", host)):
                eng.sync()
                t0 = time.perf_counter()
                call()
                eng.sync()
                walls[form].append(1e3 * (time.perf_counter() - t0))
        out = {"parents": len(parents), "generations": [[g.n_parents, g.n_variants, g.n_kept] for g in front.generations], "stop": front.stop_reason,
               "variants": sum(g.n_variants for g in front.generations), "dropped": dropped, "same_population": same, "reps": a.reps, "device": summary(walls["device"]), "host": summary(walls["host"])}
        out["host_over_device"] = out["host"]["median_ms"] / out["device"]["median_ms"]
        print(json.dumps(out))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
