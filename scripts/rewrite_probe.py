"""What scoring N rewrites of a plan costs end to end (include/eirgrid_hip.h eg_evaluate_plan_rewrites: the plans' blocks go up once, the maps
once and 8 bytes per variant, k_plan_rewrites writes the variants' plan blocks on the device) against the same children built on the
host and uploaded whole (eg_evaluate_plans, 8 832 bytes per child) — the only way to get these records without rewrites, so it is the
baseline.

    python scripts/rewrite_probe.py [--variants 512,16384] [--reps 5]

Two plans: `short`, the seeded policy's best list (28 actions): every child takes the short replay route; `long`, a script of nine
generators a year (about 270 actions): k_replay_solo and the long-replay variant, but for the children a rewrite makes short.  The
variants are the plan itself, the plan without each generator type it uses, at each cost tier, and with every second action dropped
from 2035 / 2040 on, repeated until there are N of them, variant j at global index j of the seed in both forms (same_index = 0), so that
both run the same episodes.  One process, one build: per plan and N a warm-up of both forms, then --reps INTERLEAVED repeats (rewrites,
plans, rewrites, ...), each the wall time between two synchronisations with nothing fetched, and the launches' own time between their
events (eg_timing_read); the host-built plan set is made before the clock starts.  Reports the medians, the spread (min .. max) and the
ratio of the medians, and checks that both forms returned the same metrics and statuses.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(walls):
    return {"median_ms": float(np.median(walls)), "min_ms": float(min(walls)), "max_ms": float(max(walls)), "all_ms": [round(w, 3) for w in walls]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="512,16384", help="comma-separated numbers of variants")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    a = ap.parse_args()
    sizes = [int(n) for n in a.variants.split(",")]
    from eirgrid_amd import _native as N
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionMap, ActionWeights, Engine, Plan, PlanRewrite, PlanSet, _map_array, _p, _rewrite_array, technology_rewrites
    from tests.test_refine import long_policy
    eng = Engine(synthetic_world(), device=0)
    seeded = ActionWeights()
    first = eng.run_iteration(0, seeded, False, a.seed)
    seeded.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0], first.def_log[0, :first.n_def[0].sum()])
    cases = (("short", seeded, Plan.from_policy(seeded)), ("long", long_policy(), Plan.from_policy(long_policy())))
    L = N.lib()
    opts = eng._opts(True, False, True)
    out = {"reps": a.reps, "seed": a.seed}
    for name, pol, plan in cases:
        snap = pol.snapshot()
        plan_set = PlanSet([plan])
        _, maps, kinds, _ = technology_rewrites([plan], "keep")
        maps = maps + [ActionMap.cost_tier(k) for k in range(3)] + [ActionMap.drop(range(1, 61, 2))]
        kinds = kinds + [PlanRewrite(0, len(maps) - 4 + k) for k in range(3)] + [PlanRewrite(0, len(maps) - 1, f, 26, 3) for f in (10, 15)]
        marr, n_maps = _map_array(maps)
        built = [rw.apply([plan], maps) for rw in kinds]
        out[name] = {"plan_length": len(plan), "kinds": len(kinds), "child_lengths": [len(c) for c in built]}
        for n in sizes:
            arr, k = _rewrite_array([kinds[j % len(kinds)] for j in range(n)])

            def by_rewrites():
                N.check(L.eg_evaluate_plan_rewrites(eng.h, C.byref(snap), C.byref(opts), C.byref(plan_set.s), marr, n_maps, arr, k, C.c_uint64(a.seed), C.c_uint64(0), 0,
                                                    None), "eg_evaluate_plan_rewrites")

            def results():
                metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32)
                o = N.EgEpisodeOut(metrics=_p(metrics, C.c_double), status=_p(status, C.c_int32))
                N.check(L.eg_fetch(eng.h, C.byref(o)), "eg_fetch")
                return metrics.tobytes(), status.tobytes()
            child_set = PlanSet([built[j % len(built)] for j in range(n)])

            def by_plans():
                N.check(L.eg_evaluate_plans(eng.h, C.byref(snap), C.byref(opts), C.byref(child_set.s), C.c_uint64(a.seed), C.c_uint64(0), None), "eg_evaluate_plans")
            by_rewrites(); eng.sync(); by_plans(); eng.sync()      # warm-up: pools and buffers sized
            walls = {"rewrites": [], "plans": []}
            device = {"rewrites": [], "plans": []}
            got = {}
            for _ in range(a.reps):
                for form, call in (("rewrites", by_rewrites), ("plans", by_plans)):
                    eng.sync()
                    eng.timing_reset()
                    t0 = time.perf_counter()
                    call()
                    eng.sync()
                    walls[form].append(1e3 * (time.perf_counter() - t0))
                    device[form].append(eng.timing_read()[0])
                    got[form] = results()
            row = {form: dict(summary(w), launches_ms=float(np.median(device[form]))) for form, w in walls.items()}
            row.update(same_results=bool(got["rewrites"] == got["plans"]), distinct_metric_rows=len({got["rewrites"][0][32 * j:32 * j + 32] for j in range(min(n, len(kinds)))}),
                       bytes_up={"rewrites": N.PLAN_BLOCK_BYTES + 64 * n_maps + 8 * n, "plans": N.PLAN_BLOCK_BYTES * n},
                       plans_over_rewrites=row["plans"]["median_ms"] / row["rewrites"]["median_ms"])
            out[name][str(n)] = row
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
