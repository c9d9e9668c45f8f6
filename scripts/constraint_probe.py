"""What judging plan constraints behind a plan batch costs end to end (include/eirgrid_hip.h eg_plan_constraints_set: one launch of
k_plan_constraints behind the batch's rollout grids, reading every record's 4 368 bytes of yearly rows) against the same batch without
constraints — the baseline.

    python scripts/constraint_probe.py [--variants 16384] [--reps 5]

One plan — the seeded policy's best list — and N edits of it (the round-0 variants of a refinement, repeated until there are N), every
variant at global index 0 of the seed, as a refinement round runs them.  One process, one build: a warm-up of every form, then --reps
INTERLEAVED repeats (0, 1, 32 constraints, 0, ...), each the wall time between two synchronisations with nothing fetched.  The
constraints are floors of -1e300 on four columns, every year or summed, over all 26 years (the longest fold): no variant violates one,
so the three forms leave the same statuses.  Reports the medians, the spread (min .. max) and the difference of the medians against the
baseline, and checks that all forms returned the same metrics and statuses.  Prints one JSON line."""
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
    ap.add_argument("--variants", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    a = ap.parse_args()
    from eirgrid_amd import _native as N
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.constraints import Constraint
    from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanSet, _edit_array, _p, refine_edits
    eng = Engine(synthetic_world(), device=0)
    pol = ActionWeights()
    first = eng.run_iteration(0, pol, False, a.seed)
    pol.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0], first.def_log[0, :first.n_def[0].sum()])
    plan = Plan.from_policy(pol)
    kinds = refine_edits(plan, replace_with=[12])
    n = a.variants
    arr, k = _edit_array([kinds[j % len(kinds)] for j in range(n)])
    L = N.lib()
    snap, opts, plan_set = pol.snapshot(), eng._opts(True, False, True), PlanSet([plan])
    loose = [Constraint(("balance", "gen", "net_co2", "total_cost")[i % 4], ">=", -1e300, aggregate="sum" if i & 1 else "every") for i in range(32)]
    forms = {"0": [], "1": loose[:1], "32": loose}

    def run():
        N.check(L.eg_evaluate_plan_edits(eng.h, C.byref(snap), C.byref(opts), C.byref(plan_set.s), arr, k, C.c_uint64(a.seed), C.c_uint64(0), 1, None), "eg_evaluate_plan_edits")

    def results():
        metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32)
        o = N.EgEpisodeOut(metrics=_p(metrics, C.c_double), status=_p(status, C.c_int32))
        N.check(L.eg_fetch(eng.h, C.byref(o)), "eg_fetch")
        return metrics.tobytes(), status.tobytes()
    for cs in forms.values():      # warm-up: pools and buffers sized
        eng.set_constraints(cs); run(); eng.sync()
    walls = {name: [] for name in forms}
    got = {}
    for _ in range(a.reps):
        for name, cs in forms.items():
            eng.set_constraints(cs)      # (the upload is not what is timed)
            eng.sync()
            t0 = time.perf_counter()
            run()
            eng.sync()
            walls[name].append(1e3 * (time.perf_counter() - t0))
            got[name] = results()
    eng.close()
    out = {"reps": a.reps, "seed": a.seed, "variants": n, "plan_length": len(plan), "kinds": len(kinds), "rows_bytes_read": n * 26 * 21 * 8}
    out.update({name: summary(w) for name, w in walls.items()})
    base = out["0"]["median_ms"]
    out.update(same_results=bool(got["0"] == got["1"] == got["32"]), added_ms={name: out[name]["median_ms"] - base for name in ("1", "32")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
