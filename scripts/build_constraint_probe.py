"""What judging build constraints behind a plan batch costs end to end (include/eirgrid_hip.h eg_build_constraints_set: one launch of
k_build_constraints in place of k_plan_constraints, which walks every record's gen_pack / off_pack lists besides its yearly rows) against
the same batch without constraints, and against 32 row constraints — the parent's path, the yardstick.

    python scripts/build_constraint_probe.py [--variants 16384] [--reps 5]
    EIRGRID_LIB=/path/to/the/parent/libeirgrid_hip.so python scripts/build_constraint_probe.py      # the forms a parent build has

Two plans: the seeded policy's best list (28 actions) and tests/test_refine.py's long policy (272 actions: lists ten times longer), each
with N edits of it (the round-0 variants of a refinement, repeated until there are N), every variant at global index 0 of the seed.  One
process, one build: a warm-up of every form, then --reps INTERLEAVED repeats of the forms — no constraints, 32 row constraints, 1 build
constraint, 32 build constraints, 16 + 16 —, each the wall time between two synchronisations with nothing fetched.  Every constraint is a
floor of -1e300 over all 26 years (the longest fold; the build constraints weigh all 19 classes, every year or summed): no variant
violates one, so all forms leave the same statuses.  Reports per plan the medians, the spread (min .. max) and the difference of the
medians against the baseline, and checks that all forms returned the same metrics and statuses.  Prints one JSON line."""
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
    from eirgrid_amd.constraints import BuildConstraint, Constraint, constraint_array
    from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanSet, _edit_array, _p, refine_edits
    from tests.test_refine import long_policy
    eng = Engine(synthetic_world(), device=0)
    L = N.lib()
    have_builds = hasattr(L, "eg_build_constraints_set")      # (a parent build named by EIRGRID_LIB has the first two forms only)
    seeded = ActionWeights()
    first = eng.run_iteration(0, seeded, False, a.seed)
    seeded.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0], first.def_log[0, :first.n_def[0].sum()])
    rows = [Constraint(("balance", "gen", "net_co2", "total_cost")[i % 4], ">=", -1e300, aggregate="sum" if i & 1 else "every") for i in range(32)]
    builds = [BuildConstraint((1.0 + i,) * 19, ">=", -1e300, aggregate="sum" if i & 1 else "every") for i in range(32)]
    forms = {"none": [], "rows32": rows}
    if have_builds:
        forms.update({"build1": builds[:1], "build32": builds, "rows16+build16": rows[:16] + builds[:16]})

    def set_constraints(cs):
        if have_builds:
            eng.set_constraints(cs)
        else:
            arr, k = constraint_array(cs)
            N.check(L.eg_plan_constraints_set(eng.h, arr, k), "eg_plan_constraints_set")
    n = a.variants
    out = {"reps": a.reps, "seed": a.seed, "variants": n, "build_constraints": have_builds}
    for pol in (seeded, long_policy()):
        plan = Plan.from_policy(pol)
        kinds = refine_edits(plan, replace_with=[12])
        arr, k = _edit_array([kinds[j % len(kinds)] for j in range(n)])
        snap, opts, plan_set = pol.snapshot(), eng._opts(True, False, True), PlanSet([plan])

        def run():
            N.check(L.eg_evaluate_plan_edits(eng.h, C.byref(snap), C.byref(opts), C.byref(plan_set.s), arr, k, C.c_uint64(a.seed), C.c_uint64(0), 1, None), "eg_evaluate_plan_edits")

        def results():
            metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32); n_gens = np.zeros(n, np.int32); n_offsets = np.zeros(n, np.int32)
            o = N.EgEpisodeOut(metrics=_p(metrics, C.c_double), status=_p(status, C.c_int32), n_gens=_p(n_gens, C.c_int32), n_offsets=_p(n_offsets, C.c_int32))
            N.check(L.eg_fetch(eng.h, C.byref(o)), "eg_fetch")
            return metrics.tobytes(), status.tobytes(), int(n_gens.sum()), int(n_offsets.sum())
        for cs in forms.values():      # warm-up: pools and buffers sized
            set_constraints(cs); run(); eng.sync()
        walls = {name: [] for name in forms}
        got = {}
        for _ in range(a.reps):
            for name, cs in forms.items():
                set_constraints(cs)      # (the upload is not what is timed)
                eng.sync()
                t0 = time.perf_counter()
                run()
                eng.sync()
                walls[name].append(1e3 * (time.perf_counter() - t0))
                got[name] = results()
        here = {"plan_length": len(plan), "kinds": len(kinds), "list_entries_walked": got["none"][2] + got["none"][3]}
        here.update({name: summary(w) for name, w in walls.items()})
        base = here["none"]["median_ms"]
        here.update(same_results=bool(all(g[:2] == got["none"][:2] for g in got.values())),
                    added_ms={name: here[name]["median_ms"] - base for name in forms if name != "none"})
        out[f"plan{len(plan)}"] = here
    set_constraints([])
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
