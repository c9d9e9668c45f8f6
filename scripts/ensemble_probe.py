"""What judging a plan batch over R draw streams costs end to end, two ways (include/eirgrid_hip.h eg_plan_streams_set):

  in-library   Engine.set_streams(R): one eg_evaluate_plan_edits call runs the R passes, k_ensemble_keep behind each and k_ensemble_commit
               behind the last; one fetch of the committed metrics and statuses
  host loop    R eg_evaluate_plan_edits calls at consecutive first indices, each with a fetch of metrics and statuses, then the reduction
               in numpy (reduce_numpy below: the order by a numpy score, the tail summed stream by stream) — the existing interface only

    python scripts/ensemble_probe.py [--variants 16384] [--reps 5]

Two plans: the seeded policy's best list (28 actions) and tests/test_refine.py's long policy (272 actions), each with N edits of it (the
round-0 variants of a refinement, repeated until there are N), every variant at global index 0 of the seed; R = 1, 4 and 16, the mean
outcome (tail = R: every stream is in the tail, so the two ways must agree bit for bit whatever the last bits of the host's score are).
One process, one build: a warm-up of every form, then --reps INTERLEAVED repeats, each behind 0.2 s of untimed batches (so that no form starts
on a device the previous form's host work left idle) and each the wall time from the call to the results on the host.  Reports per plan and R the medians, the spread (min .. max), the ratio to R = 1 and whether the two ways returned the same bytes.
Prints one JSON line."""
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


def numpy_score(m):
    """ai/metrics/scoring.rs:18-44 (mode None) over [..., 4] with numpy's logarithm: the order of the streams, to the last bits"""
    with np.errstate(all="ignore"):
        cost = np.maximum(m[..., 2] / 5e10, 1.0)
        cost_score = 1.0 - np.minimum(np.log(cost) / np.log(100.0), 1.0)
        w = np.where(cost > 8.0, 0.8, 0.5)
        return np.where(m[..., 0] > 0.0, 1.0 - np.minimum(m[..., 0] / 1e6, 1.0), 1.0 + (cost_score * w + m[..., 1] * (1.0 - w)))


def reduce_numpy(metrics, status, tail):
    """the reduction of include/eirgrid_hip.h over metrics [R, n, 4], status [R, n]: (committed metrics [n, 4], committed status [n])"""
    R, n = status.shape
    s = numpy_score(metrics)
    key = np.where(np.isnan(s), -np.inf, s)      # a NaN first, then the smaller score; a stable sort keeps the lower stream first
    rank = np.empty((R, n), np.int64)
    order = np.argsort(key, axis=0, kind="stable")
    np.put_along_axis(rank, order, np.arange(R)[:, None].repeat(n, 1), axis=0)
    selected = rank < tail
    committed = np.zeros((n, 4)); started = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for r in range(R):      # ascending stream order, one addition a stream
            add = selected[r]
            committed[add] = np.where(started[add, None], committed[add] + metrics[r, add], metrics[r, add])
            started |= add
        committed = committed / float(tail)
    bad = status != 0
    first_bad = np.argmax(bad, axis=0)
    return committed, np.where(bad.any(axis=0), status[first_bad, np.arange(n)], 0).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    a = ap.parse_args()
    from eirgrid_amd import _native as N
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanSet, _edit_array, _p, refine_edits
    from tests.test_refine import long_policy
    eng = Engine(synthetic_world(), device=0)
    L = N.lib()
    seeded = ActionWeights()
    first = eng.run_iteration(0, seeded, False, a.seed)
    seeded.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0], first.def_log[0, :first.n_def[0].sum()])
    n = a.variants
    out = {"reps": a.reps, "seed": a.seed, "variants": n}
    for pol in (seeded, long_policy()):
        plan = Plan.from_policy(pol)
        kinds = refine_edits(plan, replace_with=[12])
        arr, k = _edit_array([kinds[j % len(kinds)] for j in range(n)])
        snap, opts, plan_set = pol.snapshot(), eng._opts(True, False, True), PlanSet([plan])

        def batch(index):
            """one eg_evaluate_plan_edits call at `index`, then the fetch of metrics and statuses"""
            N.check(L.eg_evaluate_plan_edits(eng.h, C.byref(snap), C.byref(opts), C.byref(plan_set.s), arr, k, C.c_uint64(a.seed), C.c_uint64(index), 1, None), "eg_evaluate_plan_edits")
            metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32)
            o = N.EgEpisodeOut(metrics=_p(metrics, C.c_double), status=_p(status, C.c_int32))
            N.check(L.eg_fetch(eng.h, C.byref(o)), "eg_fetch")
            return metrics, status

        def in_library(R):
            eng.set_streams(R)      # (R = 1 clears: the batch as it always ran)
            return batch(0)

        def host_loop(R):
            eng.clear_streams()
            runs = [batch(r) for r in range(R)]
            return reduce_numpy(np.stack([m for m, _ in runs]), np.stack([s for _, s in runs]), R)
        forms = {(way.__name__, R): (way, R) for R in (1, 4, 16) for way in (in_library, host_loop)}
        for way, R in forms.values():      # warm-up: pools and buffers sized
            way(R)
        walls = {f: [] for f in forms}
        got = {}
        for _ in range(a.reps):
            for f, (way, R) in forms.items():
                eng.clear_streams()
                busy_until = time.perf_counter() + 0.2      # untimed batches first, 0.2 s of them: the host loop's numpy reduction leaves the device
                while time.perf_counter() < busy_until:     # idle, and the batches of the next 25 ms and more ran 4 to 20 ms slower
                    batch(0)
                eng.sync()
                t0 = time.perf_counter()
                res = way(R)
                walls[f].append(1e3 * (time.perf_counter() - t0))
                got[f] = (res[0].tobytes(), res[1].tobytes())
        here = {"plan_length": len(plan), "kinds": len(kinds)}
        for R in (1, 4, 16):
            lib, loop = summary(walls[("in_library", R)]), summary(walls[("host_loop", R)])
            here[f"R{R}"] = {"in_library": lib, "host_loop": loop, "same_results": got[("in_library", R)] == got[("host_loop", R)],
                             "in_library_over_R1": lib["median_ms"] / float(np.median(walls[("in_library", 1)])),
                             "host_loop_over_in_library": loop["median_ms"] / lib["median_ms"]}
        out[f"plan{len(plan)}"] = here
    eng.clear_streams()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
