"""What scoring N one-cut children of two plans costs end to end (include/eirgrid_hip.h eg_evaluate_plan_crosses: the parents' blocks go up
once and 8 bytes per child, k_plan_crosses writes the children's plan blocks on the device) against the same children built on the host
and uploaded whole (eg_evaluate_plans, 8 832 bytes per child) — the only way to get these records without crosses, so it is the baseline.

    python scripts/cross_probe.py [--children 1024,16384] [--reps 5]
    python scripts/cross_probe.py --rocprof DIR      # k_plan_crosses' own time from one rocprofv3 --kernel-trace --stats run

Two pairs of parents: `short`, the seeded policy's best list (28 actions) and tests/test_refine.py's short script (67): every child takes
the short replay route; `long`, two scripts of nine generators a year (about 270 actions each): k_replay_solo and the long-replay variant.
The children are the 50 one-cut crossovers of the pair (cross_pairs(2) without the parents), repeated until there are N of them, child j
at global index j of the seed in both forms (same_index = 0), so that both run the same episodes.  One process, one build: per pair and N
a warm-up of both forms, then --reps INTERLEAVED repeats (crosses, plans, crosses, ...), each the wall time between two synchronisations
with nothing fetched; the host-built plan set is made before the clock starts.  Reports the medians, the spread (min .. max) and the
ratio of the medians, and checks that both forms returned the same
metrics and statuses.  Prints one JSON line."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(walls):
    return {"median_ms": float(np.median(walls)), "min_ms": float(min(walls)), "max_ms": float(max(walls)), "all_ms": [round(w, 3) for w in walls]}


def kernel_times(trace_csv):
    """the durations of the k_plan_crosses launches of a kernel trace, in launch order, in ms"""
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    return [1e-6 * (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows if "k_plan_crosses" in r["Kernel_Name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--children", default="1024,16384", help="comma-separated numbers of children")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--rocprof", default=None, help="directory: run this script's --trace mode under rocprofv3 --kernel-trace --stats instead")
    ap.add_argument("--trace", action="store_true", help="(child of --rocprof) the crosses alone, untimed")
    a = ap.parse_args()
    sizes = [int(n) for n in a.children.split(",")]
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "crosses", "--", sys.executable,
               os.path.abspath(__file__), "--trace", "--children", a.children, "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        out = {"rocprof_rc": p.returncode, "children": sizes, "reps": a.reps}
        traces = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_trace.csv"), recursive=True))
        if traces:      # launches in the order (short, long) x children x (warm-up, reps)
            ms = kernel_times(traces[-1])
            per = 1 + a.reps
            for pi, pair in enumerate(("short", "long")):
                for ni, n in enumerate(sizes):
                    seg = ms[(pi * len(sizes) + ni) * per + 1:(pi * len(sizes) + ni + 1) * per]
                    if seg:
                        out.setdefault(pair, {})[str(n)] = {"k_plan_crosses_ms": float(np.median(seg)), "all_ms": [round(v, 4) for v in seg]}
        else:
            out["rocprof_tail"] = (p.stdout + p.stderr)[-2000:]
        print(json.dumps(out))
        return
    from eirgrid_amd import _native as N
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan, PlanSet, _cross_array, _p, cross_pairs
    from tests.test_refine import _full_script, long_policy, short_policy
    eng = Engine(synthetic_world(), device=0)
    seeded = ActionWeights()
    first = eng.run_iteration(0, seeded, False, a.seed)
    seeded.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0], first.def_log[0, :first.n_def[0].sum()])
    other_long = _full_script(np.random.default_rng(6), 9, [0, 4, 12, 7, 5, 1, 13, 2], offsets_per_year=1)
    pairs = (("short", seeded, [Plan.from_policy(seeded), Plan.from_policy(short_policy())]),
             ("long", long_policy(), [Plan.from_policy(long_policy()), Plan.from_policy(other_long)]))
    L = N.lib()
    opts = eng._opts(True, False, True)
    out = {"reps": a.reps, "seed": a.seed}
    for name, pol, parents in pairs:
        snap = pol.snapshot()
        parent_set = PlanSet(parents)
        one_cut = cross_pairs(2)[2:]
        out[name] = {"parent_lengths": [len(p) for p in parents]}
        for n in sizes:
            crosses = [one_cut[j % len(one_cut)] for j in range(n)]
            arr, k = _cross_array(crosses)

            def by_crosses():
                N.check(L.eg_evaluate_plan_crosses(eng.h, C.byref(snap), C.byref(opts), C.byref(parent_set.s), arr, k, C.c_uint64(a.seed), C.c_uint64(0), 0, None),
                        "eg_evaluate_plan_crosses")

            def results():
                metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32)
                o = N.EgEpisodeOut(metrics=_p(metrics, C.c_double), status=_p(status, C.c_int32))
                N.check(L.eg_fetch(eng.h, C.byref(o)), "eg_fetch")
                return metrics.tobytes(), status.tobytes()
            if a.trace:
                for _ in range(1 + a.reps):
                    by_crosses(); eng.sync()
                continue
            built = [x.apply(parents) for x in one_cut]
            child_set = PlanSet([built[j % len(built)] for j in range(n)])

            def by_plans():
                N.check(L.eg_evaluate_plans(eng.h, C.byref(snap), C.byref(opts), C.byref(child_set.s), C.c_uint64(a.seed), C.c_uint64(0), None), "eg_evaluate_plans")
            by_crosses(); eng.sync(); by_plans(); eng.sync()      # warm-up: pools and buffers sized
            walls = {"crosses": [], "plans": []}
            got = {}
            for _ in range(a.reps):
                for form, call in (("crosses", by_crosses), ("plans", by_plans)):
                    eng.sync()
                    t0 = time.perf_counter()
                    call()
                    eng.sync()
                    walls[form].append(1e3 * (time.perf_counter() - t0))
                    got[form] = results()
            row = {form: summary(w) for form, w in walls.items()}
            row.update(same_results=bool(got["crosses"] == got["plans"]), distinct_metric_rows=len({got["crosses"][0][32 * j:32 * j + 32] for j in range(min(n, len(one_cut)))}),
                       bytes_up={"crosses": len(parents) * N.PLAN_BLOCK_BYTES + 8 * n, "plans": N.PLAN_BLOCK_BYTES * n},
                       plans_over_crosses=row["plans"]["median_ms"] / row["crosses"]["median_ms"])
            out[name][str(n)] = row
    eng.close()
    if not a.trace:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
