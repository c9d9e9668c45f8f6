"""What a greedy refinement of a plan costs end to end: eg_refine_plan (include/eirgrid_hip.h; the winner picked and applied on the device)
against the loop a caller had to write before it — eg_evaluate_plan_edits per round, status and metrics fetched, scored and applied on
the host.

    python scripts/refine_probe.py [--rounds 4] [--reps 1] [--modes refine,loop]
    EIRGRID_LIB=<a build of the parent commit> python scripts/refine_probe.py --modes loop      # the loop as the parent ships it
    python scripts/refine_probe.py --rocprof DIR      # the kernels' own times from one rocprofv3 --kernel-trace --stats run

Two bases, the ones tests/test_refine.py pins with the tabled oracle: `short` (67 + 104 entries, replace_with=[12]: 239 variants a round)
and `long` (272 + 104 entries, deletes only: 377 variants), seed 1234, index 0, mode 1, both for the same --rounds (each improves for at
least four).  Per mode and base one warm-up call, then --reps timed calls: wall time of the whole refinement between two
synchronisations.  A job script alternates processes (this build, a build of the parent) for interleaved repeats and takes the medians;
this script is one repeat.  Prints one JSON line."""
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


def loop_refine(eng, pol, base, seed, rounds, replace_with):
    """the caller's loop over eg_evaluate_plan_edits: only status and metrics come back, as the CLI's --sensitivity asks for them"""
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import PlanSet, _edit_array, sensitivity_edits
    L = N.lib()
    snap = pol.snapshot()
    opts = eng._opts(True, False, True)
    plan, scores = base, []
    for _ in range(rounds):
        edits = sensitivity_edits(plan, replace_with)
        n = len(edits)
        ps = PlanSet([plan])
        arr, k = _edit_array(edits)
        metrics = np.zeros((n, 4)); status = np.zeros(n, np.int32)
        out = N.EgEpisodeOut()
        out.metrics = metrics.ctypes.data_as(C.POINTER(C.c_double)); out.status = status.ctypes.data_as(C.POINTER(C.c_int32))
        N.check(L.eg_evaluate_plan_edits(eng.h, C.byref(snap), C.byref(opts), C.byref(ps.s), arr, k, C.c_uint64(seed), C.c_uint64(0), 1, C.byref(out)),
                "eg_evaluate_plan_edits")
        score = np.array([L.eg_rank_score(metrics[j].ctypes.data_as(C.POINTER(C.c_double)), 1) if status[j] == 0 else -np.inf for j in range(n)])
        w = int(np.argmax(score))      # (the first of equal maxima)
        if w == 0:
            break
        scores.append(float(score[w]))
        plan = edits[w].apply(plan)
    return plan, scores


def kernel_stats(stats_csv):
    with open(stats_csv) as f:
        return {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": 1e-6 * float(r["TotalDurationNs"]), "mean_us": 1e-3 * float(r["AverageNs"])}
                for r in csv.DictReader(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--modes", default="refine,loop")
    ap.add_argument("--rocprof", default=None, help="directory: run this script's --trace mode under rocprofv3 --kernel-trace --stats instead")
    ap.add_argument("--trace", action="store_true", help="(child of --rocprof) untimed, refine mode only")
    a = ap.parse_args()
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "refine", "--", sys.executable,
               os.path.abspath(__file__), "--trace", "--rounds", str(a.rounds), "--reps", str(a.reps), "--modes", "refine"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        out = {"rocprof_rc": p.returncode, "rounds": a.rounds, "reps": a.reps}
        stats = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True))
        if stats:
            ks = kernel_stats(stats[-1])
            out["kernels"] = {k: v for k, v in ks.items() if any(s in k for s in ("k_refine_pick", "k_plan_edits", "k_rollout", "k_episodes", "k_replay_solo", "k_replay_lazy", "k_stalled_tables"))}
        else:
            out["rocprof_tail"] = (p.stdout + p.stderr)[-2000:]
        print(json.dumps(out))
        return
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import Engine, Plan
    from tests.test_refine import long_policy, short_policy
    eng = Engine(synthetic_world(), device=0)
    out = {"rounds": a.rounds, "reps": a.reps, "lib": os.environ.get("EIRGRID_LIB") or "shipped"}
    for name, pol, replace in (("short", short_policy(), [12]), ("long", long_policy(), None)):
        base = Plan.from_policy(pol)
        out[name] = {"list_length": len(base), "deficit_length": sum(len(l) for l in base.best_deficit_actions)}
        for mode in a.modes.split(","):
            if mode == "refine":
                def call():
                    plan, steps, stop, start, rec = eng.refine_plan(pol, base, a.seed, 0, 1, a.rounds, replace_with=replace)
                    return plan, [s.score for s in steps]
            else:
                def call():
                    return loop_refine(eng, pol, base, a.seed, a.rounds, replace)
            plan, scores = call(); eng.sync()      # warm-up: pools and buffers sized
            walls = []
            for _ in range(a.reps):
                eng.sync()
                t0 = time.perf_counter()
                call()
                eng.sync()
                walls.append(1e3 * (time.perf_counter() - t0))
            out[name][mode] = {"wall_ms": float(np.median(walls)), "all": walls, "steps": len(scores), "last_score": scores[-1] if scores else None,
                               "final_length": len(plan)}
    eng.close()
    if not a.trace:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
