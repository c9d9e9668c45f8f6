"""What scoring N one-entry edits of a plan costs end to end (include/eirgrid_hip.h eg_evaluate_plan_edits: the plan blocks written on
the device by k_plan_edits) against the same variants written out as full plans on the host (eg_evaluate_plans).

    python scripts/plan_edit_probe.py [--episodes 16384] [--reps 3] [--modes edits,plans]
    EIRGRID_LIB=<a build of the parent commit> python scripts/plan_edit_probe.py --modes plans      # the host path as the parent ships it
    python scripts/plan_edit_probe.py --rocprof DIR      # + the kernels' own times from one rocprofv3 --kernel-trace --stats run

Two bases, as scripts/plan_probe.py: `short`, the seeded policy's best list (28 actions: the short-replay variant), and `long`, the best
list of the configs[2] grown state bench.py --full pins (k_replay_solo + the long-replay variant).  The variants are the base's one-entry
edits — every delete, every replace and every insert by each of the 61 actions, on both lists — repeated until there are --episodes of
them.  Per mode and base one warm-up call, then --reps timed calls: wall time between two synchronisations, nothing fetched.  A job
script alternates processes (this build, a build of the parent) for interleaved rounds; this script is one round.  Prints one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def all_edits(base, n):
    """(kind, list, year, pos, action) tuples: the base's one-entry edits in a fixed order, cycled to n"""
    out = [(0, 0, 0, 0, 0)]
    for which, lists in enumerate((base.best_actions, base.best_deficit_actions)):
        for y, l in enumerate(lists):
            out += [(1, which, y, i, 0) for i in range(len(l))]
            out += [(2, which, y, i, a) for i in range(len(l)) for a in range(61)]
            out += [(3, which, y, i, a) for i in range(len(l) + 1) for a in range(61)]
    return [out[j % len(out)] for j in range(n)]


def applied(base, e):
    from eirgrid_amd.engine import Plan
    kind, which, y, i, a = e
    lists = ([list(l) for l in base.best_actions], [list(l) for l in base.best_deficit_actions])
    l = lists[which][y]
    if kind == 1:
        del l[i]
    elif kind == 2:
        l[i] = a
    elif kind == 3:
        l.insert(i, a)
    return Plan(lists[0], lists[1])


def trace_calls(trace_csv):
    """Per call of the trace run (a call starts with k_stalled_tables): span first..last of its plan kernels, and k_plan_edits' own time"""
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    segs = []
    for r in rows:
        name = r["Kernel_Name"]
        if "k_stalled_tables" in name:
            segs.append({"spans": [], "edit_ms": 0.0})
        elif segs and any(k in name for k in ("k_rollout", "k_episodes", "k_replay_solo", "k_replay_lazy", "k_plan_edits")):
            b, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            segs[-1]["spans"].append((b, e))
            if "k_plan_edits" in name:
                segs[-1]["edit_ms"] += 1e-6 * (e - b)
    return [{"span_ms": 1e-6 * (max(e for _, e in s["spans"]) - min(b for b, _ in s["spans"])), "k_plan_edits_ms": s["edit_ms"]} for s in segs if s["spans"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--modes", default="edits,plans")
    ap.add_argument("--rocprof", default=None, help="directory: run this script's --trace mode under rocprofv3 --kernel-trace --stats instead")
    ap.add_argument("--trace", action="store_true", help="(child of --rocprof) untimed")
    a = ap.parse_args()
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "edits", "--", sys.executable,
               os.path.abspath(__file__), "--trace", "--episodes", str(a.episodes), "--reps", str(a.reps), "--modes", a.modes]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        out = {"rocprof_rc": p.returncode, "episodes": a.episodes, "reps": a.reps, "modes": a.modes}
        traces = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_trace.csv"), recursive=True))
        if traces:      # calls in the order (short, long) x modes x (warm-up, reps)
            calls = trace_calls(traces[-1])
            modes = a.modes.split(",")
            per = 1 + a.reps
            tail = calls[-2 * len(modes) * per:]
            for bi, base in enumerate(("short", "long")):
                for mi, mode in enumerate(modes):
                    seg = tail[(bi * len(modes) + mi) * per + 1:(bi * len(modes) + mi + 1) * per]
                    out.setdefault(base, {})[mode] = {"kernel_span_ms": float(np.median([s["span_ms"] for s in seg])),
                                                     "k_plan_edits_ms": float(np.median([s["k_plan_edits_ms"] for s in seg])), "all": seg}
        else:
            out["rocprof_tail"] = (p.stdout + p.stderr)[-2000:]
        print(json.dumps(out))
        return
    from plan_probe import setup
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import Plan, PlanSet, _edit_array
    eng, seeded, grown = setup(a.episodes, a.seed)
    n = a.episodes
    opts = eng._opts(True, False, True)
    L = N.lib()
    out = {"episodes": n, "reps": a.reps, "lib": os.environ.get("EIRGRID_LIB") or "shipped"}
    for name, pol in (("short", seeded), ("long", grown)):
        base = Plan.from_policy(pol)
        edits = all_edits(base, n)
        snap = pol.snapshot()
        out[name] = {"list_length": len(base), "deficit_length": sum(len(l) for l in base.best_deficit_actions)}
        for mode in a.modes.split(","):
            if mode == "edits":
                bs = PlanSet([base])
                arr, k = _edit_array(N.EgPlanEdit(*e) for e in edits)

                def call():
                    N.check(L.eg_evaluate_plan_edits(eng.h, C.byref(snap), C.byref(opts), C.byref(bs.s), arr, k, C.c_uint64(a.seed), C.c_uint64(0), 1, None),
                            "eg_evaluate_plan_edits")
            else:
                ps = PlanSet([applied(base, e) for e in edits])

                def call():
                    N.check(L.eg_evaluate_plans(eng.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.c_uint64(a.seed), C.c_uint64(0), None), "eg_evaluate_plans")
            call(); eng.sync()      # warm-up: pools and buffers sized
            walls = []
            for _ in range(a.reps):
                eng.sync()
                t0 = time.perf_counter()
                call()
                eng.sync()
                walls.append(1e3 * (time.perf_counter() - t0))
            out[name][mode] = {"wall_ms": float(np.median(walls)), "all": walls}
    eng.close()
    if not a.trace:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
