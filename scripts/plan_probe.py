"""What scoring N distinct plans costs (include/eirgrid_hip.h eg_evaluate_plans) against one replay batch of one list of the same length.

    python scripts/plan_probe.py [--episodes 16384] [--rounds 5]
    python scripts/plan_probe.py --rocprof DIR      # + the kernels' own times from one rocprofv3 --kernel-trace --stats run

Two sets of 16 384 distinct plans, each against its single-list baseline (eg_rollout_launch of 16 384 replay episodes, replay_mask all
ones, hoist off):
  short  the seeded policy's best list (configs[1]'s first episode, bench.py's seed) — the short-replay variant;
  long   the best list of the configs[2] grown state bench.py --full pins (~228 generators) — k_replay_solo + the long-replay variant.
Plan j is the base list with the cost multipliers of its first generator actions shifted by the base-3 digits of j: the same length
and generator types, distinct lists (the JSON counts them).  Rounds interleave baseline and plans; per call the wall time between two
synchronisations
(for the plans: building and uploading the plan blocks included) and the grids' time from the library's timing ring (for a plan batch
that one also counts the host's block building: its start event takes the end of the stream's previous command); medians over the
rounds.  With --rocprof, `kernel_trace` holds the same rounds as the kernels ran them (first to last rollout kernel of a call): the
numbers to compare kernels by.  Prints one JSON line."""
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


def setup(episodes, seed):
    from bench import GROW_BATCHES
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine
    from eirgrid_amd.parallel import BatchTrainer
    eng = Engine(synthetic_world(), device=0)
    w = ActionWeights()
    first = eng.run_iteration(0, w, False, seed)
    w.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0],
                    first.def_log[0, :first.n_def[0].sum()])
    seeded = ActionWeights()
    seeded.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0],
                         first.def_log[0, :first.n_def[0].sum()])
    eng.replay_hoist(True)
    grow = BatchTrainer(eng, w, episodes, seed, 0, 1, None, replay_fraction=0.1, device_resident=True)
    for _ in range(GROW_BATCHES):
        grow.step()
    grow.sync()
    eng.replay_hoist(False)
    grown = ActionWeights()
    eng.pull(grown)
    return eng, seeded, grown


def variants(base, n):
    """n plans of base's lengths and generator types, multipliers shifted by the base-3 digits of the plan index; (PlanSet, distinct lists)"""
    from eirgrid_amd.engine import Plan, PlanSet
    flat = [a for l in base.best_actions for a in l]
    gens = [i for i, a in enumerate(flat) if a < 45]
    sizes = [len(l) for l in base.best_actions]
    plans, seen = [], set()
    for j in range(n):
        f = list(flat)
        q = j
        for p in gens:      # the base-3 digits of j shift the multipliers of the first generator actions: j < 3^L lists are distinct
            if q == 0:
                break
            f[p] = 3 * (f[p] // 3) + (f[p] % 3 + q % 3) % 3
            q //= 3
        seen.add(tuple(f))
        run, k = [], 0
        for s in sizes:
            run.append(f[k:k + s]); k += s
        plans.append(Plan(run, base.best_deficit_actions))
    return PlanSet(plans), len(seen)


def timed(eng, fn):
    eng.sync()
    eng.timing_reset()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    wall = 1e3 * (time.perf_counter() - t0)
    total, n = eng.timing_read()
    return wall, total


def trace_spans(trace_csv, n_calls):
    """Per timed call, from the kernel trace: the span from the first to the last rollout kernel (k_rollout, k_replay_solo).  Every call
    (an upload + launch, or an evaluation) starts with k_stalled_tables; the last n_calls such segments are the trace run's calls."""
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    segs = []
    for r in rows:
        name = r["Kernel_Name"]
        if "k_stalled_tables" in name:
            segs.append([])
        elif segs and ("k_rollout" in name or "k_episodes" in name or "k_replay_solo" in name or "k_replay_lazy" in name):
            segs[-1].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    segs = [s for s in segs if s][-n_calls:]
    return [1e-6 * (max(e for _, e in s) - min(b for b, _ in s)) for s in segs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--rocprof", default=None, help="directory: also run this script's --trace mode under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--trace", action="store_true", help="(child of --rocprof) one round, untimed")
    a = ap.parse_args()
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import Plan
    eng, seeded, grown = setup(a.episodes, a.seed)
    n = a.episodes
    sets, n_distinct = {}, {}
    for name, pol in (("short", seeded), ("long", grown)):
        base = Plan.from_policy(pol)
        ps, distinct = variants(base, n)
        sets[name] = (pol, base, ps)
        n_distinct[name] = distinct
    ones = np.ones(n, np.uint8)
    opts = eng._opts(True, False, True)

    def baseline(pol):
        eng.upload_snapshot(pol)
        eng.launch(a.seed, 0, n, ones)

    def plans(pol, ps):
        snap = pol.snapshot()
        N.check(N.lib().eg_evaluate_plans(eng.h, C.byref(snap), C.byref(opts), C.byref(ps.s), C.c_uint64(a.seed), C.c_uint64(0), None),
                "eg_evaluate_plans")

    rounds = a.rounds
    res = {k: {"baseline_wall": [], "baseline_grids": [], "plans_wall": [], "plans_grids": []} for k in sets}
    for name, (pol, base, ps) in sets.items():      # warm-up: pools and buffers sized
        baseline(pol); plans(pol, ps); eng.sync()
    for _ in range(rounds):
        for name, (pol, base, ps) in sets.items():
            w, g = timed(eng, lambda: baseline(pol))
            res[name]["baseline_wall"].append(w); res[name]["baseline_grids"].append(g)
            w, g = timed(eng, lambda: plans(pol, ps))
            res[name]["plans_wall"].append(w); res[name]["plans_grids"].append(g)
    if a.trace:
        eng.close()
        return
    out = {"episodes": n, "rounds": rounds, "gpu": None}
    try:
        import torch
        out["gpu"] = torch.cuda.get_device_name(0)
    except Exception:      # (the probe does not need torch)
        pass
    # one check that the timed calls computed what they should: a plan batch of copies of the base list == the baseline's records
    for name, (pol, base, ps) in sets.items():
        med = {k: float(np.median(v)) for k, v in res[name].items()}
        rec = eng.evaluate_plans(pol, [base] * 64, a.seed, 0)
        ref = eng.rollout_batch(pol, a.seed, 64, 0, np.ones(64, np.uint8))
        same = bool(np.array_equal(rec.metrics, ref.metrics) and np.array_equal(rec.n_gens, ref.n_gens))
        out[name] = {"list_length": len(base), "distinct_plans": n_distinct[name], "generators": int(ref.n_gens[0]), "same_as_replay_batch": same,
                     "baseline_ms": med["baseline_grids"], "plans_ms": med["plans_grids"],
                     "overhead_pct": 100.0 * (med["plans_grids"] - med["baseline_grids"]) / med["baseline_grids"],
                     "plans_per_s": 1e3 * n / med["plans_grids"], "baseline_wall_ms": med["baseline_wall"], "plans_wall_ms": med["plans_wall"],
                     "plans_per_s_wall": 1e3 * n / med["plans_wall"], "all": res[name]}
    eng.close()
    if a.rocprof:
        from topk_probe import kernel_rows
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "plans", "--", sys.executable,
               os.path.abspath(__file__), "--trace", "--episodes", str(n), "--rounds", str(rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        stats = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True))
        out["rocprof_rc"] = p.returncode
        out["kernels"] = kernel_rows(stats[-1]) if stats else None
        if not stats:
            out["rocprof_tail"] = (p.stdout + p.stderr)[-2000:]
        traces = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_trace.csv"), recursive=True))
        if traces:      # calls in the order warm-up, rounds: (baseline, plans) x (short, long); the warm-up dropped
            spans = trace_spans(traces[-1], 4 * (1 + rounds))[4:]
            for i, name in enumerate(("short", "long")):
                b = float(np.median(spans[2 * i::4])); pl = float(np.median(spans[2 * i + 1::4]))
                out[name]["kernel_trace"] = {"baseline_ms": b, "plans_ms": pl, "overhead_pct": 100.0 * (pl - b) / b, "plans_per_s": 1e3 * n / pl,
                                             "baseline_all": spans[2 * i::4], "plans_all": spans[2 * i + 1::4]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
