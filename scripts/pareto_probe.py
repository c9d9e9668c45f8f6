"""What the Pareto archive (include/eirgrid_hip.h eg_pareto_track) costs a configs[2] batch in the steady state bench.py pins, next to
the top-K archive as the yardstick, and its two worst cases.

    python scripts/pareto_probe.py [--rounds 5] [--batches 40]
    python scripts/pareto_probe.py --rocprof DIR      # + the kernels' own times from one rocprofv3 --kernel-trace --stats run

The policy is bench.py's headline state (scripts/topk_probe.py setup: seeded, grown, pinned by eg_policy_hold / eg_policy_rewind), 16 384
episodes per batch, every 10th a replay.  Three configurations in interleaved rounds of --batches batches each — no tracking, top-K 64,
Pareto cap 256 over all four objectives — per round the wall time per batch between two synchronisations, reported as the median over
the rounds.  Every round restarts its archive and runs two untimed batches first: the timed batches are the steady state.  Separately,
the two worst cases as wall time of one fold: the first batch of real episodes into an empty archive, and an antichain of 16 384 points
through eg_debug_pareto_fold (host copies of the synthetic records excluded: timed from a second fold of the same records into a
restarted archive, by HIP-synchronised wall clock around eg_pareto_fold_last_batch).  Prints one JSON line."""
import argparse
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

KERNELS = ("k_pareto_filter", "k_pareto_compact", "k_pareto_dominate", "k_pareto_rank", "k_pareto_finalize",
           "k_topk_keys", "k_topk_select", "k_topk_merge", "k_rollout", "k_episodes", "k_replay_solo", "k_replay_lazy", "k_apply_update")


def kernel_rows(stats_csv):
    import csv
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in KERNELS:
                if key in name:
                    agg = rows.setdefault(key, {"calls": 0, "total_ns": 0.0})
                    agg["calls"] += int(r.get("Calls", 0)); agg["total_ns"] += float(r.get("TotalDurationNs", 0.0))
    for v in rows.values():
        v["avg_us"] = v["total_ns"] / max(v["calls"], 1) / 1e3
    return rows


def set_mode(eng, mode):
    eng.track_top_k(64 if mode == "topk" else 0)
    eng.track_pareto(256 if mode == "pareto" else 0)


def one_fold_ms(eng):
    eng.sync()
    t0 = time.perf_counter()
    eng.fold_pareto_last_batch()
    eng.sync()
    return 1e3 * (time.perf_counter() - t0)


def main():
    from topk_probe import per_batch_ms, setup
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--rocprof", default=None, help="directory: also run this script's --trace mode under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--trace", action="store_true", help="(child of --rocprof) top-K and Pareto batches only, untimed")
    a = ap.parse_args()
    eng, tr = setup(a.episodes, a.seed)
    modes = ("off", "topk", "pareto")
    if a.trace:
        for mode in modes[1:]:
            set_mode(eng, mode)
            per_batch_ms(eng, tr, a.batches)
        eng.close()
        return
    out = {"episodes": a.episodes, "top_k": 64, "pareto_cap": 256, "objectives": 15, "rounds": a.rounds, "batches_per_round": a.batches}
    per_batch_ms(eng, tr, a.batches)      # warm-up (pools sized)
    ms = {m: [] for m in modes}
    for _ in range(a.rounds):
        for mode in modes:
            set_mode(eng, mode)
            per_batch_ms(eng, tr, 2)
            ms[mode].append(per_batch_ms(eng, tr, a.batches))
    for mode in modes:
        s = sorted(ms[mode])
        out[mode] = {"median_ms": s[len(s) // 2], "all_ms": ms[mode]}
    for mode in modes[1:]:
        out[mode]["overhead_pct"] = 100.0 * (out[mode]["median_ms"] - out["off"]["median_ms"]) / out["off"]["median_ms"]
    out["pareto"]["held"] = int(len(eng.fetch_pareto()[1]))
    # worst case 1: a batch of real episodes into an empty archive (the last batch of the loop above, folded again)
    set_mode(eng, "off"); per_batch_ms(eng, tr, 1)
    first = []
    for _ in range(5):
        eng.track_pareto(256)
        first.append(one_fold_ms(eng))
    out["first_batch_fold_ms"] = {"median": sorted(first)[2], "all": first, "held": int(len(eng.fetch_pareto()[1]))}
    # worst case 2: 16 384 mutually non-dominated points into an empty archive
    n = a.episodes
    r = np.random.default_rng(3).permutation(n).astype(np.float64)
    m = np.stack([1000.0 + 50.0 * r, np.full(n, 0.5), 1e9 * (n - r), np.ones(n)], axis=1)
    eng.track_pareto(256, ("emissions", "cost"))
    eng._debug_pareto_fold(m, np.zeros(n, np.int32), 0)
    anti = []
    for _ in range(5):
        eng.track_pareto(256, ("emissions", "cost"))
        anti.append(one_fold_ms(eng))
    held, dropped = eng.fetch_pareto()[1], eng.fetch_pareto()[3]
    out["antichain_fold_ms"] = {"median": sorted(anti)[2], "all": anti, "held": int(len(held)), "n_dropped": dropped}
    eng.close()
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "pareto", "--", sys.executable, os.path.abspath(__file__),
               "--trace", "--episodes", str(a.episodes), "--batches", str(a.batches)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        stats = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True))
        out["rocprof_rc"] = p.returncode
        out["kernels"] = kernel_rows(stats[-1]) if stats else None
        if not stats:
            out["rocprof_tail"] = (p.stdout + p.stderr)[-2000:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
