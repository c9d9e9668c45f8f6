"""What the top-K archive (include/eirgrid_hip.h eg_top_k_track) costs a configs[2] batch in the steady state bench.py pins.

    python scripts/topk_probe.py [--k 10] [--rounds 7] [--batches 40]
    python scripts/topk_probe.py --rocprof DIR      # + the kernels' own times from one rocprofv3 --kernel-trace --stats run

The policy is bench.py's headline state (seeded, grown for GROW_BATCHES batches, pinned by eg_policy_hold / eg_policy_rewind), 16 384
episodes per batch, every 10th a replay.  Per-episode and hoisted replays, tracking off and on (k entries) in interleaved rounds of
--batches batches each; per round the wall time per batch between two synchronisations, reported as the median over the rounds.
Every round restarts its mode and runs two untimed batches first: the timed batches are the steady state (a full archive, the replays
of the best strategy entering every batch as one scenario).  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    eng.replay_hoist(True)
    grow = BatchTrainer(eng, w, episodes, seed, 0, 1, None, replay_fraction=0.1, device_resident=True)
    for _ in range(GROW_BATCHES):
        grow.step()
    grow.sync()
    eng.replay_hoist(False)
    tr = BatchTrainer(eng, w, episodes, seed, 0, 1, None, replay_fraction=0.1, device_resident=True)
    tr.pin_policy()
    return eng, tr


def per_batch_ms(eng, tr, batches):
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(batches):
        tr.step()
    eng.sync()
    return 1e3 * (time.perf_counter() - t0) / batches


def kernel_rows(stats_csv):
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            for key in ("k_topk_keys", "k_topk_select", "k_topk_merge", "k_rollout", "k_episodes", "k_replay_solo", "k_replay_lazy", "k_apply_update"):
                if key in name:
                    calls = int(r.get("Calls", 0))
                    total = float(r.get("TotalDurationNs", 0.0))
                    agg = rows.setdefault(key, {"calls": 0, "total_ns": 0.0})
                    agg["calls"] += calls; agg["total_ns"] += total
    for v in rows.values():
        v["avg_us"] = v["total_ns"] / max(v["calls"], 1) / 1e3
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--rocprof", default=None, help="directory: also run this script's --trace mode under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--trace", action="store_true", help="(child of --rocprof) tracked batches only, per-episode and hoisted, untimed")
    a = ap.parse_args()
    eng, tr = setup(a.episodes, a.seed)
    eng.track_top_k(a.k)
    if a.trace:
        for hoist in (False, True):
            eng.replay_hoist(hoist)
            per_batch_ms(eng, tr, a.batches)
        eng.close()
        return
    out = {"episodes": a.episodes, "k": a.k, "rounds": a.rounds, "batches_per_round": a.batches}
    for hoist in (False, True):
        eng.replay_hoist(hoist)
        per_batch_ms(eng, tr, a.batches)      # warm-up (archive filled, pools sized)
        off, on = [], []
        for _ in range(a.rounds):
            eng.track_top_k(0); per_batch_ms(eng, tr, 2); off.append(per_batch_ms(eng, tr, a.batches))
            # (a restarted archive is refilled by its first batch: untimed, like the two batches before every round)
            eng.track_top_k(a.k); per_batch_ms(eng, tr, 2); on.append(per_batch_ms(eng, tr, a.batches))
        off.sort(); on.sort()
        m_off, m_on = off[len(off) // 2], on[len(on) // 2]
        out["hoisted" if hoist else "per_episode"] = {"off_ms": m_off, "on_ms": m_on, "overhead_pct": 100.0 * (m_on - m_off) / m_off,
                                                      "off_all": off, "on_all": on}
    rows, scores, index = eng.fetch_top_k()
    out["held"] = int(len(index))
    eng.close()
    if a.rocprof:
        os.makedirs(a.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "topk", "--", sys.executable, os.path.abspath(__file__),
               "--trace", "--k", str(a.k), "--episodes", str(a.episodes), "--batches", str(a.batches)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        stats = sorted(glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True))
        out["rocprof_rc"] = p.returncode
        out["kernels"] = kernel_rows(stats[-1]) if stats else None
        if not stats:
            out["rocprof_tail"] = (p.stdout + p.stderr)[-2000:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
