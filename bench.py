#!/usr/bin/env python3
"""Headline benchmark: full 26-year episodes/s of the rollout hot path on N MI355X (BASELINE.json `metric`).

Workload (default, N = 1) = BASELINE configs[2] as SURVEY.md §8(d) defines it: 16 384 parallel 2025-2050 episodes per
batch, every 10th episode (by global index) replaying the best strategy ("experience replay": force_best_actions,
sampling.rs:78-145), the rest sampling from the policy; the best strategy the first batch meets is config 1's episode
(seed 12345, index 0).  With N > 1 every rank runs that batch size on its own shard of the global index range
(configs[3]: 8 x 16 384 = 131 072 episodes per update) and the update needs ONE collective.

A batch pass = the whole hot path with the policy resident on the device: k_rollout (the episodes + the batch-update
statistics in its epilogue), when N > 1 k_pick_best + ONE RCCL all-gather of every rank's 37 008-byte update packet, k_apply_update
(the batch form of the reference's write-locked update, multi_simulation.rs:494-508), k_stalled_tables — stream-ordered
launches, no host synchronisation, world tables and policy resident in HBM before the timed region starts.
A STEP = `batches_per_step` consecutive batch passes (--batches-per-step, 1 by default; 0 = calibrate it from untimed passes so
that the K timed steps last at least --min-seconds) — `steps`, `warmup` are the K, W of the command line, `ms_per_step` is per
step, `ms_per_batch` per pass.  With a fixed step the run is the same sequence of batches every time, so --dump-outputs DIR
writes the same outputs for the same arguments: the records of the last timed batch and the policy after its update, as .npy.

Reference semantics kept: a replay episode records and applies every action twice, so once a replay
episode becomes the best strategy the replayed lists — and the generators each replay episode places — double.  Left to
itself the loop therefore changes its own workload, and differently for every global batch size: from the seeded policy
(config 1's episode as the best strategy: 35 generators per replay episode) the single-GPU loop reaches a 257-action best
list — 228 generators per replay episode — after five wins and stays there; larger global batches go further (965 actions
at 131 072 episodes per update, profiles/r03a_replay_study_131072_fresh.json).
HEADLINE (since round 3) = the state the loop SUSTAINS, not the one it starts in: every batch starts from the policy the
single-GPU training loop holds GROW_BATCHES batches after the seeded one (every rank grows it alike, without exchange), put
back on the device before each batch by eg_policy_rewind (a device-to-device copy inside the timed region) so that the work
per GPU is the same at every N; the batch's update runs in full.  The seeded state — what rounds 1-2 reported as `value`:
2.5x faster, and gone after about five updates of a real run — is the line's `config2_seeded` object (`--seeded` makes it the
headline).  `--trajectory` lets the policy evolve instead (DESIGN.md §4 has those numbers).  The line reports what the
batches did: `config.replay` (generators per replay / seeded episode, best-list length), `config.policy` and
`config.episodes_failed` (EG_EP_OVERFLOW etc.; failed episodes are NOT counted in `value`).

A plain run measures the headline alone.  --full adds every other measurement, each in a timed region of its own after the
headline's: `config2_replay_hoisted`, `config2_seeded`, `config3_one_rank_state`, `fresh_policy_steady_state` and, at N > 1,
`sustained_at_n`; the N = 1 line also carries `config1` (BASELINE configs[1]: 1 024 episodes per batch, no replay), with a timed
region and a `roofline` of its own like `config2_seeded`, and `cpu_baseline`.  `roofline.traffic / hbm_frac_measured / valu_busy` come from
the committed counter profiles of the same command and are quoted only when that profile was taken on the very library
being timed (eg_build_hash); `frac_requested` bills only what the code requests from memory.

  python bench.py --gpus 1 --steps 20 --warmup 5 [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P bench.py --gpus 8 ...
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROW_AT_N = 30        # updates of the N-shard loop to its own sustained state (the list stops growing by update 8 at 131 072 per update)
GROW_BATCHES = 48     # free-running batches (single-GPU semantics) from the seeded policy to the grown-replay state
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md (≈6.3 TB/s achievable)
CUS, SIMDS_PER_CU = 256, 4


def host_cores() -> int:
    """Threads this process may really use: the cgroup CPU quota if there is one, else the affinity mask (capped at 64)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


def newest_profile(pattern: str, key: str, sub: str):
    """(value, file name, build hash) of the newest committed profiles/<pattern> that has an entry for `sub` under `key`."""
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern))):
        try:
            doc = json.load(open(path))
            cfg = doc[key].get(sub)
        except (OSError, ValueError, KeyError, AttributeError):
            continue
        if cfg:
            best = (cfg, os.path.basename(path), doc.get("build_hash"))
    return best


def library_hash() -> str:
    from eirgrid_amd import _native as N
    return N.lib().eg_build_hash().decode()


def stale(name: str, profile_hash) -> dict:
    """Counters cannot be collected from inside the process: they come from a committed profile of the same command.  A profile
    that was taken on another build of the library says nothing about the binary being timed: it is named, not quoted."""
    return {"stale": True, "profile": name,
            "reason": f"profiles/{name} was taken on build {profile_hash or 'unknown (no build_hash recorded)'}, the library being timed is "
                      f"{library_hash()}: counters not quoted (scripts/refresh_profiles.sh regenerates them)"}


def pmc_traffic(workload: str):
    """HBM bytes per k_rollout launch from the newest committed PMC profile of this workload (profiles/*pmc_hbm_traffic.json:
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes of this same command, gfx950 correction applied), with the
    kernel duration of those passes.  Counters cannot be collected from inside the process, so the numbers come from
    the committed profile of the same build; None when there is none."""
    hit = newest_profile("*pmc_hbm_traffic.json", "configs", workload)
    if not hit:
        return None
    cfg, name, built = hit
    if built != library_hash():
        return stale(name, built)
    if "kernel_ns" in cfg:
        dur = cfg["kernel_ns"] * 1e-9
    else:      # (profiles of round 1: one grid per launch)
        rows = cfg.get("fetch_rows") or []
        dur = sum(r["dur_ns"] for r in rows) / len(rows) * 1e-9 if rows else None
    return {"bytes": float(cfg["hbm_bytes_per_launch"]), "kernel_s": dur, "profile": name}


def sq_counters(workload: str):
    """VALU-busy share of the launch from the newest committed SQ counter profile of this workload
    (profiles/*sq_counters.json): SQ_ACTIVE_INST_VALU (quad-cycles summed over the SIMDs) x 4 / (SIMDs x launch cycles)."""
    hit = newest_profile("*sq_counters.json", "runs", workload)
    if not hit:
        return None
    run, name, built = hit
    if built != library_hash():
        return stale(name, built)
    try:
        clock_hz = float(run.get("clock_hz", 2.4e9))
        busy = run["SQ_ACTIVE_INST_VALU"] * 4.0 / (CUS * SIMDS_PER_CU * run["duration_ns"] * 1e-9 * clock_hz)
    except (KeyError, ZeroDivisionError):
        return None
    eps = max(run.get("episodes_per_launch", 1), 1)
    insts = sum(run.get(k, 0.0) for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_SMEM"))
    # an issue slot = a SIMD's turn in the CU's four-cycle round (one vector instruction per turn; scalar and LDS instructions of other
    # waves may go out beside it): all instructions over those turns — the figure a serial, latency-bound wave keeps low
    slots = CUS * SIMDS_PER_CU * run["duration_ns"] * 1e-9 * clock_hz / 4.0
    out = {"valu_busy": busy, "profile": name, "valu_insts_per_episode": run.get("SQ_INSTS_VALU", 0.0) / eps,
           "salu_insts_per_episode": run.get("SQ_INSTS_SALU", 0.0) / eps, "lds_insts_per_episode": run.get("SQ_INSTS_LDS", 0.0) / eps,
           "issue_slot_frac": insts / slots if slots > 0 else None}
    for v in ("heavy", "solo", "short", "lean", "coop"):      # a batch with replay episodes: the grids of the launch, measured one after the other
        if isinstance(run.get(v), dict) and "valu_busy" in run[v]:
            out[f"valu_busy_{v}_grid"] = run[v]["valu_busy"]
    return out


def cpu_baseline(world, seconds_budget: float = 20.0):
    """The CPU oracle (C restatement of the reference algorithm — NOT the Rust/rayon binary, which cannot be built here)
    timed on this box's host cores: literal mode (same work as the reference: 100x100 candidate search with sqrt+div per
    factor, G x S opinion loops) and tabled mode (same results from the host tables).  One episode per thread."""
    from concurrent.futures import ThreadPoolExecutor
    from eirgrid_amd.engine import HostTables
    from oracle import api as O
    O.build()
    cores = host_cores()
    ow = O.OracleWorld(world)
    t0 = time.perf_counter(); O.run_episode(ow, O.OracleWeights(), 1); one = time.perf_counter() - t0
    # about `seconds_budget` seconds of WALL time on every thread, never less than 5 s (round 3 ran 0.8 s: 15 s of CPU work spread over 16 threads)
    n_lit = max(cores, cores * int(math.ceil(max(seconds_budget * 0.5, 5.0) / max(one, 1e-3))))

    def lit(e):
        return O.run_episode(ow, O.OracleWeights(), 12345 + e)[0]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        st = list(ex.map(lit, range(n_lit)))
    t_lit = time.perf_counter() - t0
    assert all(s == 0 for s in st)
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    n_tab = 2000 * cores

    def tab(chunk):
        for e in chunk:
            O.run_episode_tabled(tb, O.OracleWeights(), 12345 + e)
    chunks = [range(i, n_tab, cores) for i in range(cores)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        list(ex.map(tab, chunks))
    t_tab = time.perf_counter() - t0
    return {"value": n_lit / t_lit, "unit": "episodes/s", "cores": cores, "kind": "port",
            "sample": f"{n_lit} literal-mode episodes (seeds 12345+e, fresh policy, same synthetic world), one per thread on {cores} threads, "
                      f"{t_lit:.1f} s wall; tabled mode: {n_tab} episodes in {t_tab:.1f} s",
            "tabled_value": n_tab / t_tab,
            "note": "C restatement of the reference algorithm (oracle/eg_oracle.c), not the Rust/rayon binary"}


def measured_peak():
    """Triad bandwidth measured on an MI355X of this pool (scripts/hbm_probe.py -> profiles/*hbm_probe.json), reported beside
    the datasheet peak that `frac` is priced against; None when no probe result is committed."""
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*hbm_probe.json"))):
        try:
            best = float(json.load(open(path))["triad_GBps"])
        except Exception:
            pass
    return best


def batch_census(res, first, period, had_best):
    """What the last batch did, from its records (`res` = eng.fetch() after the timed region): episodes by status, generators
    per seeded / replay episode, the two byte counts."""
    import numpy as np
    episodes = len(res.status)
    ok = res.status == 0
    idx = np.arange(first, first + episodes)
    rep = (idx % period == 0) if (period and had_best) else np.zeros(episodes, bool)
    mean = lambda a: float(a.mean()) if a.size else None
    return {"ok": int(ok.sum()), "overflow": int((res.status == -1).sum()), "other_failures": int((~ok & (res.status != -1)).sum()),
            "replay_episodes": int(rep.sum()),
            "generators_per_seeded_episode": mean(res.n_gens[ok & ~rep]), "generators_per_replay_episode": mean(res.n_gens[ok & rep]),
            "chunks_per_search": float(res.n_chunks[ok].sum()) / max(float(res.n_gens[ok].sum()), 1.0),
            "nominal_bytes": float(res.bytes_moved[ok].sum()), "touched_bytes": float(res.bytes_touched()[ok].sum()),
            "requested_bytes": float(res.bytes_requested()[ok].sum())}


DUMP_SEED = 20250101                                       # the fixed sample of episodes --dump-outputs writes in full
DUMP_EPISODES, DUMP_YEARLY, DUMP_LOGS = 16384, 2048, 256    # episodes sampled for the per-episode arrays / yearly rows / logs (<= 46 MB)


def dump_outputs(out_dir: str, res, w, first: int) -> dict:
    """What the timed path computed in its last step, as DIR/<name>.npy (float64; the logs float32, exact for their 8- and
    16-bit entries): the records of the last batch (`res`, global episode indices first..first+n) and the policy after its
    update (`w`, pulled from the device).  Batches larger than DUMP_EPISODES are sampled with a fixed seed, the yearly rows
    and the logs always are; log entries behind an episode's counts are written as 0.  Returns {name: bytes}."""
    import numpy as np
    n = len(res.status)
    rng = np.random.default_rng(DUMP_SEED)
    pick = lambda k: np.sort(rng.choice(n, size=min(n, k), replace=False))
    ep, ey, el = pick(DUMP_EPISODES), pick(DUMP_YEARLY), pick(DUMP_LOGS)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)

    def logs(log, counts):
        held = np.arange(log.shape[1])[None, :] < counts[:, None]
        return np.where(held, log, 0).astype(np.float32)
    arrays = {"episode_index": f64(first + ep), "metrics": f64(res.metrics[ep]), "status": f64(res.status[ep]),
              "n_run": f64(res.n_run[ep]), "n_def": f64(res.n_def[ep]), "n_act": f64(res.n_act[ep]),
              "n_gens": f64(res.n_gens[ep]), "n_offsets": f64(res.n_offsets[ep]), "n_draws": f64(res.n_draws[ep]),
              "n_chunks": f64(res.n_chunks[ep]), "bytes_moved": f64(res.bytes_moved[ep]),
              "yearly_episode_index": f64(first + ey), "yearly": f64(res.yearly[ey]),
              "log_episode_index": f64(first + el),
              "run_log": logs(res.run_log[el], res.n_run[el].sum(1)), "def_log": logs(res.def_log[el], res.n_def[el].sum(1)),
              "act_log": logs(res.act_log[el], res.n_act[el].sum(1)),
              "gen_cell": logs(res.gen_cell[el], res.n_gens[el]), "gen_pack": logs(res.gen_pack[el], res.n_gens[el]),
              "off_pack": logs(res.off_pack[el], res.n_offsets[el])}
    weights, deficit_weights, count_weights = w.tables()
    arrays.update({"policy_weights": f64(weights), "policy_deficit_weights": f64(deficit_weights),
                   "policy_count_weights": f64(count_weights),
                   "policy_best_list_lengths": f64([[len(l) for l in w.lists(which)] for which in (0, 1)]),
                   "policy_scalars": f64([w.get(k) for k in sorted(w.SC)])})
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: a.nbytes for name, a in arrays.items()}


def timed_loop(trainer, eng, fence, batches):
    """`batches` batch passes between two fences; returns (seconds, k_rollout HIP-event milliseconds, launches)."""
    eng.sync(); eng.timing_reset()
    fence()
    t0 = time.perf_counter()
    for _ in range(batches):
        trainer.step()
    fence()
    elapsed = time.perf_counter() - t0
    ms, grids_ms, n = eng.timing_read_grids()
    timed_loop.grids_ms = grids_ms      # (the grids' own durations added up: side-by-side grids show span < sum)
    return elapsed, ms, n


def roofline_object(workload, census, episodes, avg_kernel_s):
    """`achieved` = bytes the implemented algorithm touches per launch / measured kernel time (the SURVEY formula with the
    2601 x 8 B score field of every search replaced by the candidate records the branch-and-bound search requested);
    `nominal_*` = the SURVEY §8(d) formula as written (it bills the field, which this kernel never reads);
    `frac_requested` = only what the code requests from the memory system (BatchResult.bytes_requested: no state term — that
    state lives in LDS — and no generator coordinates) over the same time;
    `traffic` = HBM bytes per launch from the committed PMC profile of this workload — quoted only when that profile was
    taken on the very build being timed (eg_build_hash), null with the reason otherwise; `hbm_frac_measured` = that traffic
    over the kernel time of the same profiled launches over peak; `valu_busy` from the committed SQ counters.  `bound`
    says what the counters say: the kernel is bound by VALU issue / latency of its serial episode waves, not by HBM."""
    touched = census["touched_bytes"] * episodes / max(census["ok"], 1)
    nominal = census["nominal_bytes"] * episodes / max(census["ok"], 1)
    requested = census["requested_bytes"] * episodes / max(census["ok"], 1)
    achieved = touched / avg_kernel_s / 1e9 if avg_kernel_s > 0 else 0.0
    tr, sq = pmc_traffic(workload), sq_counters(workload)
    notes = [x["reason"] for x in (tr, sq) if x and x.get("stale")]
    if tr is None or sq is None:
        notes.append(f"no committed counter profile of workload '{workload}' (profiles/*_pmc_hbm_traffic.json, *_sq_counters.json)")
    tr_ok = tr if tr and not tr.get("stale") else None
    sq_ok = sq if sq and not sq.get("stale") else None
    # The primary ceiling comes first: VALU issue / the serial latency of episode waves.  `achieved` / `frac` / `frac_requested` /
    # `nominal_frac` are BYTE ACCOUNTING divided by time (the contract's keys) — not bandwidth and not a utilisation.
    obj = {"bound": "valu-issue / serial latency of episode waves — NOT HBM (read valu_busy and issue_slot_frac first, then hbm_frac_measured)",
           "valu_busy": sq_ok["valu_busy"] if sq_ok else None,
           "valu_busy_grids": {k[10:-5]: v for k, v in sq_ok.items() if k.startswith("valu_busy_") and k.endswith("_grid")} if sq_ok else None,
           "issue_slot_frac": sq_ok.get("issue_slot_frac") if sq_ok else None,
           "insts_per_episode": {"valu": sq_ok["valu_insts_per_episode"], "salu": sq_ok["salu_insts_per_episode"], "lds": sq_ok["lds_insts_per_episode"]} if sq_ok else None,
           # HBM bytes per batch (PMC, separate passes) over the span THIS run measured for the batch's rollout grids (the counter passes
           # serialise the grids of a batch: their own duration is longer and is not what those bytes were moved in)
           "hbm_frac_measured": (tr_ok["bytes"] / avg_kernel_s / 1e9 / HBM_PEAK_GBS) if tr_ok and avg_kernel_s > 0 else None,
           "traffic": tr_ok["bytes"] if tr_ok else None,
           "north_star_40pct_of_hbm": "not met and not a meaningful target on this path: an episode moves about 1 MB algorithmically (SURVEY finding 5, "
                                      "§8(d)), the tables are L2 / Infinity-Cache resident, measured HBM use is 2-13 % of peak; the kernels are bound by "
                                      "instruction issue on serial episode waves",
           "accounting": "achieved / frac / frac_requested / nominal_frac below = bytes by construction of the algorithm divided by kernel time: "
                         "frac bills the SURVEY §8(d) state terms (state that lives in LDS and never moves) plus the candidate records really requested; "
                         "frac_requested only what the code requests from the memory system; nominal_frac the SURVEY formula verbatim (it bills a "
                         "20.8 KB score field per search that the branch-and-bound search never reads, and can exceed 1); frac itself passes 1 once "
                         "the batch is fast enough — most of what it bills never leaves LDS — and says nothing about bandwidth: hbm_frac_measured does",
           "achieved": achieved, "peak": HBM_PEAK_GBS, "peak_measured": measured_peak(), "unit": "GB/s",
           "frac": achieved / HBM_PEAK_GBS,
           "frac_requested": requested / avg_kernel_s / 1e9 / HBM_PEAK_GBS if avg_kernel_s > 0 else 0.0,
           "kernel": "k_rollout", "avg_kernel_ms": avg_kernel_s * 1e3,
           "touched_bytes_per_launch": touched, "touched_bytes_per_episode": touched / max(episodes, 1),
           "requested_bytes_per_launch": requested, "requested_bytes_per_episode": requested / max(episodes, 1),
           "nominal_bytes_per_launch": nominal, "nominal_frac": nominal / avg_kernel_s / 1e9 / HBM_PEAK_GBS if avg_kernel_s > 0 else 0.0,
           "chunks_per_search": census["chunks_per_search"],
           "kernel_only_episodes_per_s": episodes / avg_kernel_s if avg_kernel_s > 0 else 0.0,
           "profiles": {"traffic": tr["profile"] if tr else None, "sq": sq["profile"] if sq else None, "library": library_hash()}}
    if notes:
        obj["counters_not_quoted"] = notes
    return obj


def policy_digest(w) -> str:
    """sha256 over the policy a rank holds after its last update (tables, best lists, counters): equal on every rank when the
    replicas are identical."""
    import hashlib
    import numpy as np
    h = hashlib.sha256()
    for t in w.tables():
        h.update(np.ascontiguousarray(t).tobytes())
    for which in (0, 1):
        h.update(repr(w.lists(which)).encode())
    for name in ("iterations_without_improvement", "iteration_count", "has_best", "best_net_emissions", "best_opinion", "best_cost", "best_reliability"):
        h.update(repr(float(w.get(name))).encode())
    return h.hexdigest()[:16]


def workload_key(episodes: int, replay_fraction: float) -> str:
    """Key of a workload in the committed profiles (profiles/*_pmc_hbm_traffic.json, *_sq_counters.json)."""
    return f"{episodes}" if replay_fraction == 0.0 else f"{episodes}r{replay_fraction:g}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=16384, help="episodes per GPU per batch (BASELINE configs[2]/[3]: 16384; configs[1]: 1024)")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--replay-fraction", type=float, default=0.1, help="configs[2]: 0.1 (every 10th global index replays the best strategy); configs[1]: 0")
    ap.add_argument("--min-seconds", type=float, default=0.5, help="with --batches-per-step 0: the K timed steps last at least this long "
                                                                   "(batches_per_step is sized for it)")
    ap.add_argument("--batches-per-step", type=int, default=None,
                    help="batch passes per timed step (default: 1 for the headline; the --full objects calibrate theirs); "
                         "0 = calibrate from untimed passes (then the step, and the batches the run makes, depend on the timing)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (the last batch's records, the policy after its "
                         "update) to DIR/<name>.npy; the same arguments give the same outputs")
    ap.add_argument("--full", action="store_true",
                    help="also every measurement beside the headline (the objects below, config1, cpu_baseline), each with a timed "
                         "region of its own; a plain run measures the headline alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-config1", action="store_true", help="with --full: skip the secondary objects (configs[1]: 1024 episodes, no replay; the grown-replay state)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only for rehearsal)")
    ap.add_argument("--share-gpu", action="store_true", help="rehearsal: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--force-collectives", action="store_true",
                    help="rehearsal: initialise torch.distributed and issue the per-update collectives even with one rank")
    ap.add_argument("--seeded", action="store_true",
                    help="headline = the seeded policy (SURVEY §8(d) config 3 read literally: a fresh policy whose best strategy is config 1's "
                         "episode, 35 generators per replay episode) instead of the state the training loop sustains; the N = 1 line carries "
                         "that measurement as its `config2_seeded` object anyway")
    ap.add_argument("--grown", action="store_true", help="(the default since round 3; kept for the scripts that pass it)")
    ap.add_argument("--trajectory", action="store_true",
                    help="let the policy evolve from batch to batch (the training loop as it runs) instead of starting every batch "
                         "from the seeded policy; what a replay episode costs then depends on the run and on N (SURVEY Q15)")
    ap.add_argument("--replay-hoist", action="store_true",
                    help="measure the HEADLINE with the replay hoist on (eg_replay_hoist: the batch's replay episodes computed once) — for profiling "
                         "that path; the default line executes every episode on its own and reports the hoisted batches as `config2_replay_hoisted`")
    ap.add_argument("--no-yearly", action="store_true", help="skip the 26x21 yearly rows (the reference always produces them)")
    args = ap.parse_args()
    # The headline is the SUSTAINED state of configs[2]: the policy the single-GPU training loop holds GROW_BATCHES batches after the
    # seeded one (its replayed list has stopped growing: 257 actions, 228 generators per replay episode).  The seeded policy itself
    # — 35 generators per replay episode — lasts about five updates of a real run; it is reported beside it (config2_seeded).
    args.grown = not args.seeded

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:   # convenience: relaunch under torchrun as a child process
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", "29511", os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    import numpy as np
    import torch
    import torch.distributed as dist
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine
    from eirgrid_amd.parallel import BatchTrainer
    from eirgrid_amd._native import PACKET_BYTES as N_PACKET_BYTES, STATS_LEN as N_STATS_LEN

    rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the rollout engine has no CPU path")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    use_dist = world_size > 1 or args.force_collectives
    # RCCL prints a version banner on stdout when its first communicator comes up (at the first collective).  stdout is
    # reserved for the one JSON line: until the warm-up is over, file descriptor 1 points at stderr.
    saved_stdout = None
    if use_dist:
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")      # only matters for --force-collectives outside torchrun
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world_size, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world_size)

    world = synthetic_world()
    eng = Engine(world, device=local_rank)
    def seeded_policy(grown: bool, fresh: bool = False, global_shards: int = 1, grow_batches: int = GROW_BATCHES):
        """a fresh ActionWeights::new whose best-action list is config 1's episode (seed 12345, global index
        0) — installed by the reference's own sequential update (multi_simulation.rs:494-508) of that one episode, on every rank
        alike.  grown: plus GROW_BATCHES batches of the training loop from there (every rank runs the same ones, no exchange): replay
        episodes win, and every win doubles the replayed list (Q15) until it stops growing.  fresh: no seeded best strategy — the
        loop finds its own (ActionWeights::new, what `cargo run -- -n N` starts from).  global_shards > 1: the loop at THAT many
        shards of `episodes` per update — every shard rolled out on this GPU into its own packet, one k_apply_update over all of
        them, no RCCL (the 8-shard loop of tests/test_gpu_rehearsals.py): the state an N-GPU run of the free-running loop reaches,
        which depends on the GLOBAL batch (core/simulation.rs:146-162, :406-409).  (Grown with the replay hoist on: the same
        policies, tests/test_gpu_replay_hoist.py, in a fraction of the time.)"""
        w = ActionWeights()
        if args.replay_fraction > 0.0:
            if not fresh:
                first = eng.run_iteration(0, w, False, args.seed)
                w.apply_episode(first.metrics[0], first.n_run[0], first.run_log[0, :first.n_run[0].sum()], first.n_def[0],
                                first.def_log[0, :first.n_def[0].sum()])
            if grown:
                eng.replay_hoist(True)
                if global_shards > 1:
                    eng.push(w, write_yearly=not args.no_yearly)
                    packets = torch.zeros(global_shards * N_PACKET_BYTES, dtype=torch.uint8, device=f"cuda:{local_rank}")
                    period = max(1, int(round(1.0 / args.replay_fraction)))
                    for step in range(grow_batches):
                        for r in range(global_shards):
                            eng.device_rollout(args.seed, (step * global_shards + r) * args.episodes, args.episodes, period,
                                               packets.data_ptr() + r * N_PACKET_BYTES)
                        eng.device_apply(packets.data_ptr(), global_shards, packets.data_ptr(), args.seed + step)
                        for r in range(1, global_shards):      # (every rank's own k_apply_update zeroes its own statistics)
                            packets[r * N_PACKET_BYTES:r * N_PACKET_BYTES + 8 * N_STATS_LEN] = 0
                    eng.pull(w)
                else:
                    grow = BatchTrainer(eng, w, args.episodes, args.seed, 0, 1, None, replay_fraction=args.replay_fraction,
                                        write_yearly=not args.no_yearly, device_resident=True)
                    for _ in range(grow_batches):
                        grow.step()
                    grow.sync()
                eng.replay_hoist(False)
        return w

    weights = seeded_policy(args.grown)
    trainer = BatchTrainer(eng, weights, args.episodes, args.seed, rank, world_size, dist if use_dist else None,
                           replay_fraction=args.replay_fraction, write_yearly=not args.no_yearly,
                           force_collectives=args.force_collectives, device_resident=True)
    if not args.trajectory:
        trainer.pin_policy()
    eng.replay_hoist(bool(args.replay_hoist))

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def all_max(x: float) -> float:
        if not use_dist:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=f"cuda:{local_rank}" if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def measure(tr, w, after_warmup=None, bps=None):
        """W warm-up steps, K timed steps of `bps` batch passes, then what the last batch did (`res`: its records, `w`: the policy
        after its update).  bps = 0: first a calibration (untimed for the result: the last 2 passes of 10 size `batches_per_step`);
        None: --batches-per-step, else calibrated (the --full objects)."""
        replay = {"best_list_len": int(sum(len(l) for l in w.lists(0))), "best_deficit_list_len": int(sum(len(l) for l in w.lists(1)))}      # (as pushed)
        if bps is None:
            bps = 0 if args.batches_per_step is None else args.batches_per_step
        calibration = 0
        if bps <= 0:
            for _ in range(8):
                tr.step()
            el, _, _ = timed_loop(tr, eng, fence, 2)
            calibration = 10
            bps = int(min(256, max(1, math.ceil(args.min_seconds / max(args.steps, 1) / max(all_max(el) / 2.0, 1e-6)))))
        for _ in range(args.warmup * bps):
            tr.step()
        if after_warmup:
            after_warmup()
        failed_before = tr.failed_episodes()
        elapsed, kernel_ms, n_launch = timed_loop(tr, eng, fence, args.steps * bps)
        elapsed = all_max(elapsed)
        failed = tr.failed_episodes() - failed_before      # episodes of ALL ranks that did not finish (counted by the updates)
        last_first = (tr.step_index - 1) * args.episodes * tr.ws + tr.rank * args.episodes
        res = eng.fetch(args.episodes)
        census = batch_census(res, last_first, tr.replay_period, True)      # (a best strategy exists from the first batch on)
        tr.sync()                     # device-resident policy -> host copy (after the timed region)
        batches = args.steps * bps
        return {"bps": bps, "calibration": calibration, "elapsed": elapsed, "batches": batches, "failed": failed, "census": census,
                "res": res, "last_first": last_first,
                "avg_kernel_s": kernel_ms / max(n_launch, 1) * 1e-3, "avg_grids_s": timed_loop.grids_ms / max(n_launch, 1) * 1e-3, "value": (args.episodes * tr.ws * batches - failed) / elapsed,
                "replay": replay}

    def policy_text(grown: bool) -> str:
        if args.trajectory:
            return "free-running: every batch builds on the update of the one before (--trajectory)"
        start = (f"the policy the single-GPU training loop holds {GROW_BATCHES} batches after the seeded one (replay episodes have won and "
                 "doubled the replayed list, SURVEY Q15)") if grown else \
                "the seeded policy (ActionWeights::new + config 1's episode as the best strategy, SURVEY §8(d) config 3)"
        return (f"pinned: every batch starts from {start}, put back by eg_policy_rewind (a device-to-device copy inside the timed region); "
                "the batch's update runs in full and is not carried into the next batch — the same work per batch on any number of GPUs")

    def restore_stdout():
        nonlocal saved_stdout
        if saved_stdout is not None:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1); os.close(saved_stdout)
            saved_stdout = None

    m = measure(trainer, weights, restore_stdout, bps=1 if args.batches_per_step is None else args.batches_per_step)
    res = m.pop("res")
    if args.dump_outputs and rank == 0:      # (before anything else runs on this engine: the records are the last timed batch's)
        dump_outputs(args.dump_outputs, res, weights, m["last_first"])
    del res
    digests = [policy_digest(weights)]      # (measure() ends with the policy pulled from the device)
    if use_dist:
        digests = [None] * world_size
        dist.all_gather_object(digests, policy_digest(weights))
    eng.replay_hoist(False)
    wkey = workload_key(args.episodes, args.replay_fraction) + ("grown" if args.grown and args.replay_fraction > 0.0 else "") \
        + ("hoist" if args.replay_hoist else "") + ("traj" if args.trajectory else "")

    line = None
    if rank == 0:
        census = m["census"]
        cfg_name = ("BASELINE configs[2]" if world_size == 1 else f"BASELINE configs[3] at {world_size} GPUs") \
            if (args.episodes == 16384 and abs(args.replay_fraction - 0.1) < 1e-12) else \
            ("BASELINE configs[1]" if (args.episodes == 1024 and args.replay_fraction == 0.0 and world_size == 1) else "custom")
        line = {
            "metric": "26-year episodes/sec", "value": m["value"], "unit": "episodes/s",
            "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup, "ms_per_step": m["elapsed"] / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "batches_per_step": m["bps"], "ms_per_batch": m["elapsed"] / m["batches"] * 1e3, "timed_region_s": m["elapsed"],
            "calibration_batches": m["calibration"],
            "config": {"workload": f"{cfg_name}: {args.episodes} parallel 2025-2050 episodes per GPU per batch"
                                   + (f", every {trainer.replay_period}th global index replaying the best strategy (experience replay, reference "
                                      "semantics incl. its double recording, SURVEY Q15)" if trainer.replay_period else ", no replay")
                                   + "; batch pass = rollout (grid step + tabular policy sampling) + batch policy update on the device; synthetic world "
                                     "S=130 settlements / G0=59 existing plant / P=200 coast points, seed 12345",
                       "episodes_per_gpu_per_batch": args.episodes, "replay_fraction": args.replay_fraction, "replay_hoist": bool(args.replay_hoist),
                       # which kernel runs a long replay episode when every episode is executed on its own (csrc/eg_replay_solo.h)
                       "per_episode_replay_kernel": ("k_rollout<0,2> (EIRGRID_REPLAY_SOLO=0: year by year, action by action)" if os.environ.get("EIRGRID_REPLAY_SOLO", "1")[:1] == "0"
                                                     else "k_replay_solo (each replay episode's script, placements and yearly rows on its own wave; k_rollout<0,2> behind it for "
                                                          "scripts that need a seeded draw)"),
                       "batches_timed": m["batches"], "episodes_failed": m["failed"],
                       "parallelism": f"episode-sharded dp{world_size}, policy resident on every GPU, one all-gather of {N_PACKET_BYTES} bytes per rank per update "
                                      "(integer statistics summed in the update kernel)",
                       "last_batch": {k: census[k] for k in ("ok", "overflow", "other_failures", "replay_episodes",
                                                             "generators_per_seeded_episode", "generators_per_replay_episode")},
                       "policy": policy_text(args.grown),
                       "replica_digests": digests,      # the policy every rank holds after the last update: one value when the replicas are identical
                       "replay": m["replay"],
                       **({"strategy_improvements": trainer.improvements,
                           "iterations_without_improvement": int(weights.get("iterations_without_improvement"))} if args.trajectory else {})},
            "roofline": roofline_object(wkey, census, args.episodes, m["avg_kernel_s"]),
        }
        # the grids of a batch (replay variants on the side stream, the rest on the null stream), from the library's own events
        line["roofline"]["grids"] = {"span_ms": m["avg_kernel_s"] * 1e3, "sum_of_grids_ms": m["avg_grids_s"] * 1e3,
                                     "overlap": 1.0 - m["avg_kernel_s"] / m["avg_grids_s"] if m["avg_grids_s"] > 0 else 0.0}
    # ---- the same batches with the replay hoist on (include/eirgrid_hip.h eg_replay_hoist): the replay episodes of a batch — one and
    #      the same computation — computed once, every record / packet / policy byte-identical (tests/test_gpu_replay_hoist.py).
    #      `value` above executes every episode on its own, as before; this object is the same workload with that redundancy removed. ----
    def side_object(w, hoist: bool, what: str, profile_key: str = None):
        """One more pinned measurement of `w` on this engine (all ranks take part: the same collectives as the headline)."""
        tr = BatchTrainer(eng, w, args.episodes, args.seed, rank, world_size, dist if use_dist else None, replay_fraction=args.replay_fraction,
                          write_yearly=not args.no_yearly, force_collectives=args.force_collectives, device_resident=True)
        tr.pin_policy()
        eng.replay_hoist(hoist)
        g = measure(tr, w)
        served = eng.replay_hoist_stats()[1] if hoist else None
        eng.replay_hoist(False)
        obj = {"workload": what, "replay_hoist": hoist, "hoist_served_last_batch": served,
               "value": g["value"], "unit": "episodes/s", "batches_timed": g["batches"], "timed_region_s": g["elapsed"],
               "ms_per_batch": g["elapsed"] / g["batches"] * 1e3, "episodes_failed": g["failed"],
               "rollout_span_ms": g["avg_kernel_s"] * 1e3, "sum_of_grids_ms": g["avg_grids_s"] * 1e3,
               "last_batch": {k: g["census"][k] for k in ("ok", "overflow", "other_failures", "replay_episodes",
                                                          "generators_per_seeded_episode", "generators_per_replay_episode")},
               "replay": g["replay"]}
        if profile_key and rank == 0:
            obj["roofline"] = roofline_object(profile_key, g["census"], args.episodes, g["avg_kernel_s"])
        return obj

    extras = args.full and args.replay_fraction > 0.0 and not args.trajectory and not args.no_config1
    hoisted = side_object(seeded_policy(args.grown), True,
                          "the headline's batches (same pinned policy, same episodes, same update) with the replay hoist on: the batch's replay "
                          "episodes are computed once by a cooperative workgroup and handed to every replay slot",
                          workload_key(args.episodes, args.replay_fraction) + ("grown" if args.grown else "") + "hoist") if extras else None
    sustained_n = None
    if extras and world_size > 1:
        # What the N-GPU loop itself sustains: the reference's replayed list grows with the GLOBAL batch (Q15), so the state an N-rank run
        # settles in is not the single-GPU one the headline pins.  Every rank grows that state alike (the N shards of every update on its
        # own GPU, no exchange), then the batches are timed with the real exchange in the loop — per-episode replays and hoisted.
        wn = seeded_policy(True, global_shards=world_size, grow_batches=GROW_AT_N)
        a = side_object(wn, False, f"pinned at the state the {world_size}-rank loop reaches after {GROW_AT_N} updates of {world_size} x {args.episodes} episodes")
        wn = seeded_policy(True, global_shards=world_size, grow_batches=GROW_AT_N)
        b = side_object(wn, True, "the same with the replay hoist on")
        sustained_n = {"what": f"the state the FREE-RUNNING loop reaches at this N (global batch {world_size} x {args.episodes}): `value` pins the single-GPU "
                               "state on every rank so that the per-N values compare the exchange alone; this object is the N-rank loop's own state",
                       "per_episode_replays": a, "replay_hoisted": b}
    if rank == 0 and hoisted is not None:
        line["config2_replay_hoisted"] = hoisted
        line["config2_replay_hoisted"]["speedup_vs_value"] = hoisted["value"] / m["value"] if m["value"] > 0 else None
        if sustained_n is not None:
            line["sustained_at_n"] = sustained_n
    if extras and world_size == 1:
        # one rank's batch in the state of the 8-GPU loop (configs[3]: 131 072 episodes per update), measured on this one GPU without the exchange
        w8 = seeded_policy(True, global_shards=8, grow_batches=GROW_AT_N)
        a = side_object(w8, False, f"ONE rank's batch (16 384 episodes, no exchange) in the state the 8-GPU loop of configs[3] reaches after {GROW_AT_N} updates of 131 072 episodes")
        w8 = seeded_policy(True, global_shards=8, grow_batches=GROW_AT_N)
        b = side_object(w8, True, "the same with the replay hoist on")
        line["config3_one_rank_state"] = {"per_episode_replays": a, "replay_hoisted": b,
                                          "implied_8gpu_aggregate_episodes_per_s": {"per_episode_replays": 8 * a["value"], "replay_hoisted": 8 * b["value"]},
                                          "note": "aggregate = 8 x one rank's rate, without the update's all-gather (measured at +18 us per update with one rank, DESIGN §5); no 8-GPU node was measured"}
        # the single-GPU loop from a FRESH policy (no seeded best strategy): where `cargo run -- -n N` would settle
        wf = seeded_policy(True, fresh=True)
        a = side_object(wf, False, f"pinned at the state the single-GPU loop reaches {GROW_BATCHES} batches after ActionWeights::new (no seeded best strategy)")
        wf = seeded_policy(True, fresh=True)
        b = side_object(wf, True, "the same with the replay hoist on")
        line["fresh_policy_steady_state"] = {"per_episode_replays": a, "replay_hoisted": b}
    # ---- second object (N = 1): the grown-replay state of the same workload — what the training loop turns configs[2] into ----
    if args.full and world_size == 1 and not args.no_config1 and args.replay_fraction > 0.0 and not args.trajectory:
        other_grown = not args.grown      # the state the headline was NOT measured in
        wg = seeded_policy(other_grown)
        tg = BatchTrainer(eng, wg, args.episodes, args.seed, 0, 1, None, replay_fraction=args.replay_fraction,
                          write_yearly=not args.no_yearly, device_resident=True)
        tg.pin_policy()
        g = measure(tg, wg)
        line["config2_grown" if other_grown else "config2_seeded"] = {
                                 "workload": ("the same batches from the grown-replay state: " if other_grown else
                                              "the same batches from the seeded policy, as SURVEY §8(d) words config 3 (a state the free-running loop "
                                              "leaves within about five updates): ") + policy_text(other_grown),
                                 "value": g["value"], "unit": "episodes/s", "batches_timed": g["batches"], "timed_region_s": g["elapsed"],
                                 "ms_per_batch": g["elapsed"] / g["batches"] * 1e3, "episodes_failed": g["failed"],
                                 "last_batch": {k: g["census"][k] for k in ("ok", "overflow", "other_failures", "replay_episodes",
                                                                            "generators_per_seeded_episode", "generators_per_replay_episode")},
                                 "replay": g["replay"],
                                 "roofline": roofline_object(workload_key(args.episodes, args.replay_fraction) + ("grown" if other_grown else ""), g["census"],
                                                             args.episodes, g["avg_kernel_s"])}
    # ---- second object: BASELINE configs[1] (1024 episodes per batch, no replay), its own policy and timed region ----
    if args.full and world_size == 1 and not args.no_config1 and not (args.episodes == 1024 and args.replay_fraction == 0.0):
        w1 = ActionWeights()
        t1 = BatchTrainer(eng, w1, 1024, args.seed, 0, 1, None, replay_fraction=0.0, write_yearly=not args.no_yearly, device_resident=True)
        if not args.trajectory:
            t1.pin_policy()
        for _ in range(8):
            t1.step()
        el, _, _ = timed_loop(t1, eng, fence, 8)
        n1 = int(max(20, math.ceil(args.min_seconds / max(el / 8.0, 1e-6))))
        f0 = t1.failed_episodes()
        el, kms, nl = timed_loop(t1, eng, fence, n1)
        f1 = t1.failed_episodes() - f0
        c1 = batch_census(eng.fetch(1024), (t1.step_index - 1) * 1024, 0, True)
        t1.sync()
        line["config1"] = {"workload": "BASELINE configs[1]: 1024 parallel episodes per batch, no replay; batch pass = rollout + batch policy update; "
                                       + ("free-running policy" if args.trajectory else "every batch from ActionWeights::new (pinned like the headline)"),
                           "value": (1024 * n1 - f1) / el, "unit": "episodes/s", "batches_timed": n1, "timed_region_s": el,
                           "ms_per_batch": el / n1 * 1e3, "episodes_failed": f1,
                           "roofline": roofline_object(workload_key(1024, 0.0), c1, 1024, kms / max(nl, 1) * 1e-3)}
    if rank == 0:
        if args.full and world_size == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(world)
        print(json.dumps(line), flush=True)
    eng.close()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
