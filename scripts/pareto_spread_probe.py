"""What the Pareto archive's capacity rule "keep spread" (include/eirgrid_hip.h EG_PARETO_KEEP_SPREAD; csrc/eg_pareto.h k_pareto_spread)
costs next to "keep score" (k_pareto_rank), and what it buys.

    python scripts/pareto_spread_probe.py [--reps 21] [--breed-reps 5]

Everything is crafted or sampled here from seeds on the synthetic world; both rules are timed in alternation in one process, each figure
the median of --reps wall times between two synchronisations, after one untimed pass of every case.
  steady   one overflowing fold in the steady state: an archive holding cap = 256 points of a line, then a batch of 16 384 records of
           which 50 lie on the same line between the held ones and the rest are dominated by a held point — a front of cap + 50.  The
           batch is loaded first (eg_debug_load_batch); the time is eg_pareto_fold_last_batch's alone.
  worst    one fold of a whole batch of 16 384 mutually non-dominated points into an empty archive, 16 384 -> 256.
  breed    Engine.breed_front from 8 sampled plans, cap 8, 4 generations of 1 408 variants in chunks of 256: a run whose folds overflow.
  quality  the covering radius of what each rule kept in `steady` and `worst`: the largest distance, in the front's normalised
           coordinates, from a point of the front to its nearest kept point.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RULES = ("score", "spread")
LINE = ("emissions", "cost")


def line(r, n):
    """Points r of a line of n under (emissions, cost): emissions rise and cost falls with r — none dominates another."""
    r = np.asarray(r, np.float64)
    return np.stack([1000.0 + 50.0 * r, np.full(len(r), 0.5), 1e9 * (n - r), np.ones(len(r))], axis=1)


def covering_radius(front, kept):
    """Both [.., 4] metrics of a front under (emissions, cost); distances in the front's normalised coordinates."""
    lo, hi = front[:, [0, 2]].min(0), front[:, [0, 2]].max(0)
    u, k = (front[:, [0, 2]] - lo) / (hi - lo), (kept[:, [0, 2]] - lo) / (hi - lo)
    worst = 0.0
    for a in range(0, len(u), 2048):
        d = ((u[a:a + 2048, None, :] - k[None, :, :]) ** 2).sum(2).min(1)
        worst = max(worst, float(d.max()))
    return worst ** 0.5


def fold_ms(eng):
    eng.sync()
    t0 = time.perf_counter()
    eng.fold_pareto_last_batch()
    eng.sync()
    return 1e3 * (time.perf_counter() - t0)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Plan
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--breed-reps", type=int, default=5)
    a = ap.parse_args()
    eng = Engine(synthetic_world(), device=0)
    out = {"cap": 256, "batch": 16384, "reps": a.reps}
    n, cap, extra = 16384, 256, 50
    ok = np.zeros(n, np.int32)

    # steady: 306 points of a line; 50 of them arrive in the batch, among 16 334 records a held point dominates
    rng = np.random.default_rng(11)
    pos = 40.0 * np.arange(cap + extra)
    late = np.sort(rng.choice(cap + extra, extra, replace=False))
    held = np.setdiff1d(np.arange(cap + extra), late)
    front = line(pos, 40 * (cap + extra))
    filler = front[held][rng.integers(0, cap, n - extra)] + np.array([1.0, 0.0, 1e6, 0.0])
    batch = np.concatenate([front[late], filler])[rng.permutation(n)]

    def steady(rule):
        eng.track_pareto(cap, LINE, keep=rule)
        eng._debug_pareto_fold(front[held], np.zeros(cap, np.int32), 0)
        eng._debug_load_batch(batch, ok, 1000)
        ms = fold_ms(eng)
        rows, index, _, dropped = eng.fetch_pareto()
        assert dropped == extra and len(index) == cap, (rule, dropped, len(index))
        return ms, rows.metrics.copy()

    # worst: a whole batch of mutually non-dominated points
    anti = line(np.random.default_rng(3).permutation(n), n)

    def worst(rule):
        eng.track_pareto(cap, LINE, keep=rule)
        eng._debug_load_batch(anti, ok, 0)
        ms = fold_ms(eng)
        rows, index, _, dropped = eng.fetch_pareto()
        assert dropped == n - cap and len(index) == cap, (rule, dropped, len(index))
        return ms, rows.metrics.copy()

    for name, case, whole in (("steady", steady, front), ("worst", worst, anti)):
        for rule in RULES:
            case(rule)      # untimed
        ms, kept = {r: [] for r in RULES}, {}
        for _ in range(a.reps):
            for rule in RULES:
                t, kept[rule] = case(rule)
                ms[rule].append(t)
        out[name] = {rule: {"fold_ms_median": median(ms[rule]), "fold_ms_min": min(ms[rule]), "fold_ms_max": max(ms[rule]),
                            "covering_radius": covering_radius(whole, kept[rule])} for rule in RULES}
    eng.track_pareto(0)

    # breed: a run whose folds overflow
    pol = ActionWeights()
    res = eng.rollout_batch(pol, 4711, 8)
    parents = [Plan.from_result(res, e, f"sampled {e}") for e in range(8)]
    kw = dict(generations=4, cap=8, max_variants=256)

    def breed(rule):
        eng.sync()
        t0 = time.perf_counter()
        f = eng.breed_front(pol, parents, 91, 0, keep=rule, **kw)
        eng.sync()
        return 1e3 * (time.perf_counter() - t0), f

    for rule in RULES:
        breed(rule)      # untimed
    ms, last = {r: [] for r in RULES}, {}
    for _ in range(a.breed_reps):
        for rule in RULES:
            t, last[rule] = breed(rule)
            ms[rule].append(t)
    out["breed"] = {rule: {"run_ms_median": median(ms[rule]), "run_ms_all": ms[rule], "generations": len(last[rule].generations),
                           "variants": sum(g.n_variants for g in last[rule].generations), "n_dropped": sum(g.n_dropped for g in last[rule].generations),
                           "kept": len(last[rule].plans)} for rule in RULES}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
