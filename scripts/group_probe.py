"""Per-update time of an eg_group step against one context's eg_device_step at the same global batch.

    python scripts/group_probe.py --ranks 2 --global-batch 16384 --steps 30
    python scripts/group_probe.py --ranks 8 --global-batch 131072 --steps 10 --devices 0,0,0,0,0,0,0,0

Both sides start from a fresh policy, track the best_result fold and replay every 10th global index once a best strategy exists;
the first --warmup steps are not timed.  Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the k_fold_pack /
k_fold_gathered rows give the fold's own share."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--devices", default=None, help="comma-separated device per rank (default: all ranks on device 0)")
    ap.add_argument("--global-batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--period", type=int, default=10)
    ap.add_argument("--no-single", action="store_true", help="time the group only")
    a = ap.parse_args()
    from eirgrid_amd import synthetic_world
    from eirgrid_amd.engine import ActionWeights, Engine, Group

    world = synthetic_world()
    devices = [int(d) for d in a.devices.split(",")] if a.devices else [0] * a.ranks
    n = a.global_batch

    def timed(step, sync):
        per = []
        for s in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            step(s)
            sync()
            if s >= a.warmup:
                per.append(time.perf_counter() - t0)
        per.sort()
        return {"median_ms": 1e3 * per[len(per) // 2], "min_ms": 1e3 * per[0]}

    out = {"ranks": len(devices), "devices": devices, "global_batch": n, "steps": a.steps}
    g = Group(world, devices=devices)
    g.push(ActionWeights())
    g.track_best_result()
    out["group"] = timed(lambda s: g.step(5, s * n, n, a.period, 5 + s * n), lambda: [r.sync() for r in g.ranks])
    g.close()
    if not a.no_single:
        e = Engine(world, device=devices[0])
        e.push(ActionWeights())
        e.track_best_result()
        out["single"] = timed(lambda s: e.device_step(5, s * n, n, a.period, 5 + s * n), e.sync)
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
