"""N ranks in one process (include/eirgrid_hip.h eg_group_*; eirgrid-hip --gpus / --devices).

CPU: the CLI's new flags and their refusals.  GPU: a multi-rank CLI run writes the files a single-device run of the same command
writes (ranks sharing device 0, and on two devices when there are two); the cross-rank `best_result` fold (k_fold_gathered)
against a host fold of every rank's results in global index order; empty shards and the replicas' policies against one context."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def run(*args, timeout=600):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=timeout)


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_help_lists_the_rank_flags(built):
    out = run("--help")
    assert out.returncode == 0
    assert "--gpus" in out.stdout and "--devices" in out.stdout


@pytest.mark.parametrize("flags", [("--devices", "0,,1"), ("--devices", "a"), ("--devices", "0,-1"), ("--devices", ""),
                                   ("--devices", "1,"), ("--gpus", "0"), ("--gpus", "2x"),
                                   ("--devices", "0,0", "--update", "sequential"), ("--gpus", "2", "--update", "sequential"),
                                   ("--device", "0", "--devices", "0,0"), ("--gpus", "2", "--device", "1"),
                                   ("--gpus", "2", "--devices", "0,1")])
def test_bad_rank_flags_exit_2_before_any_device(built, tmp_path, flags):
    out = run("--world", WORLD, "-n", "4", "-c", str(tmp_path / "ck"), *flags)
    assert out.returncode == 2, (flags, out.stdout, out.stderr)
    assert "error:" in out.stderr
    assert "World:" not in out.stdout and not (tmp_path / "ck").exists()      # refused at parse time: no world, no device, no files


# ---- GPU: the CLI ----------------------------------------------------------------------------------------------------------

_ISO = re.compile(r"\d{4}-\d{2}-\d{2}[T ][0-9:.]+(?:Z|[+-]\d{2}:?\d{2})?")


def _run_files(ck):
    """What a run leaves behind that must not depend on the number of ranks, normalised for wall-clock stamps."""
    runs = os.listdir(ck)
    assert len(runs) == 1, runs
    rd = os.path.join(ck, runs[0])
    files = {}
    for name in ("latest_weights.json", "thread_0_weights.json", "best_weights.json"):
        text = open(os.path.join(rd, name)).read()
        files[name] = "\n".join(l for l in text.split("\n") if '"timestamp"' not in l)      # improvement-history stamps
        json.loads(text)
    files["checkpoint_iteration.txt"] = open(os.path.join(rd, "checkpoint_iteration.txt")).read()
    stamps = os.listdir(os.path.join(rd, "enhanced_csv"))
    assert len(stamps) == 1, stamps
    ed = os.path.join(rd, "enhanced_csv", stamps[0])
    for dirpath, _, names in os.walk(ed):
        for n in names:
            if n.endswith(".csv"):
                text = open(os.path.join(dirpath, n), encoding="utf-8").read()
                text = "\n".join(_ISO.sub("<stamp>", l) for l in text.split("\n") if stamps[0] not in l)
                files[os.path.relpath(os.path.join(dirpath, n), ed)] = text
    assert "simulation_summary.csv" in files
    return files


def _summary(stdout):
    lines = stdout.split("\n")
    i = next(k for k, l in enumerate(lines) if l.startswith("BEST SIMULATION RESULTS SUMMARY (iteration "))
    return lines[i:i + 6]


def _train(tmp, tag, devices, n, extra, cache, stop_after=None):
    ck = str(tmp / f"ck_{tag}")
    base = ["--world", WORLD, "-n", str(n), "--batch", "1024", "-i", "4", "--seed", "11", "-r", "100000", "-c", ck, *extra]
    if cache:
        base += ["-C", str(cache)]
    else:
        base += ["-C", str(tmp / "no_cache_here")]
    if devices:
        base += ["--devices", devices]
    if stop_after:
        out = run(*base, "--stop-after", str(stop_after))
        assert out.returncode == 0, out.stdout + out.stderr
        assert f"Stopped after {stop_after} iterations" in out.stdout
    out = run(*base)
    assert out.returncode == 0, out.stdout + out.stderr
    if devices:
        assert f"Ranks: {len(devices.split(','))} on devices" in out.stdout
    return _run_files(ck), _summary(out.stdout)


def _cache(tmp):
    d = tmp / "cache"
    d.mkdir(exist_ok=True)
    (d / "location_analysis.json").write_text("{}\n")      # only its existence matters (multi_simulation.rs:150-154)
    return d


def _compare(tmp, rank_sets, n, extra=(), cache=True, stop_after=None):
    c = _cache(tmp) if cache else None
    ref_files, ref_summary = _train(tmp, "single", None, n, extra, c, stop_after)
    for devices in rank_sets:
        files, summary = _train(tmp, devices.replace(",", "_"), devices, n, extra, c, stop_after)
        assert sorted(files) == sorted(ref_files), devices
        for name in ref_files:
            assert files[name] == ref_files[name], (devices, name)
        assert summary == ref_summary, (devices, summary, ref_summary)


# 20 000 iterations in batches of 1 024: with the cache file the batch at 17 408 is cut to 592 at the replay switch (18 000)
# and the batches after it replay; 0,0,0 shards a batch of 1 024 as 342 / 341 / 341.
@pytest.mark.gpu
def test_cli_ranks_write_what_one_device_writes(built, tmp_path):
    _compare(tmp_path, ["0,0", "0,0,0"], 20000)


@pytest.mark.gpu
def test_cli_ranks_stop_and_resume(built, tmp_path):
    _compare(tmp_path, ["0,0", "0,0,0"], 20000, stop_after=8192)


@pytest.mark.gpu
def test_cli_ranks_without_cache_replay_every_batch(built, tmp_path):
    _compare(tmp_path, ["0,0", "0,0,0"], 8000, cache=False)


@pytest.mark.gpu
def test_cli_ranks_cost_only(built, tmp_path):
    _compare(tmp_path, ["0,0", "0,0,0"], 6000, extra=("--cost-only",))


@pytest.mark.gpu
def test_cli_ranks_on_two_devices(built, tmp_path):
    from eirgrid_amd import _native as N
    if N.lib().eg_device_count() < 2:
        pytest.skip("needs two devices")
    _compare(tmp_path, ["0,1"], 20000)


@pytest.mark.gpu
def test_cli_gpus_beyond_the_visible_devices_exits_2(built, tmp_path):
    from eirgrid_amd import _native as N
    have = N.lib().eg_device_count()
    out = run("--world", WORLD, "-n", "4", "-c", str(tmp_path / "ck"), "--gpus", str(have + 1))
    assert out.returncode == 2 and "device(s) visible" in out.stderr, out.stderr


# ---- GPU: the library ----------------------------------------------------------------------------------------------------

def _shard(total, rank, n):
    """parallel.shard_range, restated (that module imports torch, which must not come after the library has initialised HIP)."""
    base, rem = divmod(total, n)
    return rank * base + min(rank, rem), base + (1 if rank < rem else 0)


_RECORD_FIELDS = ("metrics", "yearly", "status", "n_run", "n_def", "n_act", "run_log", "def_log", "act_log", "n_gens", "gen_cell",
                  "gen_pack", "n_offsets", "off_pack", "n_draws", "bytes_moved", "n_chunks")


@pytest.mark.gpu
@pytest.mark.parametrize("cost_only", [False, True])
def test_group_fold_is_the_host_fold_in_global_order(world, cost_only):
    """Three ranks on device 0, uneven and empty shards: after every step the group's held run is the one a literal fold of every
    rank's results in global index order holds, and its record is that episode's record."""
    from eirgrid_amd.engine import ActionWeights, Group, evaluate_action_impact
    g = Group(world, devices=(0, 0, 0))
    try:
        w = ActionWeights()
        g.push(w)
        g.track_best_result(cost_only=cost_only)
        sizes = [1000, 998, 1001, 700, 2, 1, 512, 333, 1000, 999, 64, 1000, 997, 3, 1000, 1000, 258, 1000, 1001, 500]
        best = idx = rec = None
        takeovers = {0: 0, 1: 0, 2: 0}
        first, seed = 0, 4242
        for step, n in enumerate(sizes):
            g.step(seed, first, n, 3, seed + first)      # every third global index replays once a best strategy exists
            for r, rank in enumerate(g.ranks):
                off, cnt = _shard(n, r, g.n_ranks)
                res = rank.fetch(cnt)
                winner = None
                for j in range(cnt):
                    if res.status[j] != 0:
                        continue
                    m = res.metrics[j]
                    if best is None or evaluate_action_impact(m, best, cost_only) > 0.0:
                        best, idx, winner = m.copy(), first + off + j, j
                        takeovers[r] += 1
                if winner is not None:
                    rec = rank.fetch_record(winner)
            got_idx, got = g.fetch_best_result()
            assert got_idx == idx, (step, got_idx, idx)
            for f in _RECORD_FIELDS:
                assert getattr(got, f).tobytes() == getattr(rec, f).tobytes(), (step, f)
            first += n
        assert takeovers[1] + takeovers[2] > 0, takeovers      # the winner's record did come from another rank than 0
    finally:
        g.close()


def _policy_state(w):
    tabs = w.tables()
    return ([t.tobytes() for t in tabs], [w.lists(k) for k in range(4)],
            {name: w.get(name) for name in w.SC})


@pytest.mark.gpu
@pytest.mark.parametrize("devices,sizes", [((0, 0), [700, 513, None, 1, 300, 1]), ((0, 0, 0), [700, 512, None, 2, 301, 2]),
                                           ((0, 0), [8191, 8192, 1, 16385])])
def test_group_replicas_equal_one_context(world, devices, sizes):
    """Every rank's policy is bit-identical to every other rank's and to one context's eg_device_step over the same global
    batches — also across steps whose shards are empty (n_global < N).  None in `sizes`: a fresh policy is pushed to both
    sides, after which an empty shard's packet would still hold its candidate from before the push, were it sent as it is.  8 191 across
    two ranks: one shard of 4 096 (replicated statistics) and one of 4 095 (added directly)."""
    from eirgrid_amd.engine import ActionWeights, Engine, Group
    g = Group(world, devices=devices)
    single = Engine(world, device=0)
    try:
        start = ActionWeights()
        g.push(start); single.push(start)
        pulled = [ActionWeights() for _ in devices]
        ref = ActionWeights()
        first, seed = 0, 77
        for n in sizes:
            if n is None:
                fresh = ActionWeights()
                g.push(fresh); single.push(fresh)
                continue
            g.step(seed, first, n, 2, seed + first)
            single.device_step(seed, first, n, 2, seed + first)
            first += n
            single.pull(ref)
            want = _policy_state(ref)
            for r in range(len(devices)):
                g.pull(r, pulled[r])
                assert _policy_state(pulled[r]) == want, (n, r)
        assert ref.get("has_best") == 1.0
    finally:
        g.close()
        single.close()
