"""GPU: the top-K archive of distinct scenarios (include/eirgrid_hip.h eg_top_k_track; csrc/eg_topk.h) against a host restatement of
its definition — rank score, key, identity, earliest occurrence, order — batch after batch while the device update changes the policy
and the replay list; the all-replay batch; the replay hoist; the policy's best strategy; groups with empty shards; the CLI's export."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")

RECORD_FIELDS = ("metrics", "yearly", "status", "n_run", "n_def", "n_act", "run_log", "def_log", "act_log", "n_gens", "gen_cell",
                 "gen_pack", "n_offsets", "off_pack", "n_draws", "bytes_moved", "n_chunks")
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _splitmix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys(n_act, act_log):
    """The key of include/eirgrid_hip.h, restated: n_act[26] as little-endian int32 ++ act_log[0 .. sum n_act), zero-padded to
    8-byte words w_i, key = sum_i splitmix64(w_i + i * 0x9E3779B97F4A7C15) mod 2^64 — for every row at once."""
    n = n_act.shape[0]
    a = np.clip(n_act.astype(np.int64).sum(axis=1), 0, act_log.shape[1])
    log = np.where(np.arange(act_log.shape[1])[None, :] < a[:, None], act_log, 0).astype(np.uint8)
    raw = np.concatenate([np.ascontiguousarray(n_act.astype("<i4")).view(np.uint8).reshape(n, -1), log], axis=1)
    words = np.ascontiguousarray(raw).view("<u8").astype(np.uint64)
    i = np.arange(words.shape[1], dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _splitmix64(words + i[None, :] * GOLDEN)
    h = np.where(i[None, :] < ((104 + a[:, None] + 7) // 8).astype(np.uint64), h, np.uint64(0))
    return h.sum(axis=1, dtype=np.uint64)


class Archive:
    """The definition, literally: every distinct scenario (metrics bits, key) at its earliest index; the archive is the k best by
    score descending, ties to the lower index.  Records are taken from the engine when an entry from the current batch enters."""

    def __init__(self, k, cost_only):
        self.k, self.cost_only = k, cost_only
        self.seen = {}      # identity -> (score, index)
        self.records = {}   # index -> one-episode BatchResult

    def feed(self, eng, res, first):
        from eirgrid_amd.engine import rank_score
        key = keys(res.n_act, res.act_log)
        for e in range(len(res.status)):
            if res.status[e] != 0:
                continue
            s = rank_score(res.metrics[e], self.cost_only)
            if s != s:
                continue
            ident = (res.metrics[e].tobytes(), int(key[e]))
            if ident not in self.seen or first + e < self.seen[ident][1]:
                self.seen[ident] = (s, first + e)
        top = self.top()
        for s, idx in top:
            if first <= idx < first + len(res.status) and idx not in self.records:
                self.records[idx] = eng.fetch_record(idx - first)
        return top

    def top(self):
        return sorted(self.seen.values(), key=lambda t: (-t[0], t[1]))[:self.k]


def assert_archive(got, want, records, what):
    rows, scores, index = got
    assert [int(i) for i in index] == [i for _, i in want], (what, index, [i for _, i in want])
    assert np.array([s for s, _ in want], dtype=np.float64).tobytes() == scores.tobytes(), what
    for r, (_, idx) in enumerate(want):
        rec = records[idx]
        for f in RECORD_FIELDS:
            assert getattr(rows, f)[r].tobytes() == getattr(rec, f)[0].tobytes(), (what, r, idx, f)


def assert_same_archive(a, b, what):
    """Entries and records byte for byte — n_chunks excepted: it counts what the search that really ran requested, and the hoisted
    replay and the small-batch kernel run other searches for the same cells (include/eirgrid_hip.h eg_replay_hoist)."""
    assert a[2].tolist() == b[2].tolist() and a[1].tobytes() == b[1].tobytes(), (what, a[2], b[2])
    for f in RECORD_FIELDS[:-1]:
        assert getattr(a[0], f).tobytes() == getattr(b[0], f).tobytes(), (what, f)


@pytest.mark.gpu
@pytest.mark.parametrize("cost_only", [False, True])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_archive_is_the_host_restatement(world, k, cost_only):
    """Six batches of 4096 with the device update between them (the policy and the replay list change) and every tenth episode a
    replay: after each batch the archive's indices and scores equal the restatement's bit for bit, and every record equals the one
    eg_fetch_record gave when its episode ran."""
    from eirgrid_amd.engine import ActionWeights, Engine
    eng = Engine(world, device=0)
    try:
        eng.push(ActionWeights())
        eng.track_top_k(k, cost_only=cost_only)
        ref = Archive(k, cost_only)
        first, seed = 0, 9001
        for b in range(6):
            eng.device_step(seed, first, 4096, 10, seed + first)
            res = eng.fetch(4096)
            want = ref.feed(eng, res, first)
            assert_archive(eng.fetch_top_k(), want, ref.records, (k, cost_only, b))
            first += 4096
        assert len(want) == k
    finally:
        eng.close()


@pytest.mark.gpu
def test_all_replay_batch_adds_one_entry_at_its_lowest_index(world):
    from eirgrid_amd.engine import ActionWeights, Engine
    eng = Engine(world, device=0)
    try:
        eng.push(ActionWeights())
        eng.device_step(5, 0, 1024, 0, 5)      # a best strategy to replay
        eng.track_top_k(10)
        eng.device_step(5, 1024, 2048, 1, 6)
        res = eng.fetch(2048)
        assert (res.status == 0).all()
        rows, scores, index = eng.fetch_top_k()
        assert index.tolist() == [1024]
        assert len({(res.metrics[e].tobytes(), res.act_log[e].tobytes()) for e in range(2048)}) == 1
    finally:
        eng.close()


@pytest.mark.gpu
def test_replay_hoist_gives_the_same_archive(world):
    from eirgrid_amd.engine import ActionWeights, Engine
    a, b = Engine(world, device=0), Engine(world, device=0)
    try:
        b.replay_hoist(True)
        for e in (a, b):
            e.push(ActionWeights())
            e.track_top_k(16)
        first = 0
        for n, period in ((4096, 0), (4096, 10), (4096, 3), (2048, 1)):
            for e in (a, b):
                e.device_step(31, first, n, period, 31 + first)
            first += n
            assert_same_archive(a.fetch_top_k(), b.fetch_top_k(), (n, period))
        armed, _ = b.replay_hoist_stats()
        assert armed >= 3, armed
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_first_entry_is_the_policys_best_strategy(world):
    """Mode 1 ranks by score_metrics, the policy's best strategy is the running maximum of the same score with strict > (strategy.rs:
    52-66): in a fresh run entry 1 is that episode, record for record."""
    from eirgrid_amd.engine import ActionWeights, Engine
    eng = Engine(world, device=0)
    try:
        eng.push(ActionWeights())
        eng.track_top_k(10)
        first = 0
        for n in (4096, 4096, 4096, 2000):
            eng.device_step(77, first, n, 10, 77 + first)
            first += n
            state, best = eng.fetch_best_run()
            rows, scores, index = eng.fetch_top_k()
            assert state == 1
            for f in RECORD_FIELDS:
                assert getattr(rows, f)[0].tobytes() == getattr(best, f)[0].tobytes(), (n, f)
        pol = ActionWeights()
        eng.pull(pol)
        assert [pol.get(n) for n in ("best_net_emissions", "best_opinion", "best_cost")] == rows.metrics[0][:3].tolist()
    finally:
        eng.close()


def _shard(n, r, N):
    base, rem = divmod(n, N)
    return r * base + min(r, rem), base + (1 if r < rem else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("devices,cost_only", [((0, 0), False), ((0, 0, 0), True)])
def test_group_archive_equals_one_context(world, devices, cost_only):
    """Ranks on device 0, shards of uneven size and empty ones (n_global < N): after every step the group's archive — entries and the
    records fetched from the ranks that ran them — is byte for byte one context's over the same global batches."""
    from eirgrid_amd.engine import ActionWeights, Engine, Group
    g = Group(world, devices=devices)
    single = Engine(world, device=0)
    try:
        w = ActionWeights()
        g.push(w); single.push(w)
        g.track_top_k(12, cost_only=cost_only); single.track_top_k(12, cost_only=cost_only)
        first, seed = 0, 555
        owners = set()
        for n in (4096, 2, 3001, 1, 4096, 1024):
            g.step(seed, first, n, 10, seed + first)
            single.device_step(seed, first, n, 10, seed + first)
            got, want = g.fetch_top_k(), single.fetch_top_k()
            assert_same_archive(got, want, (devices, n))
            for i in got[2]:
                for r in range(len(devices)):
                    off, cnt = _shard(n, r, len(devices))
                    if off <= i - first < off + cnt:
                        owners.add(r)
            first += n
        if not cost_only:      # (cost_only: every run within the acceptable cost scores 2.0, and the ties go to the first shard)
            assert len(owners) > 1, owners      # records did come from more than one rank
    finally:
        g.close(); single.close()


def _run(*args, timeout=900):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=timeout)


_ISO = re.compile(r"\d{4}-\d{2}-\d{2}[T ][0-9:.]+(?:Z|[+-]\d{2}:?\d{2})?")


def _top_k_tree(ck):
    runs = os.listdir(ck)
    assert len(runs) == 1, runs
    rd = os.path.join(ck, runs[0])
    stamps = os.listdir(os.path.join(rd, "enhanced_csv"))
    assert len(stamps) == 1, stamps
    tk = os.path.join(rd, "enhanced_csv", stamps[0], "top_k")
    files = {}
    for dirpath, _, names in os.walk(tk):
        for n in names:
            text = open(os.path.join(dirpath, n), encoding="utf-8").read()
            files[os.path.relpath(os.path.join(dirpath, n), tk)] = "\n".join(_ISO.sub("<stamp>", l).replace(stamps[0], "<stamp>")
                                                                           for l in text.split("\n"))
    return rd, files


@pytest.mark.gpu
def test_cli_top_k_on_ranks_writes_what_one_device_writes(built, tmp_path):
    cache = tmp_path / "cache"
    cache.mkdir()
    (cache / "location_analysis.json").write_text("{}\n")      # replays in the last 10 % only (multi_simulation.rs:150-154, :437-465)
    trees = []
    for tag, extra in (("single", ()), ("ranks", ("--devices", "0,0"))):
        ck = str(tmp_path / f"ck_{tag}")
        out = _run("--world", WORLD, "-n", "6000", "--batch", "1024", "-i", "4", "--seed", "11", "-r", "100000", "-c", ck,
                   "-C", str(cache), "--top-k", "8", *extra)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Top 8 distinct scenarios (8 held)" in out.stdout
        trees.append(_top_k_tree(ck)[1])
    assert sorted(trees[0]) == sorted(trees[1])
    assert "index.csv" in trees[0] and "08/simulation_summary.csv" in trees[0] and "01/yearly_details/generators.csv" in trees[0]
    for name in trees[0]:
        assert trees[0][name] == trees[1][name], name


@pytest.mark.gpu
def test_cli_top_k_row_one_is_the_best_weights_metrics(built, tmp_path):
    ck = str(tmp_path / "ck")
    out = _run("--world", WORLD, "-n", "3000", "--batch", "1024", "--seed", "3", "-r", "100000", "-c", ck, "-C", str(tmp_path / "nc"),
               "--no-continue", "--top-k", "4")
    assert out.returncode == 0, out.stdout + out.stderr
    rd, files = _top_k_tree(ck)
    rows = [l.split(",") for l in files["index.csv"].strip().split("\n")]
    assert rows[0] == ["rank", "score", "iteration", "final_net_emissions", "average_public_opinion", "total_cost", "power_reliability"]
    assert [r[0] for r in rows[1:]] == ["1", "2", "3", "4"]
    bm = json.load(open(os.path.join(rd, "best_weights.json")))["best_metrics"]
    got = [float(x) for x in rows[1][3:7]]
    assert got == [bm["final_net_emissions"], bm["average_public_opinion"], bm["total_cost"], bm["power_reliability"]]
    scores = [float(r[1]) for r in rows[1:]]
    assert scores == sorted(scores, reverse=True)


def _block_entries(res, k, cost_only, spans):
    """What k_topk_merge reads from a batch folded into an archive that is not full yet (every successful episode passes k_topk_keys),
    restated: per span of episodes — a chunk of k_topk_select, or a rank's shard — its distinct scenarios (metrics bits, key) with a
    rank score, at most k of them."""
    from eirgrid_amd.engine import rank_score
    key = keys(res.n_act, res.act_log)
    total = 0
    for lo, hi in spans:
        ids = set()
        for e in range(lo, hi):
            s = rank_score(res.metrics[e], cost_only)
            if res.status[e] == 0 and s == s:
                ids.add((res.metrics[e].tobytes(), int(key[e])))
        total += min(k, len(ids))
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("cost_only", [False, True])
@pytest.mark.parametrize("k", [63, 64])
def test_archive_at_production_size_is_the_host_restatement(world, k, cost_only):
    """Four batches of 16 384 (configs[2]'s size: 16 blocks of k_topk_select) with the device update between them: the first batch's
    blocks hold more than k_topk_merge's 512 list entries, so the merge compacts its list between blocks; after every batch the archive
    is the restatement's, entries and records."""
    from eirgrid_amd.engine import ActionWeights, Engine
    eng = Engine(world, device=0)
    try:
        eng.push(ActionWeights())
        eng.track_top_k(k, cost_only=cost_only)
        ref = Archive(k, cost_only)
        first, seed, n = 0, 4242, 16384
        for b in range(4):
            eng.device_step(seed, first, n, 10, seed + first)
            res = eng.fetch(n)
            if b == 0:
                entries = _block_entries(res, k, cost_only, [(c, min(c + 1024, n)) for c in range(0, n, 1024)])
                assert entries > 512, entries
            want = ref.feed(eng, res, first)
            assert_archive(eng.fetch_top_k(), want, ref.records, (k, cost_only, b))
            first += n
        assert len(want) == k
        print(f"k {k} cost_only {cost_only}: the first batch's blocks hold {entries} entries")
    finally:
        eng.close()


@pytest.mark.gpu
def test_group_of_eight_ranks_archive_equals_one_context(world):
    """Eight ranks on device 0 with K = 64.  A first step of 5 episodes leaves a few entries held, so that in the next one (16 384) the
    archive is not full, every rank's block is full and each rank's merge reads held + 8 x 64 > 512 entries: it compacts its list
    before the last block.  Steps whose global batch is smaller than eight leave shards empty.  After every step the archive equals one
    context's, and that one the restatement's: one context runs the same merge kernel, and a fault in it can give both the same wrong
    archive."""
    from eirgrid_amd.engine import ActionWeights, Engine, Group
    g = Group(world, devices=(0,) * 8)
    single = Engine(world, device=0)
    try:
        w = ActionWeights()
        g.push(w); single.push(w)
        g.track_top_k(64); single.track_top_k(64)
        ref = Archive(64, False)
        first, seed = 0, 808
        held = 0
        for step, n in enumerate((5, 16384, 3, 16384, 8191, 4096)):
            g.step(seed, first, n, 10, seed + first)
            single.device_step(seed, first, n, 10, seed + first)
            res = single.fetch(n)
            if step == 1:
                spans = [(o, o + c) for o, c in (_shard(n, r, 8) for r in range(8))]
                entries = held + _block_entries(res, 64, False, spans)
                assert 0 < held < 64 and entries > 512, (held, entries)
            got, want = g.fetch_top_k(), single.fetch_top_k()
            assert_same_archive(got, want, n)
            assert_archive(want, ref.feed(single, res, first), ref.records, ("eight ranks", step))      # (and got == want)
            held = len(want[2])
            first += n
        print(f"eight ranks: the 16 384-episode step's merges read {entries} entries")
        assert len(got[2]) == 64
    finally:
        g.close(); single.close()
