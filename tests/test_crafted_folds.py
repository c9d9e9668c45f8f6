"""CPU: the crafted batches of tests/test_gpu_crafted_folds.py and the restatements they are compared with — the four device reductions
that decide what a run keeps (the top-K archive, the best_result fold, the update's best pick, the refinement's pick) on inputs real
episodes never produce.  Here: the batches are what they claim to be, the best_result restatement (tests/test_best_result_fold.py _fold)
agrees with the oracle's fold on every one of them, the top-K restatement (tests/test_gpu_top_k.py Archive, keys) gives the hand-counted
answers, and the two picks' restatements give theirs.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

from eirgrid_amd import _native as N
from tests.test_best_result_fold import _fold, _random_metrics
from tests.test_gpu_top_k import Archive, keys

FAILED = -2          # EG_EP_NO_LOCATION: any status other than EG_EP_OK
FAR = 2**32 - 5      # a first_index whose batch crosses 2^32
CAP = N.ACT_CAP


# ---- metrics with a chosen order of scores ------------------------------------------------------------------------------------------
def level_metrics(level, reliability=1.0):
    """Metrics [n,4] whose rank score rises strictly with `level` (integers 0 .. 16 384) in both modes: above net zero mode 1 scores
    1 - emissions / 1e6, mode 2 falls with log(cost) above the acceptable cost of 5e10.  Equal levels give equal bits."""
    level = np.asarray(level, dtype=np.float64)
    return np.stack([500000.0 - level, np.full(level.shape, 0.5), 1e11 - 1e6 * level, np.broadcast_to(np.asarray(reliability, dtype=np.float64), level.shape)], axis=1)


def stair_metrics(level):
    """Metrics whose emissions (all above net zero) and cost rise strictly with `level`: in the best_result fold a result takes over
    exactly when its level is ABOVE the held one's, in both modes (scoring.rs:46-85 with the arguments as multi_simulation.rs:616 passes
    them); equal levels give an impact of exactly 0.0."""
    level = np.asarray(level, dtype=np.float64)
    return np.stack([1000.0 + level, np.full(level.shape, 0.5), 1e9 + level, np.ones(level.shape)], axis=1)


def tag_bytes(index):
    """What eg_debug_load_batch writes into run_log[0..8) and def_log[0..8) of the record with global index `index`."""
    g = np.uint64(int(index) & (2**64 - 1))
    return np.array([g], "<u8").tobytes(), np.array([~g], "<u8").tobytes()


# ---- best_result: the batches --------------------------------------------------------------------------------------------------------
FOLD_SIZES = (1, 1023, 1024, 1025, 8191, 8192, 8193, 16385)      # the window (1024) and tile (8192) edges of fold_windows
TAKEOVER_AT = (0, 1023, 1024, 8191, 8192)


def takeover_levels(n, at=TAKEOVER_AT):
    """Levels under which exactly the positions `at` (below n) take over: the level steps up there; every other position holds the
    held level (impact 0.0) when even and one below it when odd."""
    step = np.zeros(n, np.int64)
    step[[p for p in at if p < n]] = 1
    held = np.cumsum(step)
    i = np.arange(n)
    return np.where(step == 1, held, np.where(i % 2 == 0, held, held - 1)).astype(np.float64)


def fold_cases():
    """name -> list of batches (status, metrics, first_index), folded one after the other from an empty state."""
    rng = np.random.default_rng(20)
    ok = lambda n: np.zeros(n, np.int32)
    cases = {}
    for n in FOLD_SIZES:
        st = np.where(rng.uniform(size=n) < 0.1, FAILED, 0).astype(np.int32)
        cases[f"random {n}"] = [(st, _random_metrics(rng, n), FAR if n in (1, 8193) else 7)]
        cases[f"take-overs at the edges {n}"] = [(ok(n), stair_metrics(takeover_levels(n)), 0)]
    cases["rising staircase"] = [(ok(2049), stair_metrics(np.arange(2049)), FAR)]
    cases["falling staircase"] = [(ok(2049), stair_metrics(np.arange(2049)[::-1]), 3)]
    cases["equal metrics"] = [(ok(1500), stair_metrics(np.full(1500, 4.0)), 11)]
    st = ok(1300); st[[0, 1, 2, 1023, 1024]] = FAILED
    cases["failed at position 0"] = [(st, stair_metrics(takeover_levels(1300, (3, 1025))), 0)]
    cases["all failed"] = [(np.full(1100, FAILED, np.int32), stair_metrics(np.arange(1100)), 0)]
    # three batches: take-overs, then none (lower levels, equal levels and failures), then one at the very end
    quiet = ok(1025); quiet[::7] = FAILED
    cases["three batches"] = [(ok(1500), stair_metrics(100.0 + takeover_levels(1500)), FAR),
                              (quiet, stair_metrics(np.where(np.arange(1025) % 3 == 0, 102.0, 50.0)), FAR + 1500),
                              (ok(1025), stair_metrics(np.where(np.arange(1025) == 1024, 200.0, 102.0)), FAR + 2525)]
    inf, nan = np.inf, np.nan
    for col, name in ((0, "emissions"), (1, "opinion"), (2, "cost")):
        for below in (False, True):      # above / below net zero: the two branches of scoring.rs:46-85
            m = _random_metrics(np.random.default_rng(30 + col), 1200)
            m[:, 0] = -np.abs(m[:, 0]) if below else np.abs(m[:, 0]) + 1.0
            for k, v in enumerate((nan, inf, -inf, nan, -inf, inf)):
                m[(5, 300, 700, 1023, 1024, 1199)[k], col] = v
            cases[f"NaN and infinities in {name}, {'below' if below else 'above'} net zero"] = [(ok(1200), m, 0)]
            for v in (nan, inf, -inf):      # ... held from the start: nothing is held before position 0
                h = m.copy(); h[0, col] = v
                cases[f"{v} in {name} at position 0, {'below' if below else 'above'} net zero"] = [(ok(1200), h, 0)]
    return cases


# ---- top-K: the batches --------------------------------------------------------------------------------------------------------------
TOPK_SIZES = (1, 1023, 1024, 1025, 4097, 9217)      # the chunk (1024) edges of k_topk_select; ten blocks pass k_topk_merge's 512 entries
KEY_TOTALS = (0, 1, 7, 8, 9, CAP - 1, CAP)


def batch(metrics, status=None, n_act=None, act_log=None):
    n = len(metrics)
    return SimpleNamespace(metrics=np.ascontiguousarray(metrics, dtype=np.float64), status=np.zeros(n, np.int32) if status is None else status,
                           n_act=np.zeros((n, N.YEARS), np.int32) if n_act is None else n_act,
                           act_log=np.zeros((n, CAP), np.uint8) if act_log is None else act_log)


def sized_batch(n, seed):
    """n records with shuffled distinct levels; about one in eight repeats an earlier record of the batch (metrics and action record), one
    in sixteen failed, a NaN score here and there; action records of 0..40 entries with noise behind them."""
    rng = np.random.default_rng(seed)
    b = batch(level_metrics(rng.permutation(n)))
    total = rng.integers(0, 41, n)
    b.n_act[:, 0] = total // 2; b.n_act[:, 3] = total - total // 2
    b.act_log[:, :48] = rng.integers(0, 61, (n, 48))
    for e in np.flatnonzero(rng.uniform(size=n) < 0.125):
        if e > 0:
            src = int(rng.integers(0, e))
            b.metrics[e] = b.metrics[src]; b.n_act[e] = b.n_act[src]
            a = int(b.n_act[src].sum())
            b.act_log[e, :a] = b.act_log[src, :a]      # (what lies behind the log stays its own)
    b.status[rng.uniform(size=n) < 1 / 16] = FAILED
    b.metrics[rng.uniform(size=n) < 1 / 64, :2] = (-1.0, np.nan)      # at or below net zero mode 1 reads the opinion: a NaN score
    b.metrics[rng.uniform(size=n) < 1 / 64, 0] = np.nan               # NaN emissions are "not above net zero": a score like any other
    return b


def key_edge_batch():
    """Equal metrics throughout.  For every total A of KEY_TOTALS four records: (a) a log of A entries with noise behind it, (b) the same
    with another byte right behind the log, (c) another last valid byte, (d) the same bytes with another per-year split of n_act.  (a) and
    (b) are one scenario, (c) and (d) two more (A = 0 has neither: one scenario).  Returns the batch and the scenario of every record."""
    rng = np.random.default_rng(40)
    rows, scen = [], []
    for A in KEY_TOTALS:
        log = rng.integers(1, 61, CAP).astype(np.uint8)
        na = np.zeros(N.YEARS, np.int32); na[2] = A
        rows.append((na, log)); scen.append((A, "a"))
        behind = log.copy()
        if A < CAP:
            behind[A] ^= 0x5A
        rows.append((na, behind)); scen.append((A, "a"))
        if A >= 1:
            last = log.copy(); last[A - 1] ^= 0x21
            rows.append((na, last)); scen.append((A, "c"))
            split = na.copy(); split[2] = A - 1; split[25] = 1
            rows.append((split, log)); scen.append((A, "d"))
    n = len(rows)
    return batch(level_metrics(np.full(n, 9.0)), n_act=np.stack([r[0] for r in rows]), act_log=np.stack([r[1] for r in rows])), scen


def equal_score_batch(n=4097):
    """One score, distinct reliabilities (which no score reads), successful only at the end of every chunk of 1 024."""
    b = batch(level_metrics(np.full(n, 5.0), reliability=np.arange(n) / 8192.0))
    b.status[np.arange(n) % 1024 < 1000] = FAILED
    return b


def identical_batch(n=2500):
    b = batch(level_metrics(np.full(n, 5.0)))
    b.n_act[:, 1] = 3; b.act_log[:, :3] = (4, 5, 6)
    b.status[0] = FAILED
    return b


def chunk_duplicate_batch(n=9217):
    """Chunk 8 repeats chunk 0, and they hold the batch's best scores: with k = 64 the ten blocks are 640 entries, k_topk_merge reduces its
    list before block 8 arrives, and chunk 8's entries must still be found to repeat what the reduction kept."""
    rng = np.random.default_rng(41)
    level = rng.permutation(n - 1024).astype(np.float64)
    level = np.concatenate([n + rng.permutation(1024), level])      # chunk 0 on top
    b = batch(level_metrics(level))
    b.n_act[:, 0] = 5; b.act_log[:, :5] = rng.integers(0, 61, (n, 5))
    b.metrics[8192:9216] = b.metrics[:1024]; b.act_log[8192:9216] = b.act_log[:1024]
    return b


def mode1_scores(b):
    """What the statistics epilogue leaves in score_list: score_metrics of a successful episode, -1.0 of a failed one."""
    from eirgrid_amd.engine import rank_score
    return np.array([rank_score(m, False) if st == 0 else -1.0 for st, m in zip(b.status, b.metrics)])


def feed(archive, eng, b, first):
    """Archive.feed under the archive's rule for -inf (include/eirgrid_hip.h, "failures"): only scores above -inf can enter."""
    from eirgrid_amd.engine import rank_score
    minus_inf = np.array([rank_score(m, archive.cost_only) == -np.inf for m in b.metrics])
    return archive.feed(eng, SimpleNamespace(metrics=b.metrics, status=np.where(minus_inf, FAILED, b.status), n_act=b.n_act, act_log=b.act_log), first)


# ---- the two picks, restated ---------------------------------------------------------------------------------------------------------
def pick_best(score_list, first_index):
    """k_pick_best: (score, global index) of the first maximum among the scores above -1.0; (-1.0, -1) when there is none."""
    best, at = -1.0, -1
    for i, s in enumerate(score_list):
        if s > best:
            best, at = s, i
    return (float(best), first_index + at) if at >= 0 else (-1.0, -1)


def refine_pick(status, metrics, mode):
    """The definition at the top of csrc/eg_refine_many.h: variant j is a candidate when its status is EG_EP_OK and its rank score is not NaN;
    the winner is the candidate with the largest score, ties to the lowest j; -1 when variant 0 is no candidate.
    Returns (winner, n_failed, the winner's score, base_ok, the base's score)."""
    from eirgrid_amd.engine import rank_score
    s = np.array([rank_score(np.ascontiguousarray(m), mode == 2) for m in metrics])
    cand = (np.asarray(status) == 0) & ~np.isnan(s)
    n_failed = int((~cand).sum())
    if not cand[0]:
        return -1, n_failed, 0.0, 0, float(s[0])
    winner = min(np.flatnonzero(cand), key=lambda j: (-s[j], j))
    return int(winner), n_failed, float(s[winner]), 1, float(s[0])


def refine_block(j):
    """Block j of eg_debug_refine_pick (include/eirgrid_hip.h), None: its base block."""
    w = np.arange(N.PLAN_BLOCK_BYTES // 4, dtype=np.uint64)
    b = (0xBA5E0000 + w if j is None else j * 0x9E3779B1 + w).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    b[130], b[158] = (7, 5) if j is None else (j % 4097, (j // 3) % 4097)
    return b.astype("<u4").view(np.uint8)


# ---- CPU tests -----------------------------------------------------------------------------------------------------------------------
def test_levels_order_the_scores_in_both_modes(built):
    from eirgrid_amd.engine import rank_score
    m = level_metrics(np.arange(0, 16385, 7))
    for cost_only in (False, True):
        s = np.array([rank_score(r, cost_only) for r in m])
        assert (np.diff(s) > 0).all() and np.isfinite(s).all(), cost_only
    a, b = level_metrics([3.0, 3.0], reliability=[0.25, 0.75])
    assert rank_score(a, False) == rank_score(b, False) and rank_score(a, True) == rank_score(b, True) and a.tobytes() != b.tobytes()
    assert rank_score(np.array([-5.0, -np.inf, 1e10, 1.0]), False) == -np.inf      # the -inf the issue speaks of
    assert np.isfinite(rank_score(np.array([-5.0, -np.inf, 1e10, 1.0]), True))


def test_fold_restatement_is_the_oracles_fold_on_every_crafted_case(built):
    """tests/test_best_result_fold.py _fold against oracle.api.BestResultFold: winner, metrics bits and the number of take-overs the
    staircases are built for."""
    from oracle import api as O
    takeovers = {}
    for name, batches in fold_cases().items():
        for cost_only in (False, True):
            f = O.BestResultFold(cost_only)
            best, index = None, None
            for st, m, first in batches:
                f.feed(st, m, first)
                with np.errstate(invalid="ignore"):      # (inf - inf and the like are the point of some cases)
                    best, index = _fold(st, m, cost_only, best, index, first)
                assert f.winner == index, (name, cost_only)
                if index is not None:
                    assert f.best.tobytes() == np.asarray(best).tobytes(), (name, cost_only)
            takeovers[name, cost_only] = (f.takeovers, f.winner)
    for cost_only in (False, True):
        assert takeovers["rising staircase", cost_only] == (2049, FAR + 2048)      # 1 024 restarts of a window, twice, and one more
        assert takeovers["falling staircase", cost_only] == (1, 3)
        assert takeovers["equal metrics", cost_only] == (1, 11)
        assert takeovers["failed at position 0", cost_only] == (2, 1025)
        assert takeovers["all failed", cost_only] == (0, None)
        assert takeovers["three batches", cost_only] == (4, FAR + 2525 + 1024)
        for n in FOLD_SIZES:
            at = [p for p in TAKEOVER_AT if p < n]
            assert takeovers[f"take-overs at the edges {n}", cost_only] == (len(at), at[-1])
    # a NaN held from position 0 is never improved on above net zero: it stays (an impact of NaN is not > 0.0)
    f = O.BestResultFold().feed(np.zeros(3, np.int32), np.array([[np.nan, 0.5, 1e9, 1.0], [5.0, 0.5, 1e9, 1.0], [1e5, 0.5, 1e9, 1.0]]))
    assert (f.takeovers, f.winner) == (1, 0)


def test_the_quiet_batch_of_three_takes_nothing_over(built):
    from oracle import api as O
    b = fold_cases()["three batches"]
    f = O.BestResultFold().feed(*b[0])
    held = f.winner
    assert f.feed(*b[1]).winner == held and f.feed(*b[2]).winner != held


class _NoEngine:
    def fetch_record(self, e):
        return e


def test_key_edges_by_hand(built):
    b, scen = key_edge_batch()
    key = keys(b.n_act, b.act_log)
    assert len(scen) == 1 * 2 + 6 * 4 and len(set(scen)) == 1 + 6 * 3
    for i in range(len(scen)):
        for j in range(i):
            assert (key[i] == key[j]) == (scen[i] == scen[j]), (scen[i], scen[j])
    for cost_only in (False, True):
        top = feed(Archive(64, cost_only), _NoEngine(), b, FAR)
        first_of = {s: FAR + scen.index(s) for s in scen}
        assert [i for _, i in top] == sorted(first_of.values())      # one score: the scenarios at their first index, in index order
        assert [i for _, i in feed(Archive(2, cost_only), _NoEngine(), b, 0)] == [0, 2]


def test_equal_and_identical_batches_by_hand(built):
    b = equal_score_batch()
    ok = np.flatnonzero(b.status == 0)
    assert len(ok) == 4 * 24 and ok[24] == 2024
    for k in (1, 2, 63, 64):
        assert [i for _, i in feed(Archive(k, False), _NoEngine(), b, 10)] == (10 + ok[:k]).tolist()
    assert [i for _, i in feed(Archive(64, True), _NoEngine(), identical_batch(), FAR)] == [FAR + 1]
    d = chunk_duplicate_batch()
    top = feed(Archive(64, False), _NoEngine(), d, 0)
    assert len(top) == 64 and all(i < 1024 for _, i in top)
    assert keys(d.n_act[:1024], d.act_log[:1024]).tolist() == keys(d.n_act[8192:9216], d.act_log[8192:9216]).tolist()


def test_minus_infinity_never_enters_and_nan_is_skipped(built):
    m = level_metrics(np.arange(4.0))
    m[1] = (-5.0, -np.inf, 1e10, 1.0)      # mode 1: -inf; mode 2: a score like any other
    m[2] = (-5.0, np.nan, 1e10, 1.0)       # mode 1: NaN
    b = batch(m)
    assert [i for _, i in feed(Archive(8, False), _NoEngine(), b, 0)] == [3, 0]
    assert sorted(i for _, i in feed(Archive(8, True), _NoEngine(), b, 0)) == [0, 1, 2, 3]


def test_sized_batches_hold_what_they_promise(built):
    for n in (1025, 4097):
        b = sized_batch(n, n)
        ident = {(b.metrics[e].tobytes(), b.n_act[e].tobytes(), b.act_log[e, :b.n_act[e].sum()].tobytes()) for e in range(n)}
        assert n // 16 < n - len(ident) < n // 4 and (b.status != 0).sum() > n // 32
        s = mode1_scores(b)
        assert np.isnan(s).any() and (s == -1.0).sum() == (b.status != 0).sum()


def test_pick_best_by_hand():
    nan, inf = np.nan, np.inf
    assert pick_best([0.5, 2.0, 2.0, 1.0], 100) == (2.0, 101)
    assert pick_best([nan, -1.0, -2.0, -inf], 0) == (-1.0, -1)
    assert pick_best([nan, -1.0, -0.5, nan], FAR) == (-0.5, FAR + 2)
    assert pick_best([0.0, inf, nan, inf], 0) == (inf, 1)
    assert pick_best([], 0) == (-1.0, -1)


def test_refine_pick_by_hand(built):
    lv = level_metrics
    st = np.zeros(5, np.int32)
    for mode in (1, 2):
        assert refine_pick(st, lv([3, 9, 9, 1, 0]), mode)[:2] == (1, 0)
        assert refine_pick(st, lv([9, 9, 9, 9, 9]), mode)[:2] == (0, 0)
        assert refine_pick(np.array([FAILED, 0, 0, 0, 0], np.int32), lv([3, 9, 9, 1, 0]), mode)[:4] == (-1, 1, 0.0, 0)
        assert refine_pick(np.array([0, FAILED, FAILED, 0, FAILED], np.int32), lv([3, 9, 9, 1, 0]), mode)[:2] == (0, 3)
    m = lv([3, 9, 9, 1, 0]); m[1, 1] = m[2, 0] = np.nan; m[1, 0] = -1.0      # variant 1: NaN opinion below net zero, a NaN score in mode 1
    assert refine_pick(st, m, 1)[:2] == (2, 1)      # (variant 2: NaN emissions are "not above net zero", it scores above 1)
    base = np.array([[-5.0, -np.inf, 1e10, 1.0]] * 3)      # the base scores -inf and nothing else is a candidate: it is the winner
    w = refine_pick(np.array([0, FAILED, FAILED], np.int32), base, 1)
    assert w == (0, 2, -np.inf, 1, -np.inf)
    assert refine_pick(np.zeros(3, np.int32), base, 1)[:2] == (0, 0)      # ... and among equals the lowest
    assert refine_block(3)[:4].tobytes() == np.array([3 * 0x9E3779B1 & 0xFFFFFFFF], "<u4").tobytes()
    assert refine_block(5).view("<u4")[[130, 158]].tolist() == [5, 1] and refine_block(None).view("<u4")[[0, 130, 158]].tolist() == [0xBA5E0000, 7, 5]
