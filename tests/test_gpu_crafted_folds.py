"""GPU: the four device reductions that decide what a run keeps, exports and trains on — the best_result fold (k_fold_best / fold_windows),
the top-K archive (csrc/eg_topk.h), the update's best pick (k_pick_best) and the refinement's pick (csrc/eg_refine_many.h k_refine_pick_many) — on
crafted batches through the test hooks eg_debug_load_batch / _fold_last_batch / _pick_best / _refine_pick: ties, staircases in which every
result takes over, NaN and infinities, action logs on the key's padding edges, maxima on row, wave and stride boundaries, global
indices across 2^32.  Every comparison is exact — indices, score bits, metrics bytes, the n_draws tag and the tagged lists of every kept
record — against the oracle's fold, the Archive of tests/test_gpu_top_k.py and the restatements of tests/test_crafted_folds.py."""
import functools

import numpy as np
import pytest

from eirgrid_amd import _native as N
from tests.test_crafted_folds import (FAILED, FAR, FOLD_SIZES, TAKEOVER_AT, TOPK_SIZES, batch, chunk_duplicate_batch, equal_score_batch, feed,
                                      fold_cases, identical_batch, key_edge_batch, level_metrics, mode1_scores, pick_best, refine_block,
                                      refine_pick, sized_batch, tag_bytes)
from tests.test_gpu_top_k import RECORD_FIELDS, Archive, assert_archive, assert_same_archive

pytestmark = pytest.mark.gpu


@pytest.fixture
def engine(engine):
    """The session's engine, with every kind of tracking off again for whoever uses it next."""
    yield engine
    engine.track_pareto(0); engine.track_top_k(0); engine.track_best_result(on=False)


def bits(x):
    return np.float64(x).tobytes()


def assert_tagged(rows, r, index, what):
    """Row r is the synthetic record of global index `index`: the tag and the two tagged lists say where it was copied from."""
    run, dfl = tag_bytes(index)
    assert int(rows.n_draws[r]) == index & (2**64 - 1) and rows.status[r] == 0, (what, r, index, int(rows.n_draws[r]))
    assert rows.n_run[r].tolist() == [N.DEBUG_LIST_LEN] + [0] * 25 and rows.n_def[r].tolist() == [N.DEBUG_LIST_LEN] + [0] * 25, (what, r)
    assert rows.run_log[r, :8].tobytes() == run and rows.def_log[r, :8].tobytes() == dfl, (what, r, index)
    assert not rows.run_log[r, 8:].any() and not rows.def_log[r, 8:].any(), (what, r)


# ---- the best_result fold ------------------------------------------------------------------------------------------------------------
FOLD_CASES = fold_cases()


def _record_bytes(rec):
    return b"".join(getattr(rec, f).tobytes() for f in RECORD_FIELDS)


@pytest.mark.parametrize("name", sorted(FOLD_CASES))
def test_best_result_fold_is_the_oracles(engine, name):
    """Both modes; after every batch the held index, the metrics bits and the whole tagged record are the oracle's (oracle.api
    BestResultFold, which tests/test_crafted_folds.py holds against the literal fold), and a batch in which nothing takes over leaves the
    record byte for byte.  The cases: every size at a window or tile edge of fold_windows, random and with take-overs exactly at positions
    0, 1023, 1024, 8191, 8192; a rising staircase of 2 049 in which every result takes over (1 024 restarts of a window), a falling one,
    equal metrics (impact 0.0), failed episodes at position 0 and throughout, three batches of which the second takes nothing over, and NaN
    and +-inf in each of emissions, opinion and cost, above and below net zero, inside the batch and held from position 0."""
    from oracle import api as O
    for cost_only in (False, True):
        engine.track_best_result(cost_only)
        assert engine.fetch_best_result() == (None, None)
        fold = O.BestResultFold(cost_only)
        held = None
        for b, (st, m, first) in enumerate(FOLD_CASES[name]):
            before = fold.winner
            engine._debug_load_batch(m, st, first)
            engine._debug_fold_last_batch(best_result=True)
            fold.feed(st, m, first)
            idx, rec = engine.fetch_best_result()
            print(f"{name} cost_only {cost_only} batch {b}: device {idx} oracle {fold.winner} take-overs {fold.takeovers}")
            assert idx == fold.winner, (name, cost_only, b, idx, fold.winner)
            if idx is None:
                assert rec is None
                continue
            assert rec.metrics[0].tobytes() == fold.best.tobytes(), (name, cost_only, b)
            assert_tagged(rec, 0, idx, (name, cost_only, b))
            if fold.winner == before:
                assert _record_bytes(rec) == held, (name, cost_only, b, "the held record changed")
            else:
                assert rec.metrics[0].tobytes() == np.ascontiguousarray(m[idx - first]).tobytes(), (name, cost_only, b)
            held = _record_bytes(rec)
    if name == "rising staircase":
        assert fold.takeovers == 2049 and idx == FAR + 2048 > 2**32
    if name == "all failed":
        assert idx is None


def test_best_result_fold_takes_over_only_at_the_edges(engine):
    """The positions themselves, not only agreement: with 16 385 results the last take-over is at 8192, with 8192 at 8191, ..."""
    for n in FOLD_SIZES:
        st, m, first = FOLD_CASES[f"take-overs at the edges {n}"][0]
        engine.track_best_result()
        engine._debug_load_batch(m, st, first)
        engine._debug_fold_last_batch(best_result=True)
        assert engine.fetch_best_result()[0] == [p for p in TAKEOVER_AT if p < n][-1], n


# ---- the top-K archive ---------------------------------------------------------------------------------------------------------------
KS = (1, 2, 63, 64)
VARIANTS = [pytest.param(False, False, id="mode1"), pytest.param(False, True, id="mode1-score_list"), pytest.param(True, False, id="mode2")]


@functools.lru_cache(maxsize=None)
def _sized(n, seed):
    b = sized_batch(n, seed)
    for a in vars(b).values():
        a.setflags(write=False)
    return b, mode1_scores(b)


@functools.lru_cache(maxsize=None)
def _made(make):
    """One of the fixed batches of tests/test_crafted_folds.py, made once and left unchanged."""
    b = make()
    for a in vars(b).values():
        a.setflags(write=False)
    return b


def _fold_topk(eng, ref, b, first, use_list, what, scores=None):
    """The batch loaded and folded as behind a training batch; the archive is the restatement's: indices, score bits, every field of every
    record (as eg_fetch_record gave it when the entry entered) and the tags."""
    eng._debug_load_batch(b.metrics, b.status, first, b.n_act, b.act_log, (mode1_scores(b) if scores is None else scores) if use_list else None)
    eng._debug_fold_last_batch(top_k=True, use_score_list=use_list)
    want = feed(ref, eng, b, first)
    got = eng.fetch_top_k()
    assert_archive(got, want, ref.records, what)
    for r, (_, idx) in enumerate(want):
        assert_tagged(got[0], r, idx, what)
    return got


def _start(eng, k, cost_only):
    eng.track_top_k(k, cost_only=cost_only)
    return Archive(k, cost_only)


@pytest.mark.parametrize("cost_only,use_list", VARIANTS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", TOPK_SIZES)
def test_top_k_at_every_size(engine, n, k, cost_only, use_list):
    """Shuffled scores with repeated scenarios, failed episodes and NaN scores, below, at and above the chunk of k_topk_select and with ten
    blocks (640 entries at k = 64: k_topk_merge reduces its list on the way); then a second batch on top of the held entries."""
    ref = _start(engine, k, cost_only)
    first = FAR if n in (1025, 9217) else 50
    for s in range(2):
        b, scores = _sized(n, 1000 * s + n)
        got = _fold_topk(engine, ref, b, first, use_list, (n, k, cost_only, use_list, s), scores)
        first += n + 3
    if n >= 1023:
        assert len(got[2]) == k


@pytest.mark.parametrize("cost_only,use_list", VARIANTS)
@pytest.mark.parametrize("k", KS)
def test_top_k_key_edges_and_a_batch_folded_twice(engine, k, cost_only, use_list):
    """Action totals 0, 1, 7, 8, 9, EG_ACT_CAP - 1 and EG_ACT_CAP under one score: a byte behind the log does not make a scenario, the last
    valid byte and the per-year split of n_act do; the entries are the scenarios' first records, in index order.  Folded again: nothing moves."""
    b, scen = key_edge_batch()
    ref = _start(engine, k, cost_only)
    got = _fold_topk(engine, ref, b, FAR, use_list, ("key edges", k))
    firsts = sorted({s: FAR + scen.index(s) for s in scen}.values())
    assert got[2].tolist() == firsts[:k] and len(firsts) == 19
    again = _fold_topk(engine, ref, b, FAR, use_list, ("key edges, twice", k))
    assert_same_archive(got, again, "folded twice")
    assert again[0].n_chunks.tobytes() == got[0].n_chunks.tobytes()


@pytest.mark.parametrize("cost_only,use_list", VARIANTS)
@pytest.mark.parametrize("k", KS)
def test_top_k_equal_scores_identical_records_and_repeated_chunks(engine, k, cost_only, use_list):
    b = _made(equal_score_batch)      # one score, distinct identities: the k lowest successful indices, across chunks
    got = _fold_topk(engine, _start(engine, k, cost_only), b, 10, use_list, ("equal scores", k))
    assert got[2].tolist() == (10 + np.flatnonzero(b.status == 0)[:k]).tolist()
    got = _fold_topk(engine, _start(engine, k, cost_only), _made(identical_batch), FAR, use_list, ("identical", k))
    assert got[2].tolist() == [FAR + 1]      # one scenario, at its lowest successful index
    d = _made(chunk_duplicate_batch)      # chunk 8 repeats chunk 0 and both are on top: every entry is chunk 0's
    got = _fold_topk(engine, _start(engine, k, cost_only), d, 0, use_list, ("chunks 0 and 8", k))
    assert len(got[2]) == k and (got[2] < 1024).all()
    got = _fold_topk(engine, _start(engine, k, cost_only), d, 2**32 - 8000, use_list, ("chunks 0 and 8 across 2^32", k))      # chunk 8 is beyond 2^32
    assert (got[2] < 2**32 - 8000 + 1024).all()


@pytest.mark.parametrize("cost_only,use_list", VARIANTS)
@pytest.mark.parametrize("k", KS)
def test_top_k_ties_with_the_kth_entry(engine, k, cost_only, use_list):
    """A full archive; then entries that tie its k-th score: at a higher global index they stay out (so does a repeat of the k-th scenario
    itself and a lower score), at a lower one they enter and the old k-th entry leaves."""
    ref = _start(engine, k, cost_only)
    level = np.random.default_rng(k).permutation(k + 3) * 2.0 + 10.0
    got = _fold_topk(engine, ref, batch(level_metrics(level)), 1000, use_list, ("fill", k))
    kth_level, kth_index = sorted(level)[-k], int(got[2][-1])
    assert len(got[2]) == k and level[kth_index - 1000] == kth_level
    late = batch(np.concatenate([level_metrics([kth_level], reliability=0.25), level_metrics([kth_level - 1.0]), level_metrics([kth_level])]))
    after = _fold_topk(engine, ref, late, 5000, use_list, ("a tie at a higher index", k))
    assert_same_archive(got, after, "a tie at a higher index")
    early = batch(level_metrics([kth_level, kth_level - 1.0], reliability=0.75))
    moved = _fold_topk(engine, ref, early, 10, use_list, ("a tie at a lower index", k))
    assert int(moved[2][-1]) == 10 and kth_index not in moved[2].tolist() and moved[2][:-1].tolist() == got[2][:-1].tolist()


@pytest.mark.parametrize("cost_only,use_list", VARIANTS)
@pytest.mark.parametrize("k", KS)
def test_top_k_scenarios_arriving_later_at_lower_indices(engine, k, cost_only, use_list):
    """The same batch at 5000.. and then at 100..: every entry, its index and its record (the tag shows it) move to the lower index; a third
    time at a higher index nothing moves."""
    b, scores = _sized(1025, 1025)
    ref = _start(engine, k, cost_only)
    high = _fold_topk(engine, ref, b, 5000, use_list, ("high", k), scores)
    low = _fold_topk(engine, ref, b, 100, use_list, ("low", k), scores)
    assert (low[2] == high[2] - 4900).all() and low[1].tobytes() == high[1].tobytes()
    again = _fold_topk(engine, ref, b, FAR, use_list, ("far", k), scores)
    assert_same_archive(low, again, "a later copy at higher indices")


@pytest.mark.parametrize("cost_only,use_list", VARIANTS)
def test_top_k_failed_nan_and_minus_infinity_never_enter(engine, cost_only, use_list):
    """include/eirgrid_hip.h "failures": status != EG_EP_OK, a NaN score, a score of -inf.  (Mode 2 reads the cost alone: there the same
    records score like any other and enter.)"""
    inf, nan = np.inf, np.nan
    m = level_metrics(np.arange(6.0))
    m[1] = (-5.0, -inf, 1e10, 1.0)       # mode 1: -inf
    m[2] = (-5.0, nan, 1e10, 1.0)        # mode 1: NaN
    m[3] = (-5.0, inf, 1e10, 1.0)        # mode 1: +inf, the best there is
    m[4] = (inf, 0.5, 6e10, 1.0)         # emissions +inf: score 0 in mode 1
    b = batch(m, status=np.array([0, 0, 0, 0, 0, FAILED], np.int32))
    for k in (1, 8):
        got = _fold_topk(engine, _start(engine, k, cost_only), b, FAR, use_list, ("specials", k))
        want = ([1, 2, 3, 4, 0] if cost_only else [3, 0, 4])[:k]
        assert (got[2] - FAR).tolist() == want, got[2] - FAR
    ref = _start(engine, 4, cost_only)      # nothing but failures: the archive stays empty, and stays so under a second batch
    dead = batch(np.repeat(m[1:3], 600, axis=0), status=np.where(np.arange(1200) % 2 == 0, FAILED, 0).astype(np.int32))
    got = _fold_topk(engine, ref, dead, 0, use_list, "nothing enters")
    assert len(got[2]) == (0 if not cost_only else 2)


# ---- the update's best pick ----------------------------------------------------------------------------------------------------------
def _pick(eng, scores, first, what):
    """score_list as the statistics epilogue leaves it: score_metrics (>= 0) of an episode that ended EG_EP_OK, -1.0 of a failed one.
    k_pick_best picks the FIRST maximum among the scores above its -1.0 start — a NaN, -1.0 itself, anything below it and -inf are never
    picked — and answers score -1.0, index -1 when there is none; metrics and the four lists of the candidate are the winner's."""
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    n = len(scores)
    m = level_metrics(np.arange(n) % 97, reliability=np.arange(n) / 65536.0)
    eng._debug_load_batch(m, np.where(scores == -1.0, FAILED, 0).astype(np.int32), first, score_list=scores)
    c = eng._debug_pick_best()
    score, index = pick_best(scores, first)
    assert (bits(c.score), c.index) == (bits(score), index), (what, c.score, c.index, score, index)
    run, dfl = (b"", b"") if index < 0 else tag_bytes(index)
    assert bytes(c.metrics) == (m[index - first].tobytes() if index >= 0 else bytes(32)), what
    assert list(c.n_run) == list(c.n_def) == [len(run)] + [0] * 25, what
    assert bytes(c.run_log) == run + bytes(N.RUN_CAP - len(run)) and bytes(c.def_log) == dfl + bytes(N.DEF_CAP - len(dfl)), what
    return c.index


@pytest.mark.parametrize("n", (1, 1023, 1024, 1025, 4097))
def test_pick_best_is_the_first_maximum(engine, n):
    rng = np.random.default_rng(n)
    s = rng.uniform(0.0, 1.9, n)
    s[rng.uniform(size=n) < 0.1] = -1.0
    s[rng.uniform(size=n) < 0.05] = np.nan
    _pick(engine, s, FAR, "random")
    s[:] = np.where(np.isnan(s) | (s < 0), s, np.round(s * 4) / 4)      # a handful of values: maxima everywhere
    _pick(engine, s, 3, "quantised")
    top = s.copy(); top[n - 1] = 2.5
    assert _pick(engine, top, FAR, "the maximum at the last index") == FAR + n - 1
    for i, j in ((5, 1029), (511, 512), (0, 1023), (1023, 1024), (1000, 3048), (4095, 4096), (63, 64)):      # the same thread (i + 1024 t), the tree's halves
        if j < n:
            tie = s.copy(); tie[[i, j]] = 2.25
            assert _pick(engine, tie, FAR, ("equal maxima", i, j)) == FAR + i
            tie[max(i - 1, 0)] = np.nan; tie[j - 1 if j - 1 != i else j] = np.inf if j - 1 != i else 2.25
            _pick(engine, tie, 0, ("equal maxima beside NaN and inf", i, j))


def test_pick_best_never_picks_what_is_not_above_minus_one(engine):
    nan, inf = np.nan, np.inf
    for n in (1, 1025, 4097):
        for fill in (nan, -1.0, -2.0, -inf):
            assert _pick(engine, np.full(n, fill), FAR, ("nothing to pick", n, fill)) == -1
        mixed = np.array([nan, -1.0, -2.0, -inf])[np.arange(n) % 4]
        assert _pick(engine, mixed, 0, ("nothing to pick, mixed", n)) == -1
        one = mixed.copy(); one[n - 1] = -0.999
        assert _pick(engine, one, FAR, ("just above -1.0", n)) == FAR + n - 1
        zero = mixed.copy(); zero[n // 2] = 0.0; zero[n - 1] = -0.0
        assert _pick(engine, zero, 0, ("0.0 and -0.0 are one maximum", n)) == min(n // 2, n - 1)


# ---- the refinement's pick -----------------------------------------------------------------------------------------------------------
REFINE_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, N.REFINE_MAX_VARIANTS)


def _refine(eng, status, metrics, mode, what, first=0):
    """The step entry and the base block against the definition restated (tests/test_crafted_folds.py refine_pick): winner, n_failed, the
    winner's packed edit, score bits, metrics, the list totals of its block, what the base scored — and the base block: the winner's block
    when the winner is a variant above 0, untouched otherwise."""
    status = np.ascontiguousarray(status, dtype=np.int32)
    n = len(status)
    eng._debug_load_batch(metrics, status, first)
    e, base = eng._debug_refine_pick(mode)
    winner, n_failed, score, base_ok, base_score = refine_pick(status, metrics, mode)
    assert (e.winner, e.n_failed, e.base_ok, e.n) == (winner, n_failed, base_ok, n), (what, e.winner, e.n_failed, e.base_ok, e.n, winner, n_failed, base_ok)
    w = max(winner, 0)
    assert list(e.edit) == [w, ~w & 0xFFFFFFFF], (what, list(e.edit))
    assert bits(e.score) == bits(score), (what, e.score, score)
    assert bytes(e.metrics) == np.ascontiguousarray(metrics[w]).tobytes() and bytes(e.base_metrics) == np.ascontiguousarray(metrics[0]).tobytes(), what
    assert (e.off26, e.offd26) == (w % 4097, (w // 3) % 4097), (what, e.off26, e.offd26)
    assert (np.isnan(e.base_score) and np.isnan(base_score)) or bits(e.base_score) == bits(base_score), (what, e.base_score, base_score)
    assert base.tobytes() == refine_block(winner if winner > 0 else None).tobytes(), (what, "the base block")
    return e.winner


def _positions(n):
    """Lanes 15/16, 31/32, 47/48 (the DPP rows), 63/64 (the wave), wave 15's last lane and the stride's edge, in every trip, and n - 1."""
    if n > 4096:      # (a batch of this size a few times only)
        return [1023, 1024 + 16, 5 * 1024 + 47, 15 * 1024 + 32, n - 1 - 1024, n - 1]
    p = {q + t for q in (15, 16, 31, 32, 47, 48, 63, 64, 1023) for t in range(0, n, 1024)} | {1024, n - 1, n - 1 - 1024}
    return sorted(q for q in p if 0 < q < n)


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("n", REFINE_SIZES)
def test_refine_pick_at_every_size(engine, n, mode):
    rng = np.random.default_rng(n + mode)
    ok = np.zeros(n, np.int32)
    level = rng.integers(0, 50, n).astype(np.float64)      # few values: ties everywhere
    st = np.where(rng.uniform(size=n) < 0.2, FAILED, 0).astype(np.int32); st[0] = 0
    m = level_metrics(level)
    m[rng.uniform(size=n) < 0.05, :2] = (-1.0, np.nan)      # NaN scores in mode 1
    m[0] = level_metrics([level[0]])[0]
    _refine(engine, st, m, mode, ("random", n, mode), FAR)
    assert _refine(engine, ok, level_metrics(np.full(n, 7.0)), mode, ("all equal", n, mode)) == 0      # ... and the base block is untouched
    for p in _positions(n):
        single = np.full(n, 3.0); single[p] = 4.0
        assert _refine(engine, ok, level_metrics(single), mode, ("a single maximum", n, p)) == p


@pytest.mark.parametrize("mode", (1, 2))
def test_refine_pick_ties_go_to_the_lowest_variant(engine, mode):
    n = 3000
    ok = np.zeros(n, np.int32)
    for j in (1, 15, 63, 64, 1000, 1023, 1500):
        for d in (1, 64, 1024):
            level = np.full(n, 3.0); level[[j, j + d]] = 9.0
            assert _refine(engine, ok, level_metrics(level), mode, ("equal maxima", j, d)) == j
            level[0] = 9.0      # the base ties as well: it stays
            assert _refine(engine, ok, level_metrics(level), mode, ("equal maxima and the base", j, d)) == 0


@pytest.mark.parametrize("mode", (1, 2))
def test_refine_pick_failures(engine, mode):
    nan = np.nan
    for n in (1, 65, 1025, 2049):
        level = np.arange(n, dtype=np.float64)
        st = np.zeros(n, np.int32); st[0] = FAILED
        assert _refine(engine, st, level_metrics(level), mode, ("base failed", n)) == -1      # nothing is copied
        st = np.full(n, FAILED, np.int32); st[0] = 0
        m = level_metrics(level)
        m[2::2] = (-1.0, nan, nan, 1.0)      # mode 1: a NaN score.  (Mode 2 has none: a NaN cost is "not above the acceptable cost", score 2.0)
        assert _refine(engine, st, m, mode, ("only the base is a candidate", n)) == 0
        st = np.zeros(n, np.int32)
        assert _refine(engine, st, m, mode, ("NaN or OK", n)) == ((n - 1 if n % 2 == 0 or n == 1 else n - 2) if mode == 1 else min(2, n - 1))
        if n > 1024:      # failures in the partial last trip, and nowhere else
            st = np.zeros(n, np.int32); st[1024 * ((n - 1) // 1024):] = FAILED
            e = _refine(engine, st, level_metrics(level), mode, ("failures in the last trip", n))
            assert e == 1024 * ((n - 1) // 1024) - 1
    m = level_metrics(np.arange(70.0)); m[0] = (-1.0, nan, nan, 1.0)
    assert _refine(engine, np.zeros(70, np.int32), m, mode, "the base scores NaN") == (-1 if mode == 1 else 0)


def test_refine_pick_a_base_that_scores_minus_infinity(engine):
    """rm::score is -inf when opinion is -inf at or below net zero.  Such a base is a candidate (its score is not NaN): when every other
    variant failed it is the winner, variant 0 — not the clamp's variant n - 1, whose block would be copied over the base."""
    low = np.array([-5.0, -np.inf, 1e10, 1.0])
    for n in (2, 64, 65, 1025, 2049):
        st = np.full(n, FAILED, np.int32); st[0] = 0
        m = level_metrics(np.arange(n, dtype=np.float64)); m[0] = low
        assert _refine(engine, st, m, 1, ("-inf base, the others failed", n)) == 0
        st[n - 1] = 0; m[n - 1] = low      # another -inf candidate: the lowest of equals
        assert _refine(engine, st, m, 1, ("two -inf candidates", n)) == 0
        m[n - 1] = level_metrics([0.0])[0]      # any finite score beats it
        assert _refine(engine, st, m, 1, ("-inf base and a finite candidate", n)) == n - 1
        m[:] = low; st[:] = 0      # every variant scores -inf
        assert _refine(engine, st, m, 1, ("all -inf", n)) == 0


def test_the_hooks_refuse_a_rank_of_a_group(world):
    from eirgrid_amd.engine import Group
    L = N.lib()
    g = Group(world, devices=(0, 0))
    try:
        h = g.ranks[0].h
        m = np.zeros((1, 4)); st = np.zeros(1, np.int32); buf = np.zeros(N.CANDIDATE_BYTES, np.uint8)
        dp, ip, bp = (m.ctypes.data_as(N.C.POINTER(N.C.c_double)), st.ctypes.data_as(N.C.POINTER(N.C.c_int32)), buf.ctypes.data_as(N.C.POINTER(N.C.c_uint8)))
        for rc in (L.eg_debug_load_batch(h, dp, ip, None, None, None, 1, 0), L.eg_debug_fold_last_batch(h, 1, 0),
                   L.eg_debug_pick_best(h, bp), L.eg_debug_refine_pick(h, 1, bp, bp)):
            assert rc == N.EG_ERR_BAD_ARG and "eg_group" in L.eg_last_error().decode(), L.eg_last_error()
    finally:
        g.close()
