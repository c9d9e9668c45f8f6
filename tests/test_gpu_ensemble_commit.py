"""GPU: k_ensemble_keep and k_ensemble_commit (csrc/eg_ensemble.h) over crafted records, through the two hooks eg_debug_ensemble_keep /
eg_debug_ensemble_commit: the committed records and the eg_ensemble_rows equal engine.ensemble_reduce bit for bit, for R = 2, 3 (idle
lanes), 63 (one idle lane) and 64 (a full wave), tail = 1, 2 and R, n = 1, 65 (a wave short of a block's multiple) and 1025 (a block's
tail).  The crafted streams hold equal scores, -0.0 against +0.0, a NaN metric, a -inf score, EG_EP_INFEASIBLE in stream 2 with
EG_EP_OVERFLOW in stream 5, and a variant that fails in every stream.

A batch's variants repeat N_PATTERNS crafted patterns (variant j holds pattern 7 j mod N_PATTERNS), so the restatement runs once per
pattern and (R, tail, mode) and every size shares it.  The NaNs are np.nan carried through additions and one division, never made by
the arithmetic (inf - inf has another sign on the host than on the device); the -inf and the NaN sit in patterns of their own."""
import dataclasses
import functools

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ensemble_reduce, rank_score

pytestmark = pytest.mark.gpu

OK, OVERFLOW, NO_LOCATION, INFEASIBLE = N.EG_EP_OK, N.EG_EP_OVERFLOW, N.EG_EP_NO_LOCATION, N.EG_EP_INFEASIBLE
N_PATTERNS = 23
FIRST = 40


@functools.lru_cache(maxsize=None)
def _patterns(R):
    """(metrics [N_PATTERNS, R, 4], status [N_PATTERNS, R]): pattern p is one variant's R streams"""
    rng = np.random.default_rng(1000 + R)
    m = np.empty((N_PATTERNS, R, 4))
    m[:, :, 0] = -rng.integers(0, 50000, (N_PATTERNS, R)).astype(np.float64)                 # net emissions at or below zero: the score reads cost and opinion
    m[:, :, 1] = rng.choice(np.array([0.125, 0.25, 0.5, 0.625, 0.75]), (N_PATTERNS, R))      # few opinions: equal scores are common
    m[:, :, 2] = rng.choice(np.array([4e10, 6e10, 6e10, 1.3e11, 4.5e11]), (N_PATTERNS, R))   # below, above and beyond eight times the acceptable cost
    m[:, :, 3] = rng.normal(0.0, 1e4, (N_PATTERNS, R)).round(3)
    st = np.zeros((N_PATTERNS, R), np.int32)
    above = rng.random((N_PATTERNS, R)) < 0.15      # some streams above net zero: the score's other branch
    m[:, :, 0][above] = rng.integers(1, 2000000, int(above.sum())).astype(np.float64)
    st[rng.random((N_PATTERNS, R)) < 0.08] = OVERFLOW
    m[:7, :, 0] = -np.arange(1.0, R + 1.0)[None, :] * np.arange(1.0, 8.0)[:, None]; st[:7] = OK      # the named patterns start clean
    # 0: streams 0 and R-1 share the lowest score, with different rows: the tie goes to stream 0
    m[0, :, 1] = 0.75; m[0, :, 2] = 6e10; m[0, 0, 1] = m[0, R - 1, 1] = 0.125
    # 1: -0.0 against +0.0, in a column the score reads (as a sign only) and in one it does not
    m[1, :, 0] = np.where(np.arange(R) % 2 == 0, -0.0, 0.0); m[1, :, 3] = np.where(np.arange(R) % 3 == 0, 0.0, -0.0); m[1, :, 1] = 0.5; m[1, 1, 1] = 0.25; m[1, :, 2] = 6e10
    # 2: a NaN metric in one stream (its score is NaN: the worst stream)
    m[2, R - 1, 1] = np.nan
    # 3: a -inf score in one stream
    m[3, 1, 1] = -np.inf
    # 4: EG_EP_INFEASIBLE in stream 2 with EG_EP_OVERFLOW in stream 5 (as far as R goes): the committed status is stream 2's
    if R > 2:
        st[4, 2] = INFEASIBLE
    if R > 5:
        st[4, 5] = OVERFLOW
    # 5: the variant fails in every stream, not everywhere the same way
    st[5] = np.where(np.arange(R) % 4 == 1, OVERFLOW, NO_LOCATION)
    # 6: every stream the same row
    m[6] = m[6, 0]
    return m, st


@functools.lru_cache(maxsize=None)
def _reduced(R, tail, cost_only):
    m, st = _patterns(R)
    return [ensemble_reduce(m[p], st[p], tail, cost_only) for p in range(N_PATTERNS)]


def _batch(R, n):
    m, st = _patterns(R)
    which = (7 * np.arange(n)) % N_PATTERNS
    return which, np.ascontiguousarray(m[which].transpose(1, 0, 2)), np.ascontiguousarray(st[which].T)      # [R, n, 4], [R, n]


def _run(engine, R, tail, n, cost_only=False):
    which, metrics, status = _batch(R, n)
    for r in range(R - 1, -1, -1):      # the passes' order: stream 0's records are the ones left
        engine._debug_load_batch(metrics[r], status[r], FIRST)
        engine._debug_ensemble_keep(r)
    before = engine.fetch(n)
    assert engine.last_batch_streams()[0] == 0      # (a crafted batch runs no passes)
    engine._debug_ensemble_commit(R, tail, cost_only)
    assert engine.last_batch_streams() == (R, tail, cost_only)
    after, rows, (kept_m, kept_st) = engine.fetch(n), engine.fetch_ensemble(), engine.fetch_streams()
    assert kept_m.tobytes() == metrics.tobytes() and kept_st.tobytes() == status.tobytes()      # what k_ensemble_keep copied
    want = [_reduced(R, tail, cost_only)[p] for p in which]
    assert after.metrics.tobytes() == np.array([w["committed"] for w in want]).tobytes()
    assert after.status.tolist() == [w["status"] for w in want]
    for f in dataclasses.fields(after):      # every byte outside metrics and status: what eg_debug_load_batch put there
        if f.name not in ("metrics", "status"):
            assert getattr(after, f.name).tobytes() == getattr(before, f.name).tobytes(), f.name
    assert after.n_draws.tolist() == list(range(FIRST, FIRST + n))      # (the tag of a crafted record)
    for name in ("nominal", "committed"):
        assert getattr(rows, name).tobytes() == np.array([w[name] for w in want]).tobytes(), name
    for name in ("score_min", "score_max", "score_sum"):
        assert getattr(rows, name).tobytes() == np.array([w[name] for w in want], np.float64).tobytes(), name
    for name in ("n_ok", "n_infeasible", "n_failed", "worst_stream", "status"):
        assert getattr(rows, name).tolist() == [w[name] for w in want], name
    return which, want, after


@pytest.mark.parametrize("n", [1, 65, 1025])
@pytest.mark.parametrize("tail", [1, 2, "R"])
@pytest.mark.parametrize("R", [2, 3, 63, 64])
def test_committed_records_and_rows_equal_the_restatement(engine, R, tail, n):
    _run(engine, R, R if tail == "R" else tail, n)


def test_the_cost_only_score(engine):
    _run(engine, 3, 2, 65, cost_only=True)
    _run(engine, 64, 1, 5, cost_only=True)


@pytest.mark.parametrize("R", [3, 64])
def test_the_crafted_patterns_do_what_they_are_there_for(engine, R):
    m, st = _patterns(R)
    score = lambda p, r: rank_score(m[p, r])
    one, mean = _reduced(R, 1, False), _reduced(R, R, False)
    # 0: equal lowest scores, different rows, the lower stream wins
    assert score(0, 0) == score(0, R - 1) == min(score(0, r) for r in range(R)) and m[0, 0].tobytes() != m[0, R - 1].tobytes()
    assert one[0]["worst_stream"] == 0 and one[0]["committed"].tobytes() == m[0, 0].tobytes()
    # 1: the worst stream holds a zero of either sign, and tail = 1 keeps it
    w = one[1]["worst_stream"]
    assert w == 1 and np.signbit(one[1]["committed"][3]) and not np.signbit(one[1]["committed"][0]) and not np.signbit(mean[1]["committed"][3])
    # 2, 3: the NaN score ranks first and poisons the sum of scores; the -inf score is a number
    assert one[2]["worst_stream"] == R - 1 and np.isnan(one[2]["committed"][1]) and np.isnan(one[2]["score_sum"]) and not np.isnan(one[2]["score_min"])
    assert one[3]["worst_stream"] == 1 and one[3]["score_min"] == -np.inf and mean[3]["committed"][1] == -np.inf
    # 4: stream 2's status, and the counters; 5: a variant that fails everywhere keeps stream 0's failure
    assert one[4]["status"] == INFEASIBLE and (one[4]["n_infeasible"], one[4]["n_failed"]) == (1, 1 if R > 5 else 0)
    assert one[5]["status"] == NO_LOCATION and one[5]["n_ok"] == 0 and one[5]["n_failed"] == R
    which, want, after = _run(engine, R, 1, N_PATTERNS)
    assert sorted(which.tolist()) == list(range(N_PATTERNS))      # every pattern is in a batch of this size


def test_the_hooks_refuse_what_they_cannot_run(engine):
    engine._debug_load_batch(np.zeros((2, 4)), np.zeros(2, np.int32), FIRST)
    for call, expect in ((lambda: engine._debug_ensemble_keep(64), "r = 64 (a stream 0..63)"), (lambda: engine._debug_ensemble_keep(-1), "r = -1"),
                         (lambda: engine._debug_ensemble_commit(65, 1), "n_streams = 65 (1..64)"), (lambda: engine._debug_ensemble_commit(4, 5), "tail = 5 (1..n_streams = 4)"),
                         (lambda: N.check(N.lib().eg_debug_ensemble_commit(engine.h, 2, 1, 3), "eg_debug_ensemble_commit"), "mode 3 is neither")):
        with pytest.raises(N.EirgridError, match="eg_debug_ensemble_(keep|commit): "):
            try:
                call()
            except N.EirgridError as e:
                assert expect in str(e), str(e)
                raise
    # a commit wants slabs 0..R-1 kept for a batch of exactly this size: what an earlier, other crafted batch left in the store does not count
    engine._debug_load_batch(np.zeros((7, 4)), np.zeros(7, np.int32), FIRST)
    engine._debug_ensemble_keep(0); engine._debug_ensemble_keep(1)
    engine._debug_load_batch(np.zeros((2, 4)), np.zeros(2, np.int32), FIRST)
    with pytest.raises(N.EirgridError, match=r"eg_debug_ensemble_keep first \(the store does not hold slabs 0..1 of a batch of 2 records\)"):
        engine._debug_ensemble_commit(2, 1)
    engine._debug_ensemble_keep(1)
    with pytest.raises(N.EirgridError, match="eg_debug_ensemble_keep first"):
        engine._debug_ensemble_commit(2, 1)      # (slab 0 is missing)
    engine._debug_ensemble_keep(0)
    with pytest.raises(N.EirgridError, match="slabs 0..2 of a batch of 2 records"):
        engine._debug_ensemble_commit(3, 1)
    engine._debug_ensemble_commit(2, 1)
    engine._debug_load_batch(np.zeros((2, 4)), np.zeros(2, np.int32), FIRST)
    with pytest.raises(N.EirgridError, match="the last batch ran without plan streams"):
        engine.fetch_ensemble()
    with pytest.raises(N.EirgridError, match="the last batch ran without plan streams"):
        engine.fetch_streams()
