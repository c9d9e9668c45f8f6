"""CPU: plan streams (include/eirgrid_hip.h eg_plan_streams_set; csrc/eg_streams.cpp) without a device — what the validator refuses and
how it says so, the struct through the binding, and the properties of engine.ensemble_reduce, the restatement the GPU tests hold
k_ensemble_commit to bit for bit."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from eirgrid_amd import _native as N
from eirgrid_amd.engine import ensemble_reduce, rank_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVERFLOW, NO_LOCATION, INFEASIBLE = N.EG_EP_OK, N.EG_EP_OVERFLOW, N.EG_EP_NO_LOCATION, N.EG_EP_INFEASIBLE


def _bits(x):
    return struct.pack("<d", float(x))


def _row(net, opinion, cost, emissions=0.0):
    return [net, opinion, cost, emissions]


def test_struct_constant_and_header_agree(built):
    assert C.sizeof(N.EgEnsembleRow) == 128
    f = N.EgEnsembleRow
    assert (f.nominal.offset, f.committed.offset, f.score_min.offset, f.score_max.offset, f.score_sum.offset) == (0, 32, 64, 72, 80)
    assert (f.n_ok.offset, f.n_infeasible.offset, f.n_failed.offset, f.worst_stream.offset, f.status.offset, f.pad.offset) == (88, 92, 96, 100, 104, 108)
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert int(re.search(r"#define EG_STREAMS_MAX (\d+)", header).group(1)) == N.STREAMS_MAX == 64


@pytest.mark.parametrize("args, expect", [
    ((65, 1, 1), "n_streams = 65 (0..64; 0 or 1 clears)"),
    ((-1, 1, 1), "n_streams = -1 (0..64; 0 or 1 clears)"),
    ((4, 0, 1), "tail = 0 (1..n_streams = 4)"),
    ((4, 5, 1), "tail = 5 (1..n_streams = 4)"),
    ((64, 65, 2), "tail = 65 (1..n_streams = 64)"),
    ((4, 4, 0), "mode 0 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ((4, 1, 3), "mode 3 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
    ((2, 2, 0x101), "mode 257 is neither 1 (optimization_mode None) nor 2 (cost_only)"),
])
def test_validate_names_what_is_wrong(built, args, expect):
    L = N.lib()
    assert L.eg_plan_streams_validate(*args) == N.EG_ERR_BAD_ARG
    assert L.eg_last_error().decode() == "eg_plan_streams_validate: " + expect


def test_validate_accepts_the_range_and_the_clearing_forms(built):
    L = N.lib()
    for args in ((0, 0, 0), (1, 7, 9), (2, 1, 1), (2, 2, 2), (64, 64, 1), (64, 1, 2), (3, 2, 1)):      # (0 or 1: tail and mode are not read)
        assert L.eg_plan_streams_validate(*args) == N.EG_OK, args


def test_the_entry_points_refuse_a_null_context_before_any_device(built):
    L = N.lib()
    assert L.eg_plan_streams_set(None, 4, 4, 1) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_plan_streams_set: bad argument"
    assert L.eg_last_batch_streams(None, None, None) == N.EG_ERR_BAD_ARG and L.eg_last_error().decode() == "eg_last_batch_streams: bad argument"
    rows = (N.EgEnsembleRow * 1)()
    assert L.eg_fetch_plan_ensemble(None, rows) == N.EG_ERR_BAD_ARG and L.eg_fetch_plan_streams(None, None, None) == N.EG_ERR_BAD_ARG
    assert L.eg_debug_ensemble_keep(None, 0) == N.EG_ERR_BAD_ARG and L.eg_debug_ensemble_commit(None, 2, 1, 1) == N.EG_ERR_BAD_ARG


# ---------------------------------------------------------------- ensemble_reduce
# five streams with five different scores in mode None: the net-zero branch, the opinion moving the score
ROWS = np.array([_row(-5.0, 0.50, 6e10), _row(-7.0, 0.30, 6e10), _row(-1.0, 0.90, 6e10), _row(-2.0, 0.10, 6e10), _row(-3.0, 0.70, 6e10)])


def test_tail_one_is_the_worst_streams_row_bitwise(built):
    scores = [rank_score(r) for r in ROWS]
    assert len(set(scores)) == 5
    worst = int(np.argmin(scores))
    got = ensemble_reduce(ROWS, [OK] * 5, 1)
    assert got["worst_stream"] == worst == 3 and got["committed"].tobytes() == ROWS[worst].tobytes()
    assert got["nominal"].tobytes() == ROWS[0].tobytes()
    assert got["score_min"] == min(scores) and got["score_max"] == max(scores)
    total = scores[0]
    for s in scores[1:]:
        total = total + s
    assert _bits(got["score_sum"]) == _bits(total)
    assert (got["n_ok"], got["n_infeasible"], got["n_failed"], got["status"]) == (5, 0, 0, OK)
    # a negative zero survives tail = 1 (the sum starts from the stream's own value, and x / 1.0 is x)
    neg = ROWS.copy(); neg[worst, 3] = -0.0
    assert ensemble_reduce(neg, [OK] * 5, 1)["committed"].tobytes() == neg[worst].tobytes()


def test_tail_r_of_equal_rows_is_the_row(built):
    for R in (2, 3, 4, 64):
        m = np.tile(np.array(_row(-123.456, 0.1, 7.7e10, 1e-3)), (R, 1))
        got = ensemble_reduce(m, [OK] * R, R)
        if R in (2, 4):      # (x + x, and ((x + x) + x) + x, whose one tie rounds to the even 4 x: exact, as the division is)
            assert got["committed"].tobytes() == m[0].tobytes(), R
        assert np.allclose(got["committed"], m[0], rtol=R * np.finfo(float).eps, atol=0.0)      # (R - 1 roundings of at most half an ulp each, and the division's)
        assert got["worst_stream"] == 0 and got["score_min"] == got["score_max"], R      # (equal scores: the tie goes to stream 0)


def test_the_tail_adds_the_selected_streams_in_ascending_stream_order(built):
    scores = [rank_score(r) for r in ROWS]
    order = sorted(range(5), key=lambda r: (scores[r], r))
    for tail in (2, 3, 5):
        chosen = sorted(order[:tail])
        want = []
        for i in range(4):
            c = ROWS[chosen[0], i]
            for r in chosen[1:]:
                c = c + ROWS[r, i]
            want.append(c / np.float64(tail))
        assert ensemble_reduce(ROWS, [OK] * 5, tail)["committed"].tobytes() == np.array(want).tobytes(), tail


def test_a_nan_score_ranks_before_every_number(built):
    m = ROWS.copy()
    m[4, 1] = np.nan      # the opinion: the score of stream 4 is NaN
    assert rank_score(m[4]) != rank_score(m[4])
    got = ensemble_reduce(m, [OK] * 5, 1)
    assert got["worst_stream"] == 4 and got["committed"].tobytes() == m[4].tobytes()
    assert got["score_sum"] != got["score_sum"] and got["score_min"] == rank_score(m[3]) and got["score_max"] == rank_score(m[2])
    m[1, 1] = np.nan      # two NaN scores: the lower stream first
    assert ensemble_reduce(m, [OK] * 5, 1)["worst_stream"] == 1
    got = ensemble_reduce(m, [OK] * 5, 2)      # both NaN streams are the tail
    assert np.isnan(got["committed"][1]) and _bits(got["committed"][0]) == _bits((m[1, 0] + m[4, 0]) / 2.0)
    m[:, 1] = np.nan      # every score NaN: min and max are NaN
    got = ensemble_reduce(m, [OK] * 5, 5)
    assert got["worst_stream"] == 0 and got["score_min"] != got["score_min"] and got["score_max"] != got["score_max"]
    # -inf is a number: it ranks behind a NaN and before everything else
    m = ROWS.copy(); m[2, 1] = -np.inf; m[3, 1] = np.nan
    assert rank_score(m[2]) == -np.inf
    got = ensemble_reduce(m, [OK] * 5, 2)
    assert got["worst_stream"] == 3 and got["score_min"] == -np.inf and _bits(got["committed"][0]) == _bits((m[2, 0] + m[3, 0]) / 2.0)


def test_a_tie_goes_to_the_lower_stream(built):
    m = ROWS.copy()
    m[4] = m[1]; m[4, 3] = 99.0      # streams 1 and 4: equal scores (the emissions column does not enter the score), different rows
    assert rank_score(m[1]) == rank_score(m[4]) < min(rank_score(m[r]) for r in (0, 2))
    m[3] = ROWS[2]      # (take the old worst out of the way)
    got = ensemble_reduce(m, [OK] * 5, 1)
    assert got["worst_stream"] == 1 and got["committed"].tobytes() == m[1].tobytes()
    swapped = m.copy(); swapped[[1, 4]] = swapped[[4, 1]]
    assert ensemble_reduce(swapped, [OK] * 5, 1)["committed"].tobytes() == swapped[1].tobytes()


def test_the_status_rule(built):
    assert ensemble_reduce(ROWS, [OK, OK, INFEASIBLE, OK, OK], 5)["status"] == INFEASIBLE
    got = ensemble_reduce(ROWS, [OK, OK, INFEASIBLE, OK, OVERFLOW], 5)
    assert (got["status"], got["n_ok"], got["n_infeasible"], got["n_failed"]) == (INFEASIBLE, 3, 1, 1)      # the lowest stream that is not OK
    got = ensemble_reduce(ROWS, [OK, NO_LOCATION, INFEASIBLE, OK, OVERFLOW], 1)
    assert (got["status"], got["n_ok"], got["n_infeasible"], got["n_failed"]) == (NO_LOCATION, 2, 1, 2)
    got = ensemble_reduce(ROWS, [OVERFLOW] * 5, 2)
    assert (got["status"], got["n_ok"], got["n_infeasible"], got["n_failed"]) == (OVERFLOW, 0, 0, 5)
    # the order covers every stream, whatever its status: the metrics are reduced all the same
    assert got["committed"].tobytes() == ensemble_reduce(ROWS, [OK] * 5, 2)["committed"].tobytes()


def test_the_cost_only_score_orders_the_streams_by_cost(built):
    m = ROWS.copy(); m[:, 2] = [6e10, 9e10, 5e10, 7e10, 8e10]      # stream 2 below the acceptable cost: score 2.0
    got = ensemble_reduce(m, [OK] * 5, 1, cost_only=True)
    assert got["worst_stream"] == 1 and got["score_max"] == 2.0 and got["committed"].tobytes() == m[1].tobytes()


def test_arguments_are_checked(built):
    for bad in (lambda: ensemble_reduce(ROWS, [OK] * 4, 1), lambda: ensemble_reduce(ROWS, [OK] * 5, 0), lambda: ensemble_reduce(ROWS, [OK] * 5, 6),
                lambda: ensemble_reduce(ROWS[:, :3], [OK] * 5, 1)):
        with pytest.raises(ValueError):
            bad()
