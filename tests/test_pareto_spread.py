"""CPU: the Pareto archive's second capacity rule, "keep spread" (include/eirgrid_hip.h EG_PARETO_KEEP_SPREAD; csrc/eg_pareto.h
k_pareto_spread) — the constant, what the compiler makes of the kernel, the scripts' flag, the validators — and the restatement of the
rule that tests/test_gpu_pareto_spread.py holds the device against: SpreadFront, beside tests/test_pareto.py Front, written from the
header's definition with numpy elementwise operations in the stated order."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_pareto import Front, front, oriented, valid

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP_SPREAD = 0x100


# ---- the definition, restated (imports nothing from the feature) ---------------------------------------------------------------------

def normalised(v):
    """u[i][k] = (v[i][k] - lo_k) / (hi_k - lo_k) where that range is a finite number > 0, else 0.0 — a subtraction and a division."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 4)
    u = np.zeros_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = v.min(0), v.max(0)
        r = hi - lo
    for k in range(4):
        if np.isfinite(r[k]) and r[k] > 0:
            u[:, k] = (v[:, k] - lo[k]) / r[k]
    return u


def dist2(u, p):
    """((e0*e0 + e1*e1) + e2*e2) + e3*e3 of every row of u against the point p, every product and sum rounded on its own."""
    e = u - p
    return ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + e[:, 3] * e[:, 3]


def preference(score, index):
    """place[i] of row i in the order of preference: larger score first (NaN last), then lower index, then earlier row."""
    key = np.where(np.isnan(score), -np.inf, score)
    order = sorted(range(len(key)), key=lambda r: (-key[r], index[r], r))
    place = np.empty(len(key), np.int64)
    place[order] = np.arange(len(key))
    return place


def spread_select(v, score, index, cap):
    """The rows s_0 .. s_{cap-1} of the front whose oriented coordinates are v (rows in list order): farthest-point selection."""
    u, place = normalised(v), preference(np.asarray(score, np.float64), np.asarray(index, np.int64))
    picked = [int(np.argmin(place))]
    chosen = np.zeros(len(u), bool)
    chosen[picked[0]] = True
    mind = dist2(u, u[picked[0]])
    for _ in range(1, cap):
        live = np.where(chosen, -1.0, mind)
        tied = np.nonzero(live == live.max())[0]
        s = int(tied[np.argmin(place[tied])])
        picked.append(s)
        chosen[s] = True
        mind = np.minimum(mind, dist2(u, u[s]))
    return np.array(picked)


class SpreadFront:
    """Front with the capacity rule "keep spread": after a batch front(held u valid(batch)); more than cap points: the cap rows of
    spread_select stay and n_dropped grows by the number removed.  Entries in ascending index."""

    def __init__(self, cap, mask, score):
        self.cap, self.mask, self.score = cap, mask, score      # score: metrics row -> rank score
        self.m = np.zeros((0, 4)); self.index = np.zeros(0, np.int64); self.n_dropped = 0

    def fold(self, metrics, status, first):
        metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 4)
        ok = valid(metrics, status)
        m = np.concatenate([self.m, metrics[ok]])
        idx = np.concatenate([self.index, first + np.nonzero(ok)[0].astype(np.int64)])
        keep = front(m, idx, self.mask)      # (ascending rows: the list order)
        if len(keep) > self.cap:
            s = np.array([self.score(m[p]) for p in keep])
            self.n_dropped += len(keep) - self.cap
            keep = keep[spread_select(oriented(m[keep], self.mask), s, idx[keep], self.cap)]
        keep = keep[np.lexsort((keep, idx[keep]))]
        self.m, self.index = m[keep], idx[keep]
        return self

    def scores(self):
        return np.array([self.score(r) for r in self.m], dtype=np.float64)


def covering_radius(front_metrics, kept_metrics, mask):
    """The largest distance, in the front's normalised coordinates, from a point of the front to its nearest kept point."""
    both = normalised(np.concatenate([oriented(front_metrics, mask), oriented(kept_metrics, mask)]))      # (kept is a subset: the ranges are the front's)
    u, k = both[:len(front_metrics)], both[len(front_metrics):]
    return float(np.sqrt(max(min(dist2(k, p)) for p in u)))


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

def _score(cost_only=False):
    from eirgrid_amd.engine import rank_score
    return lambda row: rank_score(np.ascontiguousarray(row), cost_only)


def test_the_constant(built):
    from eirgrid_amd import _native as N
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert int(re.search(r"#define EG_PARETO_KEEP_SPREAD (0x[0-9a-fA-F]+)", header).group(1), 16) == N.PARETO_KEEP_SPREAD == KEEP_SPREAD


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_spread_kernel_compiles_without_scratch():
    out = "\n".join(kernel_resource_lines())
    lines = [l for l in out.splitlines() if re.search(r"remark: k_pareto_spread(\b|E)", l)]
    assert len(lines) == 1, lines
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", lines[0])
    assert m, lines[0]
    scratch, sspill, vspill, lds = (int(m.group(k)) for k in (1, 2, 3, 4))
    assert scratch == 0 and sspill == 0 and vspill == 0, lines[0]
    assert lds <= 65536, lds


@pytest.mark.parametrize("script", ["pareto_front.py", "breed_front.py", "explore_front.py"])
def test_the_scripts_have_the_flag(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--keep" in out.stdout and "spread" in out.stdout


@pytest.mark.parametrize("validator", ["eg_breed_validate", "eg_explore_validate"])
def test_the_validators_take_the_flag_with_a_rank_score_only(built, validator):
    from eirgrid_amd import _native as N
    from tests.test_plan_search_messages import _validate
    for mode in (1, 2, 0x101, 0x102):
        rc, msg = _validate(validator, mode=mode)
        assert rc == N.EG_OK, (mode, msg)
    for mode in (0x100, 0x103, 0x201):
        rc, msg = _validate(validator, mode=mode)
        assert rc == N.EG_ERR_BAD_ARG and msg.startswith(validator + ": mode " + str(mode)), (mode, msg)


def _line(n, seed):
    from tests.test_gpu_pareto import _antichain
    return _antichain(n, seed)


def test_cap_one_keeps_the_best_score(built):
    m = _line(300, 1)
    ref = SpreadFront(1, 5, _score()).fold(m, np.zeros(300, np.int32), 0)
    s = np.array([_score()(r) for r in m])
    assert ref.index.tolist() == [int(np.argmax(s))] and ref.n_dropped == 299
    same = Front(1, 5, _score()).fold(m, np.zeros(300, np.int32), 0)
    assert same.index.tolist() == ref.index.tolist() and same.m.tobytes() == ref.m.tobytes()


def test_a_front_within_the_cap_is_kept_whole(built):
    m = _line(40, 2)
    for cap in (40, 256):
        ref = SpreadFront(cap, 5, _score()).fold(m[:25], np.zeros(25, np.int32), 0).fold(m[25:], np.zeros(15, np.int32), 25)
        assert ref.n_dropped == 0 and ref.index.tolist() == list(range(40)) and ref.m.tobytes() == m.tobytes()


def test_spread_covers_the_front_better_than_the_best_scores(built):
    n, cap = 3000, 8
    m = _line(n, n + cap)
    ok = np.zeros(n, np.int32)
    spread, best = SpreadFront(cap, 5, _score()).fold(m, ok, 0), Front(cap, 5, _score()).fold(m, ok, 0)
    assert len(spread.index) == len(best.index) == cap and spread.n_dropped == best.n_dropped == n - cap
    r_spread, r_best = covering_radius(m, spread.m, 5), covering_radius(m, best.m, 5)
    print(f"covering radius of {cap} of {n}: spread {r_spread:.4f}, score {r_best:.4f}")
    assert r_spread < r_best
    assert int(best.index[np.argmax(best.scores())]) in spread.index.tolist()      # (s_0: the best score is never dropped)
