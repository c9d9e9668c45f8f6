"""CPU: the Pareto archive's interface (include/eirgrid_hip.h eg_pareto_track) — the exported symbols, what the compiler makes of the
five kernels (csrc/eg_pareto.h), the user script — and the restatement of its definition that tests/test_gpu_pareto.py holds the device
against, checked here on episodes of the tabled oracle."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "pareto_front.py")
KERNELS = ("k_pareto_filter", "k_pareto_compact", "k_pareto_dominate", "k_pareto_rank", "k_pareto_finalize")
_SIGN = np.array([1.0, -1.0, 1.0, -1.0])      # lower emissions and cost, higher opinion and reliability are better


# ---- the definition, restated (imports nothing from the feature) ---------------------------------------------------------------------

def oriented(metrics, mask):
    """Lower is better in every column; inactive metrics are 0.0 and so equal in every pair."""
    v = np.asarray(metrics, dtype=np.float64).reshape(-1, 4) * _SIGN
    v[:, [i for i in range(4) if not mask >> i & 1]] = 0.0
    return v


def front(metrics, index, mask):
    """Positions of the representatives of F(S): the points no point dominates, each once, at its lowest global index (of two rows with
    the same index the earlier one).  O(n^2), a block of rows against all at a time, a metric at a time."""
    v = oriented(metrics, mask)
    index = np.asarray(index, dtype=np.int64)
    n = len(v)
    pos = np.arange(n)
    keep = np.ones(n, bool)
    for lo in range(0, n, 512):
        hi = min(lo + 512, n)
        le, eq = np.ones((hi - lo, n), bool), np.ones((hi - lo, n), bool)
        for k in range(4):
            le &= v[None, :, k] <= v[lo:hi, None, k]
            eq &= v[None, :, k] == v[lo:hi, None, k]
        ai, ap = index[lo:hi, None], pos[lo:hi, None]
        beaten = le & (~eq | (index[None] < ai) | ((index[None] == ai) & (pos[None] < ap)))
        keep[lo:hi] = ~beaten.any(1)
    return pos[keep]


def valid(metrics, status):
    return (np.asarray(status) == 0) & ~np.isnan(np.asarray(metrics, dtype=np.float64).reshape(-1, 4)).any(1)


class Front:
    """The archive by the streaming rule of the header: after a batch front(held u valid(batch)); more than cap points: the cap with the
    largest rank score stay (NaN last, ties to the lower index) and n_dropped grows by the number removed.  Entries in ascending index."""

    def __init__(self, cap, mask, score):
        self.cap, self.mask, self.score = cap, mask, score      # score: metrics row -> rank score
        self.m = np.zeros((0, 4)); self.index = np.zeros(0, np.int64); self.n_dropped = 0

    def fold(self, metrics, status, first):
        metrics = np.asarray(metrics, dtype=np.float64).reshape(-1, 4)
        ok = valid(metrics, status)
        m = np.concatenate([self.m, metrics[ok]])
        idx = np.concatenate([self.index, first + np.nonzero(ok)[0].astype(np.int64)])
        keep = front(m, idx, self.mask)
        if len(keep) > self.cap:
            s = np.array([self.score(m[p]) for p in keep])
            key = np.where(np.isnan(s), -np.inf, s)
            order = sorted(range(len(keep)), key=lambda r: (-key[r], idx[keep[r]], keep[r]))
            self.n_dropped += len(keep) - self.cap
            keep = keep[np.array(order[:self.cap])]
        keep = keep[np.lexsort((keep, idx[keep]))]
        self.m, self.index = m[keep], idx[keep]
        return self

    def scores(self):
        return np.array([self.score(r) for r in self.m], dtype=np.float64)


SPLIT7 = (0.03, 0.2, 0.21, 0.5, 0.55, 0.9)      # seven uneven parts of a set


def split7(n):
    cuts = [0] + [int(n * f) for f in SPLIT7] + [n]
    return [(a, b) for a, b in zip(cuts, cuts[1:])]


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_pareto_symbols(built):
    from eirgrid_amd import _native as N
    L = N.lib()
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    for name in ("eg_pareto_track", "eg_pareto_fold_last_batch", "eg_fetch_pareto", "eg_debug_pareto_fold"):
        assert hasattr(L, name) and name in N.EXPORTS, name
        assert re.search(rf"\b{name}\(", header), name
    assert int(re.search(r"#define EG_PARETO_MAX (\d+)", header).group(1)) == N.PARETO_MAX == 256


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_pareto_kernels_compile_without_scratch():
    """The five kernels exist for gfx950 in exactly one of eg_rollout.hip's two objects, spill nothing, need no scratch and at most
    64 KB of LDS."""
    out = "\n".join(kernel_resource_lines())
    for name in KERNELS:
        lines = [l for l in out.splitlines() if re.search(rf"remark: {name}(\b|E)", l)]
        assert len(lines) == 1, (name, lines)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", lines[0])
        assert m, lines[0]
        scratch, sspill, vspill, lds = (int(m.group(k)) for k in (1, 2, 3, 4))
        assert scratch == 0 and sspill == 0 and vspill == 0, (name, lines[0])
        assert lds <= 65536, (name, lds)


@pytest.fixture(scope="module")
def oracle_metrics(world, built):
    """The tabled oracle's first 3 000 episodes: synthetic world, a fresh policy each, seed 9001 + i."""
    from eirgrid_amd.engine import HostTables
    from oracle import api as O
    tb = O.OracleTables(HostTables(world), len(world.existing_x))
    m, st = np.zeros((3000, 4)), np.zeros(3000, np.int32)
    for i in range(3000):
        st[i], out = O.run_episode_tabled(tb, O.OracleWeights(), 9001 + i)
        m[i] = list(out.metrics)
    m.setflags(write=False); st.setflags(write=False)
    return m, st


@pytest.mark.parametrize("mask", [15, 5])
def test_restatement_on_oracle_episodes(oracle_metrics, mask):
    """front(front(S)) = front(S); seven uneven parts of S folded in shuffled order give front(S); the front is neither trivial nor
    near the capacity."""
    from oracle import api as O
    m, st = oracle_metrics
    ok = valid(m, st)
    idx = np.arange(len(m), dtype=np.int64)
    mv, iv = m[ok], idx[ok]
    f = front(mv, iv, mask)
    print(f"mask {mask}: {ok.sum()} valid episodes, front of {len(f)} points")
    assert 5 < len(f) < 256
    again = front(mv[f], iv[f], mask)
    assert again.tolist() == list(range(len(f)))
    parts = split7(len(m))
    order = np.random.default_rng(5).permutation(len(parts))
    assert sorted(order.tolist()) != order.tolist()
    arch = Front(256, mask, lambda r: O.score_metrics(r))
    for p in order:
        a, b = parts[p]
        arch.fold(m[a:b], st[a:b], a)
    assert arch.n_dropped == 0
    assert arch.index.tolist() == iv[f].tolist()
    assert arch.m.tobytes() == mv[f].tobytes()


def test_restatement_holds_a_point_once_at_its_lowest_index():
    m = np.array([[1, 0, 5, 0], [1, 9, 5, 9], [0, 0, 6, 0], [2, 0, 6, 0]], dtype=np.float64)
    assert front(m, [7, 3, 4, 5], 5).tolist() == [1, 2]      # rows 0 and 1 are one point under mask 5; row 3 is dominated by row 2
    assert front(m, [7, 3, 4, 5], 15).tolist() == [1, 2]     # opinion and reliability 9 dominate 0
    assert front(m, [7, 3, 4, 5], 1).tolist() == [2]


def test_pareto_front_script_help():
    out = subprocess.run([sys.executable, SCRIPT, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--objectives" in out.stdout and "--cap" in out.stdout
