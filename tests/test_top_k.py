"""CPU: the top-K archive's interface (include/eirgrid_hip.h eg_top_k_track) — the CLI flag and its refusals, the exported symbols,
the host side of the rank score, and what the compiler makes of the three kernels (csrc/eg_topk.h)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "eirgrid_amd", "eirgrid-hip")
WORLD = os.path.join(ROOT, "tests", "golden", "world_v1.json")


def run(*args, timeout=600):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=timeout)


def test_help_lists_top_k(built):
    out = run("--help")
    assert out.returncode == 0
    assert "--top-k <K>" in out.stdout


@pytest.mark.parametrize("value", ["65", "-1", "x", "", "1e1", "3 ", "100", "9999"])
def test_bad_top_k_exits_2_before_any_device(built, tmp_path, value):
    out = run("--world", WORLD, "-n", "4", "-c", str(tmp_path / "ck"), "--top-k", value)
    assert out.returncode == 2, (value, out.stdout, out.stderr)
    assert "error: --top-k" in out.stderr
    assert "World:" not in out.stdout and not (tmp_path / "ck").exists()      # refused at parse time: no world, no device, no files


def test_library_exports_the_top_k_symbols(built):
    from eirgrid_amd import _native as N
    L = N.lib()
    for name in ("eg_top_k_track", "eg_fetch_top_k", "eg_group_top_k_track", "eg_group_fetch_top_k", "eg_rank_score"):
        assert hasattr(L, name) and name in N.EXPORTS, name
    header = open(os.path.join(ROOT, "include", "eirgrid_hip.h")).read()
    assert int(re.search(r"#define EG_TOPK_MAX (\d+)", header).group(1)) == N.TOPK_MAX == 64


def _sweep():
    rng = np.random.default_rng(17)
    n = 4000
    net = np.where(rng.uniform(size=n) < 0.5, rng.uniform(1.0, 2e6, n), -rng.uniform(0.0, 5e5, n))
    cost = 10.0 ** rng.uniform(8.0, 14.0, n)
    m = np.stack([net, rng.uniform(0.0, 1.0, n), cost, rng.uniform(0.0, 1.0, n)], axis=1)
    edges = np.array([[0.0, 0.5, 5e10, 1.0], [-1.0, 0.5, 5e10, 1.0], [1e6, 0.5, 4e11, 1.0], [-1.0, 0.3, 4e11, 1.0],
                      [-1.0, 0.3, 4.0000001e11, 1.0], [-1.0, 0.9, 5e12, 1.0], [-1.0, 0.9, 1e15, 1.0], [-1.0, 0.9, 0.0, 1.0]])
    return np.concatenate([m, edges])


def test_rank_score_mode_none_is_score_metrics(built):
    from eirgrid_amd import _native as N
    from eirgrid_amd.engine import rank_score, score_metrics
    L = N.lib()
    for m in _sweep():
        want = score_metrics(m)
        mm = np.ascontiguousarray(m)
        got0 = L.eg_rank_score(mm.ctypes.data_as(N._dp), 0)
        assert got0 == rank_score(m)      # mode 0 and mode 1 are both optimization_mode None
        assert abs(got0 - want) <= 1e-14 * abs(want), (m, got0, want)


def test_rank_score_cost_only_follows_scoring_rs(built):
    """scoring.rs:7-15: 2.0 up to MAX_ACCEPTABLE_COST, falling with log(cost) to 1.0 at 100 times it, 1.0 beyond; emissions and
    opinion play no part."""
    from eirgrid_amd.engine import rank_score, score_metrics
    costs = np.concatenate([[0.0, 1e9, 5e10], np.geomspace(5e10, 5e12, 300), [5e12, 6e12, 1e15]])
    s = [rank_score([123.0, 0.4, c, 1.0], cost_only=True) for c in costs]
    assert all(a >= b for a, b in zip(s, s[1:]))
    assert s[0] == s[1] == s[2] == 2.0 and s[-3] == s[-2] == s[-1] == 1.0
    assert 1.0 < rank_score([0.0, 0.0, 5e11, 0.0], cost_only=True) < 2.0
    assert rank_score([-5.0, 0.9, 7e11, 1.0], cost_only=True) == rank_score([9e5, 0.1, 7e11, 0.0], cost_only=True)
    for m in _sweep():
        want = score_metrics(m, cost_only=True)
        assert abs(rank_score(m, cost_only=True) - want) <= 1e-14 * abs(want), m


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_top_k_kernels_compile_without_scratch():
    """The three kernels exist for gfx950 in exactly one of eg_rollout.hip's two objects, spill nothing and need no scratch."""
    out = "\n".join(kernel_resource_lines())
    for name in ("k_topk_keys", "k_topk_select", "k_topk_merge"):
        lines = [l for l in out.splitlines() if re.search(rf"remark: {name}(\b|E)", l)]
        assert len(lines) == 1, (name, lines)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", lines[0])
        assert m, lines[0]
        scratch, spill, lds = (int(m.group(k)) for k in (1, 2, 3))
        assert scratch == 0 and spill == 0, (name, lines[0])
        assert lds <= 64 * 1024, (name, lds)
