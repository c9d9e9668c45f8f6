"""What the compiler makes of k_refine_pick, and that adding it left the kernels of a plan batch alone (no GPU needed:
scripts/kernel_resources.sh, device code only).

k_refine_pick (csrc/eg_refine.h) runs once per refinement round behind the rollout grids: it must not touch scratch memory.  k_rollout,
k_replay_solo and k_plan_edits are not to change with this feature: their resource lines must be the ones the build before it gave,
kept in tests/golden/kernel_resources_before_refine.txt (the same script's output, file positions removed)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def _plain(line):
    """a resource line without the positions the remarks of a kernel in a header carry (they move with every edit of the header)"""
    return re.sub(r"\s+", " ", re.sub(r"\./\w+\.h:\d+:\d+: remark: ?", "", line)).strip()


@pytest.fixture(scope="module")
def resources():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh")], capture_output=True, text=True, timeout=900).stdout
    return [_plain(line) for line in out.splitlines()]


def test_refine_pick_uses_no_scratch_and_little_lds(resources):
    rows = [line for line in resources if re.search(r"\bk_refine_pick", line)]
    assert len(rows) == 1, resources      # (eg_rollout.o only: the throughput object does not carry it)
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert lds <= 1024, lds      # one exchange across sixteen waves: a score, an index and a count each
    assert vgprs <= 64, vgprs    # a workgroup of 1 024 threads needs at most 128; nothing here wants more than a few dozen


def test_the_plan_batch_kernels_are_unchanged(resources):
    want = [_plain(line) for line in open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_refine.txt")) if line.strip()]
    assert len(want) == 8 and sum("k_rollout" in w for w in want) == 6
    got = [line for line in resources if re.search(r"\bk_rollout|\bk_replay_solo|\bk_plan_edits", line)]
    assert got == want, "\n".join(sorted(set(got) ^ set(want)))
