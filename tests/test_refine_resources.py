"""That plan refinement left the kernels of a plan batch alone (no GPU needed: scripts/kernel_resources.sh, device code only).

k_rollout, k_replay_solo and k_plan_edits are not to change with this feature: their resource lines must be the ones the build before
it gave, kept in tests/golden/kernel_resources_before_refine.txt (the same script's output, file positions removed).  What the compiler
makes of the refinement's own kernels — the pick runs once per launch behind the rollout grids and must not touch scratch memory — is
tests/test_refine_many_resources.py's: k_refine_pick_many serves eg_refine_plan as well."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def _plain(line):
    """a resource line without the positions the remarks of a kernel in a header carry (they move with every edit of the header)"""
    return re.sub(r"\s+", " ", re.sub(r"\./\w+\.h:\d+:\d+: remark: ?", "", line)).strip()


@pytest.fixture(scope="module")
def resources():
    out = "\n".join(kernel_resource_lines())
    return [_plain(line) for line in out.splitlines()]


def test_the_plan_batch_kernels_are_unchanged(resources):
    want = [_plain(line) for line in open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_refine.txt")) if line.strip()]
    assert len(want) == 8 and sum("k_rollout" in w for w in want) == 6
    got = [line for line in resources if re.search(r"\bk_rollout|\bk_replay_solo|\bk_plan_edits", line)]
    assert got == want, "\n".join(sorted(set(got) ^ set(want)))
