"""What the compiler makes of the two kernels of eg_refine_plans (csrc/eg_refine_many.h; no GPU needed: scripts/kernel_resources.sh, device
code only).  k_refine_pick_many runs once per launch behind the rollout grids and k_plan_edits_many in front of them: neither may touch
scratch memory or spill, and both stay small.  (That the one-plan kernels and the rollout kernels did not change with them is what
tests/test_refine_resources.py, test_plan_edit_resources.py, test_solo_kernel_resources.py and test_kernel_resources.py pin.)"""
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


@pytest.mark.parametrize("kernel, lds_most", [("k_refine_pick_many", 1024), ("k_plan_edits_many", 0)])
def test_the_kernels_use_no_scratch_and_few_registers(resources, kernel, lds_most):
    rows = [line for line in resources if kernel in line]
    assert len(rows) == 1, resources      # (eg_rollout.o only: the throughput object does not carry it)
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert lds <= lds_most, lds      # the pick: one exchange across sixteen waves; the edits kernel: none
    assert vgprs <= 64, vgprs
