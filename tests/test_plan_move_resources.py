"""What the compiler makes of k_plan_moves (csrc/eg_plan_moves.h; no GPU needed: scripts/kernel_resources.sh, device code only).  The
kernel runs in front of a plan batch's rollout grids, a wave per variant: it may not touch scratch memory or LDS, may not spill, and
stays small.  It lives in eg_rollout.o only.  (That the kernels beside it did not change with it is what tests/test_plan_edit_resources.py,
test_refine_many_resources.py, test_solo_kernel_resources.py and test_kernel_resources.py pin.)"""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def test_the_kernel_uses_no_scratch_no_lds_and_few_registers():
    out = "\n".join(kernel_resource_lines())
    lines = out.splitlines()
    rows = [line for line in lines if "k_plan_moves" in line]
    assert len(rows) == 1, rows      # (eg_rollout.o only: the throughput object does not carry it)
    second = next(i for i, line in enumerate(lines) if line.startswith("# eg_rollout.hip") and i > 0)
    assert lines.index(rows[0]) < second, "k_plan_moves belongs to eg_rollout.o"
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert lds == 0, lds
    assert vgprs <= 64, vgprs
