"""What the compiler makes of k_plan_edits (no GPU needed: scripts/kernel_resources.sh, device code only).

The kernel builds the plan blocks of a plan-edit batch in front of the rollout grids (csrc/eg_plan_edits.h): a block is 8.8 KB per wave,
written once — it must not touch scratch memory or spill a register on the way."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_plan_edits_kernel_uses_no_scratch_and_spills_nothing():
    out = "\n".join(kernel_resource_lines())
    rows = [line for line in out.splitlines() if re.search(r"\bk_plan_edits", line)]
    assert len(rows) == 1, out      # (eg_rollout.o only: the throughput object does not carry it)
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0, scratch
    assert vgpr_spill == 0 and sgpr_spill == 0, (vgpr_spill, sgpr_spill)
    assert lds == 0, lds
    assert vgprs <= 64, vgprs      # eight waves per SIMD: the grid is memory-bound
