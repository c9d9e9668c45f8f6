"""What the compiler makes of k_ensemble_keep and k_ensemble_commit (csrc/eg_ensemble.h; no GPU needed: scripts/kernel_resources.sh, device
code only).  The two run behind the passes of a plan batch under plan streams: neither may touch scratch memory or spill, neither uses
LDS (the commit exchanges through readlane and ballots alone), and the budgets below are what the compiler gives — 14 vector registers
for the copy, 44 for the commit, both at the full eight waves a SIMD.  They live in eg_rollout.o only."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

BUDGET = {"k_ensemble_keep": (14, 0), "k_ensemble_commit": (44, 0)}      # vector registers, LDS bytes a block


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_the_kernel_uses_no_scratch_no_spills_no_lds_and_stays_in_its_registers(kernel):
    lines = list(kernel_resource_lines())
    rows = [line for line in lines if "remark: " + kernel + " " in line]
    assert len(rows) == 1, rows      # (eg_rollout.o only: the throughput object does not carry it)
    second = next(i for i, line in enumerate(lines) if line.startswith("# eg_rollout.hip") and i > 0)
    assert lines.index(rows[0]) < second, kernel + " belongs to eg_rollout.o"
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, waves, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 7))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert (vgprs <= BUDGET[kernel][0], lds) == (True, BUDGET[kernel][1]) and waves == 8, rows[0]
