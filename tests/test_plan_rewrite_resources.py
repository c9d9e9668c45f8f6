"""What the compiler makes of k_plan_rewrites (csrc/eg_plan_rewrites.h; no GPU needed: scripts/kernel_resources.sh, device code only).  The
kernel runs in front of a plan batch's rollout grids, a wave per variant: it may not touch scratch memory, may not spill, keeps its map
in the wave's registers (no LDS, or at most a 64-byte table per wave) and stays at four waves a SIMD or better.  It lives in eg_rollout.o
only."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def test_the_kernel_uses_no_scratch_no_spills_and_at_most_a_map_table_of_lds():
    out = "\n".join(kernel_resource_lines())
    lines = out.splitlines()
    rows = [line for line in lines if "k_plan_rewrites" in line]
    assert len(rows) == 1, rows      # (eg_rollout.o only: the throughput object does not carry it)
    second = next(i for i, line in enumerate(lines) if line.startswith("# eg_rollout.hip") and i > 0)
    assert lines.index(rows[0]) < second, "k_plan_rewrites belongs to eg_rollout.o"
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert lds <= 256, lds           # (the map is held a lane an entry: 0; a 64-byte table per wave would be 256)
    assert vgprs <= 128, vgprs       # (four waves a SIMD of the 512-register file)
