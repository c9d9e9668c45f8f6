"""What the compiler makes of k_build_constraints (csrc/eg_build_constraints.h; no GPU needed: scripts/kernel_resources.sh, device code only).
The kernel runs behind a plan batch's rollout grids in place of k_plan_constraints, a wave per variant, four variants per workgroup: it may
not touch scratch memory, may not spill, holds a variant's 546 staged doubles and its 26 x 19 counters in 4 368 + 1 976 bytes of LDS per
wave and no more, and stays at four waves a SIMD or better.  It lives in eg_rollout.o only."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

LDS_GRANULE = 1280                                                                       # gfx950 hands LDS out in granules of 1 280 bytes
LDS_BOUND = -(-4 * (26 * 21 * 8 + 26 * 19 * 4) // LDS_GRANULE) * LDS_GRANULE              # 4 x (4 368 + 1 976) bytes, rounded to the granule


def test_the_kernel_uses_no_scratch_no_spills_and_four_variants_of_lds():
    out = "\n".join(kernel_resource_lines())
    lines = out.splitlines()
    rows = [line for line in lines if "k_build_constraints" in line]
    assert len(rows) == 1, rows      # (eg_rollout.o only: the throughput object does not carry it)
    assert "k_plan_constraints" not in rows[0]      # (tests/test_plan_constraint_resources.py finds its one row by that text)
    second = next(i for i, line in enumerate(lines) if line.startswith("# eg_rollout.hip") and i > 0)
    assert lines.index(rows[0]) < second, "k_build_constraints belongs to eg_rollout.o"
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert LDS_BOUND == 25600 and 0 < lds <= LDS_BOUND, lds      # (rows and counters: some LDS, at most four variants' worth)
    assert vgprs <= 128, vgprs                                    # (four waves a SIMD of the 512-register file)
