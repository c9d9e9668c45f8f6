"""What the compiler makes of k_repair_pick_many (csrc/eg_repair.h; no GPU needed: scripts/kernel_resources.sh, device code only).  The kernel
runs once per launch of a repair round behind the rollout grids and k_plan_constraints, a workgroup of sixteen waves per plan: it may not
touch scratch memory, may not spill, keeps its LDS to the one exchange across the waves — less than a granule — and stays at four waves a
SIMD or better.  It lives in eg_rollout.o only.  (That no other kernel moved with it is what the other resource tests pin.)"""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

LDS_GRANULE = 1280      # gfx950 hands LDS out in granules of 1 280 bytes


def test_the_kernel_uses_no_scratch_no_spills_and_less_than_a_granule_of_lds():
    lines = list(kernel_resource_lines())
    rows = [line for line in lines if "k_repair_pick_many" in line]
    assert len(rows) == 1, rows      # (exactly one row: the throughput object does not carry it)
    second = next(i for i, line in enumerate(lines) if line.startswith("# eg_rollout.hip") and i > 0)
    assert lines.index(rows[0]) < second, "k_repair_pick_many belongs to eg_rollout.o"
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert 0 < lds < LDS_GRANULE, lds
    assert vgprs <= 128, vgprs


def test_its_name_is_not_one_the_other_resource_tests_select():
    row = next(line for line in kernel_resource_lines() if "k_repair_pick_many" in line)
    name = re.search(r"(\w*k_repair_pick_many\w*)", row).group(1)
    for other in ("k_plan_edits", "k_plan_moves", "k_plan_crosses", "k_plan_rewrites", "k_plan_constraints", "k_refine_pick"):
        assert other not in name, (name, other)
