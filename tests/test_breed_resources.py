"""What the compiler makes of k_breed_gather and k_breed_turnover (csrc/eg_breed.h; no GPU needed: scripts/kernel_resources.sh, device code
only).  The two kernels copy plan blocks behind a chunk's fold and behind a generation, a wave per archive entry: they may not touch
scratch memory or LDS, may not spill, and stay small.  They live in eg_rollout.o only."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@pytest.fixture(scope="module")
def lines():
    return list(kernel_resource_lines())


@pytest.mark.parametrize("kernel", ["k_breed_gather", "k_breed_turnover"])
def test_the_kernel_uses_no_scratch_no_lds_and_few_registers(lines, kernel):
    rows = [line for line in lines if kernel in line]
    assert len(rows) == 1, rows      # (eg_rollout.o only: the throughput object does not carry it)
    second = next(i for i, line in enumerate(lines) if line.startswith("# eg_rollout.hip") and i > 0)
    assert lines.index(rows[0]) < second, f"{kernel} belongs to eg_rollout.o"
    m = re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", rows[0])
    assert m, rows[0]
    vgprs, scratch, sgpr_spill, vgpr_spill, lds = (int(m.group(k)) for k in range(1, 6))
    assert scratch == 0 and vgpr_spill == 0 and sgpr_spill == 0, rows[0]
    assert lds == 0, lds
    assert vgprs <= 72, vgprs      # (seven waves a SIMD: 512 registers in granules of 8)
