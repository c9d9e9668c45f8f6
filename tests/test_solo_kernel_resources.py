"""What the compiler makes of the per-episode replay kernel (no GPU needed: scripts/kernel_resources.sh, device code only).

k_replay_solo runs beside the lean grid at four waves per SIMD; its tile search (csrc/eg_field.h place_tiles) must not cost it
that: no scratch memory, at most 128 vector registers, and no more LDS than the long-replay variant of k_rollout it stands in for."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_replay_solo_keeps_four_waves_per_simd_and_no_scratch():
    out = "\n".join(kernel_resource_lines())
    solo = [re.search(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", line)
            for line in out.splitlines() if re.search(r"\bk_replay_solo\b", line)]
    long_replay = [re.search(r"LDS Size \[bytes/block\]: (\d+)", line) for line in out.splitlines() if line.startswith("k_rolloutILi0ELi2E")]
    assert solo and all(solo) and long_replay and all(long_replay), out
    for m in solo:
        vgprs, scratch, lds = (int(m.group(k)) for k in (1, 2, 3))
        assert vgprs <= 128, vgprs
        assert scratch == 0, scratch
        assert lds <= int(long_replay[0].group(1)), (lds, long_replay[0].group(1))
