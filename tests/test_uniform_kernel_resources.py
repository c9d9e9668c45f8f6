"""What the compiler makes of k_episodes<kind>, the lean and the short-replay kind of a throughput batch with the episode's control
state uniform (csrc/eg_rollout_episode.h, kUniform) — no GPU needed: scripts/kernel_resources.sh, device code only.

They run where k_rollout<0, 0> and k_rollout<0, 1> ran, at four waves per SIMD beside the long replays: no scratch memory, at most 128
vector registers, k_rollout's 8 736 bytes of LDS.  And the point of them is that values which are the same in every lane stay out of
the vector registers: neither their vector registers nor their spilled scalar registers may exceed those of the k_rollout instance
of the same kind FROM THE SAME COMPILE (not a fixed number: both move with the compiler)."""
import os
import re
import shutil

import pytest

from tests.kernel_resources import kernel_resource_lines

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
_FIELDS = re.compile(r"VGPRs: (\d+) .*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)")


@pytest.fixture(scope="module")
def lines():
    return "\n".join(kernel_resource_lines()).splitlines()


def _one(lines, prefix):
    got = [_FIELDS.search(line) for line in lines if line.startswith(prefix)]
    assert len(got) == 1 and got[0], (prefix, got)
    return dict(zip(("vgprs", "scratch", "sgpr_spills", "lds"), (int(got[0].group(k)) for k in (1, 2, 3, 4))))


@pytest.mark.parametrize("kind", (0, 1))
def test_uniform_kernels_fit_beside_the_long_replays_and_are_leaner_than_k_rollout(lines, kind):
    new, old = _one(lines, f"k_episodesILi{kind}E"), _one(lines, f"k_rolloutILi0ELi{kind}E")
    assert new["scratch"] == 0, new
    assert new["vgprs"] <= 128, new
    assert new["lds"] == 8736 == old["lds"], (new, old)
    assert new["vgprs"] <= old["vgprs"], (new, old)
    assert new["sgpr_spills"] <= old["sgpr_spills"], (new, old)
