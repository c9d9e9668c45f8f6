"""scripts/kernel_resources.sh once per test process: the script compiles eg_rollout.hip's two objects (device code only, no GPU needed),
and every test that reads a kernel's resource line reads the same output."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def kernel_resource_lines():
    """the script's output lines, as a tuple (one line per kernel behind a '# eg_rollout.hip ...' line per object)"""
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh")], capture_output=True, text=True, timeout=900).stdout
    return tuple(out.splitlines())
