"""Compiler-reported resources of the component kernels: every kernel is there and none spills to scratch.  Needs hipcc
(cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lungmask_amd", "csrc", "component_kernels.hip")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_component_kernels_use_no_scratch(tmp_path):
    from lungmask_amd import components  # noqa: F401  (the feature these kernels belong to)

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", SRC, "-o",
                        str(tmp_path / "t.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    found = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            found[name] = int(m.group(1))
    for kernel in ("comp_select_kernel", "comp_table_kernel", "comp_relabel_kernel"):
        assert sum(kernel in n for n in found) == 1, (kernel, sorted(found))
    assert all(s == 0 for s in found.values()), found
