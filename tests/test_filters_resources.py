"""Compiler-reported resources of the filter kernels: every kernel is there and none spills to scratch.  Needs hipcc
(cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lungmask_amd", "csrc", "filter_kernels.hip")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_filter_kernels_use_no_scratch(tmp_path):
    from lungmask_amd import filters  # noqa: F401  (the feature these kernels belong to)

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
    # the median for three dtypes, each from registers (3 x 3 x 3) and from the tile; the pass kernels unmasked and masked
    for kernel, count in (("median_kernel", 6), ("sep_x_kernel", 2), ("sep_line_kernel", 2), ("filter_fill_kernel", 1)):
        assert sum(kernel in n for n in found) == count, (kernel, sorted(found))
    assert all(s == 0 for s in found.values()), found
