"""Compiler-reported resources of the metrics kernels: none of them may spill to scratch.  Needs hipcc (cross-compiles for gfx950
without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lungmask_amd", "csrc", "metrics_kernels.hip")
KERNELS = ("edt_x_kernel", "edt_line_kernel", "agree_init_kernel", "agree_overlap_kernel", "surf_reduce_kernel", "surf_sum_kernel",
           "select_hist_kernel", "select_scan_kernel")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_metrics_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", SRC, "-o",
                        str(tmp_path / "m.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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
    for k in KERNELS:
        hits = {n: s for n, s in found.items() if k in n}
        assert hits, (k, sorted(found))
        assert all(s == 0 for s in hits.values()), hits
    assert sum("agree_overlap_kernel" in n for n in found) == 2  # the per-label and the binarised form
    assert all(s == 0 for s in found.values()), found
