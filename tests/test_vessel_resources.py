"""Compiler-reported resources of the vessel kernels (the pattern of test_kernel_resources.py): vessel_kernels.hip compiles with the
product flags, every kernel is there in its expected number of instantiations, and none spills to scratch -- the eigen-solve and the
six accumulator sets of the fused z pass stay in registers.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the z pass unmasked and masked
KERNELS = {"vessel_x_kernel": 1, "vessel_y_kernel": 1, "vessel_z_kernel": 2, "vessel_counts_kernel": 1}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_vessel_kernels_use_no_scratch(tmp_path):
    import lungmask_amd.vessels  # noqa: F401  (the feature module the kernels belong to)

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c",
                        os.path.join(ROOT, "lungmask_amd", "csrc", "vessel_kernels.hip"), "-o", str(tmp_path / "t.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    found, lds = {}, {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            found[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    for kernel, count in KERNELS.items():
        assert sum(kernel in n for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    assert all(s == 0 for s in found.values()), found
    assert all(v <= 33 * 1024 for v in lds.values()), lds  # one line tile, as the separable filter's line pass
