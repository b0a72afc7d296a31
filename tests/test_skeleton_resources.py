"""Compiler-reported resources of the skeleton kernels (the pattern of test_vessel_resources.py): skeleton_kernels.hip compiles with
the product flags, every kernel is there in its expected number of instantiations, none spills to scratch -- the neighbourhood word
and the two flood fills of the simple-point test stay in registers -- and the LDS stays within what the file's comment claims (the
keep table, a scan buffer or the 16 x 9 counters: under 2 KiB).  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = {"skel_init_kernel": 1, "skel_substep_kernel": 1, "skel_code_kernel": 1, "points_count_kernel": 1, "points_scan_kernel": 1,
           "points_write_kernel": 1, "calibre_class_kernel": 1, "calibre_out_kernel": 1, "vessel_mask_kernel": 1}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_skeleton_kernels_use_no_scratch(tmp_path):
    import lungmask_amd.skeleton  # noqa: F401  (the feature module the kernels belong to)

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c",
                        os.path.join(ROOT, "lungmask_amd", "csrc", "skeleton_kernels.hip"), "-o", str(tmp_path / "t.o"),
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
    assert all(v <= 2048 for v in lds.values()), lds
    assert max(v for n, v in lds.items() if "skel_substep_kernel" in n) <= 16, lds  # the thinning itself: one counter
