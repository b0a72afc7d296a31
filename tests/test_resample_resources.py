"""Compiler-reported resources of the resampling kernels (the pattern of test_skeleton_resources.py): resample_kernels.hip compiles
with the product flags, every kernel is there in its expected number of instantiations -- the shared gathers of sample_common.h with
this file's map type, RsMap, in their names -- none spills to scratch -- the 3 x 4 tap indices and weights of the cubic gather and
the eight corners of the label-linear one stay in registers -- and only the x pass of the prefilter uses LDS: its 64 x 65 float64
tile, 33280 bytes, as the file's comment claims.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nearest: one per element size; linear: five sources x (float32, float16) + three integer sources x int16; cubic: three outputs
KERNELS = {"gather_nearest_kernel": 4, "gather_linear_kernel": 13, "gather_cubic_kernel": 3, "gather_label_linear_kernel": 1, "rs_convert_kernel": 5,
           "rs_prefilter_lines_kernel": 1, "rs_prefilter_x_kernel": 1}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_resample_kernels_use_no_scratch(tmp_path):
    import lungmask_amd.resample  # noqa: F401  (the feature module the kernels belong to)

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "lungmask_amd", "csrc", "resample_kernels.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", src, "-o", str(tmp_path / "t.o"),
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
    for n in found:  # every gather is this file's: its mangled name carries the map type
        assert ("gather_" in n) == ("5RsMap" in n) and "DfMap" not in n, n
    assert all(s == 0 for s in found.values()), found
    claimed = int(re.search(r"LDS: 64 \* 65 \* 8 = (\d+) bytes", open(src).read()).group(1))
    assert claimed == 64 * 65 * 8
    for n, v in lds.items():
        assert v <= (claimed if "rs_prefilter_x_kernel" in n else 0), lds
