"""Compiler-reported resources of the deformable-registration kernels (the pattern of test_register_resources.py):
deform_kernels.hip compiles with the product flags, every kernel is there in its expected number of instantiations -- the shared
gathers of sample_common.h with this file's map type, DfMap, in their names -- none spills to
scratch -- the eight corners, the 64 cubic taps and the nine Jacobian entries stay in registers -- and the LDS per workgroup is what
the file's comment claims: five counters and the label table for the demons step, two counters for the Jacobian, none for the
gathers.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nearest: four element sizes; linear: five source dtypes x (float32, float16) and int16 for the three integer ones; cubic: three
# output dtypes; the demons step: five moving dtypes (the fixed volume's dtype is read at run time)
KERNELS = {"gather_nearest_kernel": 4, "gather_linear_kernel": 13, "gather_cubic_kernel": 3, "gather_label_linear_kernel": 1, "df_demons_kernel": 5,
           "df_jacobian_kernel": 1}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_deform_kernels_use_no_scratch(tmp_path):
    import lungmask_amd.deformable  # noqa: F401  (the feature module the kernels belong to)

    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "lungmask_amd", "csrc", "deform_kernels.hip")
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
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    for n in found:  # every gather is this file's: its mangled name carries the map type
        assert ("gather_" in n) == ("5DfMap" in n) and "RsMap" not in n, n
    assert all(s == 0 for s in found.values()), found
    text = open(src).read()
    m = re.search(r"40 \(five counters\) \+ 256 \(label table\) = (\d+) bytes for the demons step, (\d+) bytes \(two counters\) for the Jacobian", text)
    demons_claimed, jacobian_claimed = int(m.group(1)), int(m.group(2))
    assert demons_claimed == 5 * 8 + 256 and jacobian_claimed == 2 * 8
    for n, v in lds.items():
        assert v == (demons_claimed if "df_demons_kernel" in n else jacobian_claimed if "df_jacobian_kernel" in n else 0), lds
