"""Compiler-reported resources of the field kernel (the pattern of test_deform_resources.py): field_kernels.hip compiles for gfx950
with the product flags, fc_combine_kernel is there exactly once and nothing else, it does not spill to scratch -- the taps and the 24
corner values stay in registers -- and its LDS per workgroup is what the file's head comment claims: the four counters.  Needs hipcc
(cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = {"fc_combine_kernel": 1}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_field_kernel_uses_no_scratch(tmp_path):
    from lungmask_amd import deformable

    assert callable(deformable.invert) and callable(deformable.compose)  # (the feature the kernel belongs to)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "lungmask_amd", "csrc", "field_kernels.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", src, "-o", str(tmp_path / "t.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    scratch, lds, vgprs = {}, {}, {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for table, pattern in ((scratch, r"ScratchSize \[bytes/lane\]: (\d+)"), (lds, r"LDS Size \[bytes/block\]: (\d+)"), (vgprs, r" VGPRs: (\d+)")):
            m = re.search(pattern, line)
            if m and name:
                table[name] = int(m.group(1))
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in scratch) == count, (kernel, sorted(scratch))
    assert len(scratch) == sum(KERNELS.values()), sorted(scratch)
    assert all(s == 0 for s in scratch.values()), scratch
    text = open(src).read()
    m = re.search(r"LDS per workgroup: (\d+) bytes \(four counters\)\.  VGPRs: (\d+) ", text)
    lds_claimed, vgprs_claimed = int(m.group(1)), int(m.group(2))
    assert lds_claimed == 4 * 8 and list(lds.values()) == [lds_claimed], lds
    assert max(vgprs.values()) <= 128 and vgprs_claimed <= 128, vgprs  # at least four waves per SIMD
