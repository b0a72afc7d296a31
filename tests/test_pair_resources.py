"""Compiler-reported resources of the paired-analysis kernel (the pattern of test_deform_resources.py): pair_kernels.hip compiles
for gfx950 with the product flags and without a warning of its own, pm_pair_kernel is there in its five instantiations -- one per
moving dtype; the fixed volume's dtype is read at run time -- and nothing else, none spills to scratch -- the eight corners, the nine
Jacobian entries and the thirteen columns of a thread's label stay in registers -- and the LDS per workgroup is what the file's head
comment claims: the 16 x 13 table and the label table.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = {"pm_pair_kernel": 5}


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_pair_kernel_uses_no_scratch(tmp_path):
    from lungmask_amd import pairs

    assert callable(pairs.pair_analysis)  # (the feature the kernel belongs to)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "lungmask_amd", "csrc", "pair_kernels.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", src, "-o", str(tmp_path / "t.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert not [ln for ln in r.stderr.splitlines() if "warning" in ln and "pair_kernels.hip" in ln], r.stderr
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
    m = re.search(r"LDS per workgroup: (\d+) \(16 x 13 cells of 8 bytes\) \+ (\d+) \(label table\) = (\d+) bytes\.  No scratch\.", text)
    cells, table, claimed = (int(v) for v in m.groups())
    assert (cells, table, claimed) == (16 * 13 * 8, 256, 16 * 13 * 8 + 256) and set(lds.values()) == {claimed}, lds
    assert max(vgprs.values()) <= 128, vgprs  # at least four waves per SIMD
