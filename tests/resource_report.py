"""What the *_resources.py tests share: one compile of a kernel file for gfx950 with the product flags and
-Rpass-analysis=kernel-resource-usage, and the compiler's report per kernel.  Needs hipcc (cross-compiles without a GPU)."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lungmask_amd", "csrc")

needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")

FIELDS = {"scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "lds": r"LDS Size \[bytes/block\]: (\d+)", "vgprs": r" VGPRs: (\d+)",
          "sgprs": r"TotalSGPRs: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)"}


@functools.lru_cache(maxsize=None)
def kernel_resources(source):
    """(stderr of the compile, {mangled kernel name: {scratch, lds, vgprs, sgprs, occupancy}}) of csrc/<source>; compiled once."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-c", os.path.join(CSRC, source),
                            "-o", os.path.join(tmp, "t.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    kernels, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for field, pattern in FIELDS.items():
            m = re.search(pattern, line)
            if m and name:
                kernels.setdefault(name, {})[field] = int(m.group(1))
    return r.stderr, kernels


def column(kernels, field):
    """{kernel name: its `field`}"""
    return {n: v[field] for n, v in kernels.items()}


def source_text(source):
    """The text of csrc/<source>: the tests match the figures its head comment claims."""
    with open(os.path.join(CSRC, source)) as f:
        return f.read()
