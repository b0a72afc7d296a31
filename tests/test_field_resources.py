"""Compiler-reported resources of the field kernel (the pattern of test_deform_resources.py): field_kernels.hip compiles for gfx950
with the product flags, fc_combine_kernel is there exactly once and nothing else, it does not spill to scratch -- the taps and the 24
corner values stay in registers -- and its LDS per workgroup is what the file's head comment claims: the four counters.  Needs hipcc
(cross-compiles for gfx950 without a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

KERNELS = {"fc_combine_kernel": 1}


@needs_hipcc
def test_field_kernel_uses_no_scratch():
    from lungmask_amd import deformable

    assert callable(deformable.invert) and callable(deformable.compose)  # (the feature the kernel belongs to)
    _, kernels = kernel_resources("field_kernels.hip")
    scratch, lds, vgprs = column(kernels, "scratch"), column(kernels, "lds"), column(kernels, "vgprs")
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in scratch) == count, (kernel, sorted(scratch))
    assert len(scratch) == sum(KERNELS.values()), sorted(scratch)
    assert all(s == 0 for s in scratch.values()), scratch
    text = source_text("field_kernels.hip")
    m = re.search(r"LDS per workgroup: (\d+) bytes \(four counters\)\.  VGPRs: (\d+) ", text)
    lds_claimed, vgprs_claimed = int(m.group(1)), int(m.group(2))
    assert lds_claimed == 4 * 8 and list(lds.values()) == [lds_claimed], lds
    assert max(vgprs.values()) <= 128 and vgprs_claimed <= 128, vgprs  # at least four waves per SIMD
