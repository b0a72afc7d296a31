"""Compiler-reported resources of the joint-histogram kernels (the pattern of test_resample_resources.py): register_kernels.hip
compiles with the product flags, every kernel is there in its expected number of instantiations, none spills to scratch -- the eight
trilinear corners stay in registers -- and the LDS per workgroup is what the file's comment claims: 32 KiB of 64-bit counters, four
sample counters and the label table for the histogram kernel, 2 KiB for the reduction.  Needs hipcc (cross-compiles for gfx950 without
a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

# the histogram kernel: six moving dtypes x two modes (the fixed volume's dtype is read at run time)
KERNELS = {"jh_kernel": 12, "jh_reduce_kernel": 1}


@needs_hipcc
def test_register_kernels_use_no_scratch():
    import lungmask_amd.registration  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("register_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    assert all(s == 0 for s in found.values()), found
    text = source_text("register_kernels.hip")
    claimed = int(re.search(r"32768 \(histogram\) \+ 32 \(four counters\) \+ 256 \(label table\) = (\d+) bytes", text).group(1))
    reduce_claimed = int(re.search(r"8 x 32 x 8 = (\d+) bytes of LDS", text).group(1))
    assert claimed == 64 * 64 * 8 + 4 * 8 + 256 and reduce_claimed == 8 * 32 * 8
    for n, v in lds.items():
        assert v == (reduce_claimed if "jh_reduce_kernel" in n else claimed), lds
