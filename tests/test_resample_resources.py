"""Compiler-reported resources of the resampling kernels (the pattern of test_skeleton_resources.py): resample_kernels.hip compiles
with the product flags, every kernel is there in its expected number of instantiations -- the shared gathers of sample_common.h with
this file's map type, RsMap, in their names -- none spills to scratch -- the 3 x 4 tap indices and weights of the cubic gather and
the eight corners of the label-linear one stay in registers -- and only the x pass of the prefilter uses LDS: its 64 x 65 float64
tile, 33280 bytes, as the file's comment claims.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

# nearest: one per element size; linear: five sources x (float32, float16) + three integer sources x int16; cubic: three outputs
KERNELS = {"gather_nearest_kernel": 4, "gather_linear_kernel": 13, "gather_cubic_kernel": 3, "gather_label_linear_kernel": 1, "rs_convert_kernel": 5,
           "rs_prefilter_lines_kernel": 1, "rs_prefilter_x_kernel": 1}


@needs_hipcc
def test_resample_kernels_use_no_scratch():
    import lungmask_amd.resample  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("resample_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(kernel in n for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    for n in found:  # every gather is this file's: its mangled name carries the map type
        assert ("gather_" in n) == ("5RsMap" in n) and "DfMap" not in n, n
    assert all(s == 0 for s in found.values()), found
    claimed = int(re.search(r"LDS: 64 \* 65 \* 8 = (\d+) bytes", source_text("resample_kernels.hip")).group(1))
    assert claimed == 64 * 65 * 8
    for n, v in lds.items():
        assert v <= (claimed if "rs_prefilter_x_kernel" in n else 0), lds
