"""Compiler-reported resources of the local-correlation kernels (the pattern of test_deform_resources.py): lcc_kernels.hip compiles
with the product flags, its three kernels are there once each and nothing else is -- sample_common.h's gathers are not instantiated
here --, none spills to scratch -- the six accumulators of the x pass and the step's sums stay in registers -- and the LDS per
workgroup is what the file's comment claims: the two line tiles of the x pass, the tile of a line pass, six counters and the label
table for the step.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

KERNELS = {"lc_moments_x_kernel": 1, "lc_moments_line_kernel": 1, "lc_step_kernel": 1}


@needs_hipcc
def test_lcc_kernels_use_no_scratch():
    import lungmask_amd.deformable  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("lcc_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    assert all(s == 0 for s in found.values()), found
    text = source_text("lcc_kernels.hip")
    m = re.search(r"LDS per workgroup: (\d+) bytes for the x pass \(4 waves x 2 lines x 272 floats\), (\d+) bytes for a line pass \(80 x 64 doubles\)", text)
    x_claimed, line_claimed = int(m.group(1)), int(m.group(2))
    assert x_claimed == 4 * 2 * (256 + 2 * 8) * 4 and line_claimed == (64 + 2 * 8) * 64 * 8
    m = re.search(r"48 \(six counters\) \+ 256 \(label table\) = (\d+) bytes for the step", text)
    step_claimed = int(m.group(1))
    assert step_claimed == 6 * 8 + 256
    for n, v in lds.items():
        assert v == (x_claimed if "lc_moments_x_kernel" in n else line_claimed if "lc_moments_line_kernel" in n else step_claimed), lds
    # occupancy: every kernel keeps at least four waves per SIMD (the line pass is bounded by its 40 KB tile)
    occ = column(kernels, "occupancy")
    assert all(v >= 4 for v in occ.values()), (occ, column(kernels, "vgprs"))
