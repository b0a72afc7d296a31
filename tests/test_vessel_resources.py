"""Compiler-reported resources of the vessel kernels (the pattern of test_kernel_resources.py): vessel_kernels.hip compiles with the
product flags, every kernel is there in its expected number of instantiations, and none spills to scratch -- the eigen-solve and the
six accumulator sets of the fused z pass stay in registers.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
from resource_report import column, kernel_resources, needs_hipcc

# the z pass unmasked and masked
KERNELS = {"vessel_x_kernel": 1, "vessel_y_kernel": 1, "vessel_z_kernel": 2, "vessel_counts_kernel": 1}


@needs_hipcc
def test_vessel_kernels_use_no_scratch():
    import lungmask_amd.vessels  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("vessel_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(kernel in n for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    assert all(s == 0 for s in found.values()), found
    assert all(v <= 33 * 1024 for v in lds.values()), lds  # one line tile, as the separable filter's line pass
