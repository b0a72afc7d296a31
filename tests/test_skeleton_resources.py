"""Compiler-reported resources of the skeleton kernels (the pattern of test_vessel_resources.py): skeleton_kernels.hip compiles with
the product flags, every kernel is there in its expected number of instantiations, none spills to scratch -- the neighbourhood word
and the two flood fills of the simple-point test stay in registers -- and the LDS stays within what the file's comment claims (the
keep table, a scan buffer or the 16 x 9 counters: under 2 KiB).  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
from resource_report import column, kernel_resources, needs_hipcc

KERNELS = {"skel_init_kernel": 1, "skel_substep_kernel": 1, "skel_code_kernel": 1, "points_count_kernel": 1, "points_scan_kernel": 1,
           "points_write_kernel": 1, "calibre_class_kernel": 1, "calibre_out_kernel": 1, "vessel_mask_kernel": 1}


@needs_hipcc
def test_skeleton_kernels_use_no_scratch():
    import lungmask_amd.skeleton  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("skeleton_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(kernel in n for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    assert all(s == 0 for s in found.values()), found
    assert all(v <= 2048 for v in lds.values()), lds
    assert max(v for n, v in lds.items() if "skel_substep_kernel" in n) <= 16, lds  # the thinning itself: one counter
