"""Compiler-reported resources of the analysis kernels, one case per kernel file: the file compiles with the product flags, every
kernel is there in its expected number of instantiations, and none spills to scratch.  Needs hipcc (cross-compiles for gfx950
without a GPU)."""
import importlib

import pytest

from resource_report import column, kernel_resources, needs_hipcc

# (source file, feature module the kernels belong to (imported first) or None, {kernel name: instantiations})
CASES = [
    ("morph_kernels.hip", "morphology", {"nl_x_kernel": 1, "nl_line_kernel": 1, "morph_feat_kernel": 1, "morph_apply_kernel": 1}),
    ("component_kernels.hip", "components", {"comp_select_kernel": 1, "comp_table_kernel": 1, "comp_relabel_kernel": 1}),
    # the counting pass and the emitting pass
    ("mesh_kernels.hip", None, {"mesh_pass_kernel": 2, "mesh_scan_kernel": 1, "mesh_quad_ids_kernel": 1, "mesh_smooth_kernel": 1}),
    # the overlap kernel in the per-label and the binarised form
    ("metrics_kernels.hip", None, {"edt_x_kernel": 1, "edt_line_kernel": 1, "agree_init_kernel": 1, "agree_overlap_kernel": 2,
                                   "surf_reduce_kernel": 1, "surf_sum_kernel": 1, "select_hist_kernel": 1, "select_scan_kernel": 1}),
    # int16, int32, int64, float32, float64
    ("texture_kernels.hip", "texture", {"texture_code_kernel": 5, "texture_kernel": 1, "texture_reduce_kernel": 1}),
    # 5 source types x float32 / float16, 3 integer types x int16
    ("roi_kernels.hip", None, {"roi_resample_kernel": 13, "roi_keepmask_kernel": 1}),
    # the median for three dtypes, each from registers (3 x 3 x 3) and from the tile; the pass kernels unmasked and masked
    ("filter_kernels.hip", "filters", {"median_kernel": 6, "sep_x_kernel": 2, "sep_line_kernel": 2, "filter_fill_kernel": 1}),
]


@needs_hipcc
@pytest.mark.parametrize("source, feature, kernels", CASES, ids=[c[0].split("_")[0] for c in CASES])
def test_kernels_use_no_scratch(source, feature, kernels):
    if feature:
        importlib.import_module("lungmask_amd." + feature)
    found = column(kernel_resources(source)[1], "scratch")
    for kernel, count in kernels.items():
        assert sum(kernel in n for n in found) == count, (kernel, sorted(found))
    assert all(s == 0 for s in found.values()), found
