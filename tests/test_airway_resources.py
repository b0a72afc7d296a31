"""Compiler-reported resources of the airway kernels (the pattern of test_lcc_resources.py): airway_kernels.hip compiles with the
product flags, its five kernels are there once each and nothing else is, none spills to scratch, and the LDS per workgroup is what
the file's head comment claims: the packed brick with its face halos and the flags for a round, the histogram for the curve, the 256
label counters for the mask.  The relaxation kernel keeps at least four waves per SIMD.  Needs hipcc (cross-compiles for gfx950
without a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

KERNELS = {"seed_init_kernel": 1, "seed_plant_kernel": 1, "seed_round_kernel": 1, "seed_hist_kernel": 1, "airway_mask_kernel": 1}


@needs_hipcc
def test_airway_kernels_use_no_scratch():
    import lungmask_amd.airways  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("airway_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    assert all(s == 0 for s in found.values()), found
    text = source_text("airway_kernels.hip")
    m = re.search(r"LDS per workgroup of a round: 10 \* 10 \* 35 \* 4 \+ 16 \(flags\) = (\d+) bytes", text)
    round_claimed = int(m.group(1))
    assert round_claimed == 10 * 10 * 35 * 4 + 16
    m = re.search(r"a histogram of cap_hu \+ 1025 bins in LDS \((\d+) bytes for the largest cap\)", text)
    hist_claimed = int(m.group(1))
    assert hist_claimed == (3071 + 1025) * 4
    want = {"seed_round_kernel": round_claimed, "seed_hist_kernel": hist_claimed, "airway_mask_kernel": 256 * 4, "seed_init_kernel": 0,
            "seed_plant_kernel": 0}
    for n, v in lds.items():
        assert v == next(w for k, w in want.items() if k in n), lds
    occ = column(kernels, "occupancy")
    assert all(v >= 4 for n, v in occ.items() if "seed_round_kernel" in n), (occ, column(kernels, "vgprs"))
