"""Compiler-reported resources of the deformable-registration kernels (the pattern of test_register_resources.py):
deform_kernels.hip compiles with the product flags, every kernel is there in its expected number of instantiations -- the shared
gathers of sample_common.h with this file's map type, DfMap, in their names -- none spills to
scratch -- the eight corners, the 64 cubic taps and the nine Jacobian entries stay in registers -- and the LDS per workgroup is what
the file's comment claims: five counters and the label table for the demons step, two counters for the Jacobian, none for the
gathers.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

# nearest: four element sizes; linear: five source dtypes x (float32, float16) and int16 for the three integer ones; cubic: three
# output dtypes; the demons step: five moving dtypes (the fixed volume's dtype is read at run time)
KERNELS = {"gather_nearest_kernel": 4, "gather_linear_kernel": 13, "gather_cubic_kernel": 3, "gather_label_linear_kernel": 1, "df_demons_kernel": 5,
           "df_jacobian_kernel": 1}


@needs_hipcc
def test_deform_kernels_use_no_scratch():
    import lungmask_amd.deformable  # noqa: F401  (the feature module the kernels belong to)

    _, kernels = kernel_resources("deform_kernels.hip")
    found, lds = column(kernels, "scratch"), column(kernels, "lds")
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in found) == count, (kernel, sorted(found))
    assert len(found) == sum(KERNELS.values()), sorted(found)
    for n in found:  # every gather is this file's: its mangled name carries the map type
        assert ("gather_" in n) == ("5DfMap" in n) and "RsMap" not in n, n
    assert all(s == 0 for s in found.values()), found
    text = source_text("deform_kernels.hip")
    m = re.search(r"40 \(five counters\) \+ 256 \(label table\) = (\d+) bytes for the demons step, (\d+) bytes \(two counters\) for the Jacobian", text)
    demons_claimed, jacobian_claimed = int(m.group(1)), int(m.group(2))
    assert demons_claimed == 5 * 8 + 256 and jacobian_claimed == 2 * 8
    for n, v in lds.items():
        assert v == (demons_claimed if "df_demons_kernel" in n else jacobian_claimed if "df_jacobian_kernel" in n else 0), lds
