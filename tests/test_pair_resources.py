"""Compiler-reported resources of the paired-analysis kernel (the pattern of test_deform_resources.py): pair_kernels.hip compiles
for gfx950 with the product flags and without a warning of its own, pm_pair_kernel is there in its five instantiations -- one per
moving dtype; the fixed volume's dtype is read at run time -- and nothing else, none spills to scratch -- the eight corners, the nine
Jacobian entries and the thirteen columns of a thread's label stay in registers -- and the LDS per workgroup is what the file's head
comment claims: the 16 x 13 table and the label table.  Needs hipcc (cross-compiles for gfx950 without a GPU)."""
import re

from resource_report import column, kernel_resources, needs_hipcc, source_text

KERNELS = {"pm_pair_kernel": 5}


@needs_hipcc
def test_pair_kernel_uses_no_scratch():
    from lungmask_amd import pairs

    assert callable(pairs.pair_analysis)  # (the feature the kernel belongs to)
    stderr, kernels = kernel_resources("pair_kernels.hip")
    assert not [ln for ln in stderr.splitlines() if "warning" in ln and "pair_kernels.hip" in ln], stderr
    scratch, lds, vgprs = column(kernels, "scratch"), column(kernels, "lds"), column(kernels, "vgprs")
    for kernel, count in KERNELS.items():
        assert sum(re.search(r"\d" + kernel + r"[A-Z]", n) is not None for n in scratch) == count, (kernel, sorted(scratch))
    assert len(scratch) == sum(KERNELS.values()), sorted(scratch)
    assert all(s == 0 for s in scratch.values()), scratch
    text = source_text("pair_kernels.hip")
    m = re.search(r"LDS per workgroup: (\d+) \(16 x 13 cells of 8 bytes\) \+ (\d+) \(label table\) = (\d+) bytes\.  No scratch\.", text)
    cells, table, claimed = (int(v) for v in m.groups())
    assert (cells, table, claimed) == (16 * 13 * 8, 256, 16 * 13 * 8 + 256) and set(lds.values()) == {claimed}, lds
    assert max(vgprs.values()) <= 128, vgprs  # at least four waves per SIMD
