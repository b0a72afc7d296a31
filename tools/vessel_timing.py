"""What the vessel filter costs (lm_vesselness_dev) on the 300 x 512 x 512 int16 phantom of lungmask_amd.synthetic with its lung-like
label volume (the phantom under the 'lunglike' head, as bench.py), spacing (1.0, 0.7, 0.7) mm:

  (a) vesselness_dev at the four default scales, masked by the labels: per kernel (engine profiler, HIP events around every launch)
      and as a whole call on device-resident arrays;
  (b) what the separable filter offers for the same six components: six filter_dev calls per scale with the derivative taps,
      unmasked (derivative orders have no masked form there), eighteen passes per scale and no eigen-analysis;
  (c) the unmasked vesselness, the single-scale Hessian with eigenvalues, and the vessel analysis (erosion and counts included).

The bar: (a) per scale takes no longer than (b) per scale.  Medians of `--reps` passes after two warm-up passes; the effective rate
of every vessel pass is the bytes its launch accounts for (what it must read and write) over its kernel time."""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import filters as flt  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402
from lungmask_amd import vessels as vs  # noqa: E402
from tools.filter_timing import kernels, median_ms  # noqa: E402

SPACING = (1.0, 0.7, 0.7)
ORDERS = [(0, 0, 2), (0, 2, 0), (2, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]  # (oz, oy, ox) of xx, yy, zz, xy, xz, yz


def clock_lines():
    """The GPU's current clocks as the system tool reports them (read only); empty when the tool is missing."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln]
    except (OSError, subprocess.SubprocessError):
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vessel_timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    log = open(args.log, "w")

    def out(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    n, h, w = args.n, 512, 512
    eng = nat.Engine(0)
    eng.load_state_dict(0, syn.synthetic_state_dict(3, head="lunglike"))
    vol = syn.phantom(n, h, w)
    lab = eng.apply(0, vol)
    sigmas_mm = vs.DEFAULT_SIGMAS_MM
    sig = vs.scale_sigmas(sigmas_mm, SPACING)
    out(f"volume {n} x {h} x {w} {vol.dtype}, spacing {SPACING} mm, {(lab > 0).mean() * 100:.1f} % labelled; scales {sigmas_mm} mm; "
        f"medians of {args.reps} (min..max) after 2 warm-up passes")
    for ln in clock_lines():
        out("clock: " + ln)
    vd, ld = eng.to_device(vol), eng.to_device(lab)
    bb = eng.roi_plan_dev(ld)
    out(f"box of the labels (zmin, zmax, ymin, ymax, xmin, xmax): {bb} = {(bb[1] - bb[0]) * (bb[3] - bb[2]) * (bb[5] - bb[4]) / vol.size * 100:.1f} % "
        f"of the volume; the passes of a scale run in it grown by the scale's radii")
    for s_mm, s in zip(sigmas_mm, sig):
        out(f"  scale {s_mm:g} mm: tap radii (z, y, x) {[flt.gaussian_taps(v).size // 2 for v in s]}")
    outv, outs, outf = eng.empty(vol.shape, np.float32), eng.empty(vol.shape, np.uint8), eng.empty(vol.shape, np.float32)

    def report(what, fn, per=1):
        call = median_ms(fn, args.reps)
        ks = kernels(eng, fn, args.reps)
        total = sum(v[0] for v in ks.values())
        out(f"{what:44s} whole call {call[0]:9.3f} ms ({call[1]:.3f}..{call[2]:.3f})   kernels {total:9.3f} ms = {total / per:8.3f} ms per scale")
        for k, (ms, b) in ks.items():
            out(f"{'':44s}   {k:18s} {ms:9.3f} ms" + (f"  {b / ms / 1e6:8.1f} GB/s" if ms > 0 and b > 0 else ""))
        return total / per

    def fused_masked():
        eng.vesselness_dev(vd, sig, lab=ld, out=outv)
        eng.sync()

    def fused_unmasked():
        eng.vesselness_dev(vd, sig, out=outv)
        eng.sync()

    taps = [[[flt.gaussian_taps(s[i], o) for o in range(3)] for i in range(3)] for s in sig]

    def six_filters():
        for t in taps:
            for oz, oy, ox in ORDERS:
                eng.filter_dev(vd, None, kind="separable", taps=[t[0][oz], t[1][oy], t[2][ox]], out=outf)
        eng.sync()

    a = report("(a) vesselness_dev, 4 scales, masked", fused_masked, len(sig))
    b = report("(b) 6 x filter_dev per scale, 4 scales, unmasked", six_filters, len(sig))
    out(f"(a) / (b) per scale: {a:.3f} ms / {b:.3f} ms = {a / b:.3f}   [{'PASS' if a <= b else 'FAIL'}: the bar is (a) <= (b)]")
    report("(c) vesselness_dev, 4 scales, unmasked", fused_unmasked, len(sig))

    def hessian():
        comp, eig = eng.hessian_dev(vd, sig[1], lab=ld, eigenvalues=True)
        eng.sync()
        comp.free()
        eig.free()

    report("(c) hessian_dev 1.5 mm + eigenvalues, masked", hessian)

    def analysis():
        for d in vs.analysis_dev(eng, vd, ld, sigmas_mm, 0.5, 2.0, SPACING)[:3]:
            d.free()

    report("(c) vessel analysis (filter, erosion, counts)", analysis)
    for d in (vd, ld, outv, outs, outf):
        d.free()
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
