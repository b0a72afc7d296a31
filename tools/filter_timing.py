"""What the image filters cost (lm_filter_dev) on the 300 x 512 x 512 int16 phantom of lungmask_amd.synthetic with its lung-like
label volume (the phantom under the 'lunglike' head, as bench.py), spacing (1.0, 0.7, 0.7) mm:

  1. median 3 (masked and unmasked) and median 5 (masked and unmasked), Gaussian at 1 mm and at 3 mm (masked and unmasked) and the
     low-attenuation map (5 mm), per kernel (engine profiler, HIP events) and as whole calls on device-resident arrays;
  2. beside each, where scipy is present (--no-scipy skips it): scipy.ndimage.median_filter / gaussian_filter (mode="nearest", whole
     volume: scipy has no masked form) on this machine's CPU, one pass; the 5 x 5 x 5 median on 60 of the slices, scaled;
  3. the effective bytes/s of every separable pass (the bytes its launch accounts for: what it must read and write) against the
     line passes of lm_edt_dev on the same volume.

Medians of `--reps` passes after two warm-up passes."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import components as cp  # noqa: E402
from lungmask_amd import filters as flt  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

SPACING = (1.0, 0.7, 0.7)


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernels(eng, fn, reps):
    """{kernel: (mean ms, mean bytes) per call of fn} from the engine profiler (HIP events around every launch), after fn has run warm."""
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        fn()
    prof = eng.profile_read()
    eng.profile(False)
    return {s["name"]: (s["total_ms"] / reps, s["bytes"] / reps) for s in prof}


def report(out, what, eng, fn, reps, rates):
    call = median_ms(fn, reps)
    ks = kernels(eng, fn, reps)
    total = sum(v[0] for v in ks.values())
    parts = "  ".join(f"{k} {v[0]:.3f}" for k, v in ks.items())
    out(f"{what:26s} whole call {call[0]:8.3f} ms ({call[1]:.3f}..{call[2]:.3f})   kernels {total:8.3f} ms:  {parts}")
    for k, (ms, b) in ks.items():
        if k.startswith(("sep_", "edt_")) and ms > 0:
            rates.append((what, k, b / ms / 1e6))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true", help="skip part 2 (scipy.ndimage on the CPU, one pass each)")
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "filter_timing.log"))
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
    out(f"volume {n} x {h} x {w} {vol.dtype}, spacing {SPACING} mm, {(lab > 0).mean() * 100:.1f} % labelled; "
        f"medians of {args.reps} (min..max) after 2 warm-up passes")
    ndimage = None
    if not args.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            out("scipy is not installed: no host figures")
    vd, ld = eng.to_device(vol), eng.to_device(lab)
    fd = eng.to_device((lab > 0).astype(np.uint8))
    out16, outf = eng.empty(vol.shape, np.int16), eng.empty(vol.shape, np.float32)
    rates = []

    def edt():
        eng.edt_dev(fd, SPACING, out=outf)
        eng.sync()

    report(out, "lm_edt_dev (yardstick)", eng, edt, args.reps, rates)

    def host(what, fn, scale=1.0, note=""):
        if ndimage is None:
            return
        t0 = time.perf_counter()
        fn()
        out(f"{'':26s} {what} on the CPU: {(time.perf_counter() - t0) * scale * 1e3:.0f} ms (one pass{note})")

    for size in (3, 5):
        for masked in (True, False):
            def run():
                eng.filter_dev(vd, ld if masked else None, kind="median", size=size, out=out16)
                eng.sync()

            report(out, f"median {size} {'masked' if masked else 'unmasked'}", eng, run, args.reps, rates)
        if size == 3:
            host("scipy.ndimage.median_filter(size=3)", lambda: ndimage.median_filter(vol, size=3, mode="nearest"))
        else:
            k = min(n, 60)
            host("scipy.ndimage.median_filter(size=5)", lambda: ndimage.median_filter(vol[:k], size=5, mode="nearest"), n / k,
                 f" over {k} slices, scaled to {n}")
    for mm in (1.0, 3.0):
        taps = flt.separable_taps(mm, SPACING)
        for masked in (True, False):
            def run():
                eng.filter_dev(vd, ld if masked else None, kind="separable", taps=taps, out=outf)
                eng.sync()

            report(out, f"gaussian {mm:g} mm {'masked' if masked else 'unmasked'}", eng, run, args.reps, rates)
        out(f"{'':26s} tap radii (z, y, x) {[t.size // 2 for t in taps]}")
        sig = [mm / s for s in SPACING]
        host(f"scipy.ndimage.gaussian_filter(sigma={mm:g} mm, float32)",
             lambda: ndimage.gaussian_filter(vol.astype(np.float32), sig, mode="nearest", truncate=4.0))
    taps = flt.separable_taps(5.0, SPACING)

    def laa():
        eng.filter_dev(vd, ld, kind="separable", taps=taps, fill=0.0, indicator=cp.cluster_range(-950), out=outf)
        eng.sync()

    report(out, "low-attenuation map 5 mm", eng, laa, args.reps, rates)
    out(f"{'':26s} tap radii (z, y, x) {[t.size // 2 for t in taps]}")
    out("effective rate of the separable passes (bytes each launch must move / kernel time) beside lm_edt_dev's passes:")
    for what, k, gbs in rates:
        out(f"  {what:26s} {k:14s} {gbs:8.1f} GB/s")
    out("Not tuned.")
    for d in (vd, ld, fd, out16, outf):
        d.free()
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
