"""What the label morphology costs (lm_nearest_label_dev, lm_morph_dev) on the lung-like 300 x 512 x 512 label volume of
lungmask_amd.synthetic (the phantom under the 'lunglike' head, as bench.py), spacing (1.0, 0.7, 0.7) mm:

  1. lm_edt_dev of the binarised labels -- the yardstick -- and lm_nearest_label_dev on the same input, per kernel (engine profiler,
     HIP events) and as whole calls; the ratio of the two transforms;
  2. close at 5 mm and at 10 mm, and propagate (an infinite dilation), per kernel and as whole calls;
  3. where scipy is present (--no-scipy skips it): the same 10 mm closing on this machine's CPU, one pass, for context.  NOT
     scipy.ndimage.binary_closing itself: its cost grows with the ball (here 21 x 29 x 29 voxels) and one pass over this volume
     takes many minutes; the figure is the faster host recipe a user would pick, two scipy.ndimage.distance_transform_edt calls
     thresholded at the radius, whose result is compared with the device's.

Medians of `--reps` passes after two warm-up passes."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
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


def kernels_ms(eng, fn, reps):
    """{kernel: mean ms per call of fn} from the engine profiler (HIP events around every launch), after fn has run warm."""
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        fn()
    prof = eng.profile_read()
    eng.profile(False)
    return {s["name"]: s["total_ms"] / reps for s in prof}


def report(out, what, eng, fn, reps):
    call = median_ms(fn, reps)
    ks = kernels_ms(eng, fn, reps)
    total = sum(ks.values())
    parts = "  ".join(f"{k} {v:.3f}" for k, v in ks.items())
    out(f"{what:24s} whole call {call[0]:8.3f} ms ({call[1]:.3f}..{call[2]:.3f})   kernels {total:8.3f} ms:  {parts}")
    return call[0], total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true", help="skip part 3 (the 10 mm closing with scipy.ndimage on the CPU, one pass)")
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "morph_timing.log"))
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
    lab = eng.apply(0, syn.phantom(n, h, w))
    out(f"labels {n} x {h} x {w}, spacing {SPACING} mm, {(lab > 0).mean() * 100:.1f} % labelled, labels {sorted(np.unique(lab).tolist())}; "
        f"medians of {args.reps} (min..max) after 2 warm-up passes")
    ld = eng.to_device(lab)
    fd = eng.to_device((lab > 0).astype(np.uint8))
    d2 = eng.empty(lab.shape, np.float32)
    near = eng.empty(lab.shape, np.uint8)
    res = eng.empty(lab.shape, np.uint8)
    keep = nat.Engine._keep_table(None)
    sp = nat.Engine._spacing3(SPACING, "morph_timing")

    def edt():
        eng.edt_dev(fd, SPACING, out=d2)
        eng.sync()

    def nearest():
        eng.L.check(eng.L.lib.lm_nearest_label_dev(eng.h, ld.ptr, n, h, w, keep, sp, d2.ptr, near.ptr), "lm_nearest_label_dev")
        eng.sync()

    _, edt_k = report(out, "lm_edt_dev (yardstick)", eng, edt, args.reps)
    _, nl_k = report(out, "lm_nearest_label_dev", eng, nearest, args.reps)
    out(f"nearest-label transform / lm_edt_dev on the same input: {nl_k / edt_k:.2f} x (kernel time)")
    for what, op, r in (("close 5 mm", "close", 5.0), ("close 10 mm", "close", 10.0), ("propagate", "dilate", float("inf"))):
        changed = []

        def run():
            changed[:] = [eng.morph_dev(ld, op, r, spacing=SPACING, out=res)[1]]

        report(out, what, eng, run, args.reps)
        out(f"{'':24s} voxels added {changed[0][0]}, removed {changed[0][1]}")
    if not args.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            out("scipy is not installed: no host figure")
        else:
            S = lab > 0
            t0 = time.perf_counter()
            D = ndimage.distance_transform_edt(~S, sampling=SPACING) <= 10.0
            C = ndimage.distance_transform_edt(D, sampling=SPACING) > 10.0
            dt = time.perf_counter() - t0
            dev = eng.morph(lab, "close", 10.0, spacing=SPACING)[0]
            # (scipy measures the erosion's distance to background voxels only INSIDE the volume as well; float64 against float32
            # distances may differ on voxels at exactly 10 mm)
            out(f"scipy.ndimage on the CPU, 10 mm closing by two distance_transform_edt (not binary_closing, which is slower still): {dt * 1e3:.0f} ms (one pass); "
                f"voxels that differ from the device's closing: {int(((dev > 0) != (C | S)).sum())}")
    for d in (ld, fd, d2, near, res):
        d.free()
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
