"""What the lung ROI costs (lm_roi_dev, LMInferer.apply_roi) on the bench workload, 300 x 512 x 512 with R231-like labels:

  1. lm_roi_dev alone (engine profiler, HIP events: roi_resample, and with dilate_mm > 0 roi_keepmask + the three EDT passes) for the
     crop and the 1 mm isotropic form, with and without dilate_mm, float32 / float16 / int16 output; achieved GB/s over the
     algorithmic bytes (the box of the source + its labels read once, both outputs written once) against the 8 TB/s HBM peak;
  2. the whole roi_dev call (host clock: the box read-back, the two allocations, the launch, the stream synchronise);
  3. LMInferer.apply against apply_roi host to host, and apply plus the scipy.ndimage recipe on this machine's CPU.

Medians of `--reps` passes after two warm-up passes.  Synthetic weights (lungmask_amd.synthetic, head 'lunglike' as bench.py)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import LMInferer  # noqa: E402
from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

PEAK = 8.0e12  # HBM3E peak, bytes/s
SPACING = (1.25, 0.7, 0.7)


def median_ms(fn, reps, sync):
    for _ in range(2):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def scipy_recipe(vol, lab, spacing, spacing_out, margin_mm=5.0, fill=-1024):
    """What callers run on the host today: box, margin, zoom (order 1 / order 0), blank."""
    from scipy import ndimage

    z, y, x = np.nonzero(lab)
    m = [int(np.ceil(margin_mm / s)) for s in spacing]
    sl = tuple(slice(max(int(a.min()) - k, 0), min(int(a.max()) + 1 + k, n)) for a, k, n in zip((z, y, x), m, lab.shape))
    img, lb = vol[sl].astype(np.float32), lab[sl]
    if spacing_out is not None:
        zoom = [s / spacing_out for s in spacing]
        img, lb = ndimage.zoom(img, zoom, order=1), ndimage.zoom(lb, zoom, order=0)
    return np.where(lb > 0, img, np.float32(fill))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip part 3 (the host-to-host calls and the scipy recipe)")
    args = ap.parse_args()
    n, h, w = args.n, 512, 512
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    print(f"volume {n} x {h} x {w} int16, spacing {SPACING} mm, medians of {args.reps} (min..max)")
    eng.load_state_dict(0, syn.synthetic_state_dict(3, head="lunglike"))
    lab = eng.apply(0, vol)
    print(f"R231-like labels: {(lab > 0).mean() * 100:.1f} % labelled")
    ld, vd = eng.to_device(lab), eng.to_device(vol)
    for what, spo in (("crop", None), ("1 mm iso", 1.0)):
        for dilate in (0.0, 3.0):
            for dt in (np.float32, np.float16, np.int16):
                kw = dict(spacing=SPACING, spacing_out=spo, dilate_mm=dilate, dtype=dt)

                def run():
                    img, ol, info = eng.roi_dev(vd, ld, **kw)
                    eng.sync()
                    img.free()
                    ol.free()
                    return info

                info = run()
                eng.profile(True)
                eng.profile_reset()
                for _ in range(args.reps):
                    run()
                prof = {s["name"]: s for s in eng.profile_read()}
                eng.profile(False)
                ms = {k: prof[k]["total_ms"] / prof[k]["launches"] for k in prof}
                b = info["bbox"]
                box = (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4])
                nout = int(np.prod(info["out_dims"]))
                nbytes = box * (vol.itemsize + 1) + nout * (np.dtype(dt).itemsize + 1)
                call = median_ms(run, args.reps, lambda: None)
                k_ms = ms["roi_resample"]
                extra = "".join(f"  {k} {ms[k] * 1e3:.1f} us" for k in ("roi_keepmask", "edt_x", "edt_y", "edt_z", "mask_bbox") if k in ms)
                print(f"[kernel] {what:8s} dilate {dilate:3.1f} {np.dtype(dt).name:7s} box {b} -> {info['out_dims']}: roi_resample "
                      f"{k_ms * 1e3:7.1f} us, {nbytes / 1e6:6.1f} MB -> {nbytes / k_ms / 1e6:7.1f} GB/s = {nbytes / k_ms / 1e3 / PEAK * 100:4.1f} % of 8 TB/s;"
                      f"{extra};  whole call {call[0]:.3f} ms ({call[1]:.3f}..{call[2]:.3f})", flush=True)
    ld.free()
    vd.free()
    if not args.no_host:
        inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=eng)
        reps = max(3, args.reps // 2)
        a = median_ms(lambda: inf.apply(vol), reps, lambda: None)
        print(f"[host]   LMInferer.apply                         {a[0]:8.2f} ms ({a[1]:.2f}..{a[2]:.2f})")
        for what, spo in (("crop", None), ("1 mm iso", 1.0)):
            r = median_ms(lambda: inf.apply_roi(vol, spacing=SPACING, spacing_out=spo), reps, lambda: None)
            print(f"[host]   LMInferer.apply_roi {what:8s}            {r[0]:8.2f} ms ({r[1]:.2f}..{r[2]:.2f})  +{r[0] - a[0]:.2f} ms")
            labels = inf.apply(vol)
            t0 = time.perf_counter()
            scipy_recipe(vol, labels, SPACING, spo)
            print(f"[host]   scipy.ndimage recipe {what:8s} on the CPU after apply: {(time.perf_counter() - t0) * 1e3:8.1f} ms (one pass)", flush=True)
        inf.close()
    eng.close()


if __name__ == "__main__":
    main()
