"""What resampling costs (lm_resample_dev, lm_spline_prefilter_dev) on the bench volume, the 300 x 512 x 512 int16 phantom with
spacing (1.25, 0.7, 0.7) mm brought to 1 mm isotropic (374 x 358 x 358):

  1. per kernel (engine profiler, HIP events around each launch): the conversion to float64 and the three prefilter passes
     separately, the cubic gather, the linear gather, label-linear and nearest labels -- milliseconds, the algorithmic bytes (what
     the kernel must read and write once: ProfScope's figure) and the achieved bytes/s;
  2. beside each, a device-to-device copy that moves the same number of bytes (half read, half written), timed with HIP events in
     the same run: what the memory system gives a kernel with no arithmetic and perfect access at that size;
  3. the whole calls (host clock around resample_dev and a stream synchronise).

Medians of `--reps` passes after two warm-up passes."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import resample as rs  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

SPACING = (1.25, 0.7, 0.7)


def copy_ms(nbytes, reps):
    """Median milliseconds of a device-to-device copy with `nbytes` of traffic (nbytes / 2 read, nbytes / 2 written)."""
    n = max(int(nbytes) // 2, 1)
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    a.zero_()
    for _ in range(2):
        b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b.copy_(a)
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    n, h, w = args.n, 512, 512
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    eng.load_state_dict(0, syn.synthetic_state_dict(3, head="lunglike"))
    lab = eng.apply(0, vol)
    src = rs.Grid.of(vol, SPACING)
    out = rs.Grid.isotropic(src, 1.0)
    A, b = rs.index_map(src, out)
    print(f"volume {n} x {h} x {w} int16, spacing {SPACING} mm -> {out.shape} at 1 mm; {(lab > 0).mean() * 100:.1f} % labelled; "
          f"medians of {args.reps}", flush=True)
    vd, ld = eng.to_device(vol), eng.to_device(lab)
    runs = (("cubic float32", vd, "cubic", np.float32), ("cubic float16", vd, "cubic", np.float16), ("linear float32", vd, "linear", np.float32),
            ("linear int16", vd, "linear", np.int16), ("label-linear", ld, "label_linear", np.uint8), ("nearest labels", ld, "nearest", np.uint8))
    for what, sd, mode, dt in runs:
        res = eng.empty(out.shape, dt)

        def run():
            eng.resample_dev(sd, A, b, out.shape, mode, 0 if sd is ld else -1024, dt, out=res)
            eng.sync()

        for _ in range(2):
            run()
        eng.profile(True)
        eng.profile_reset()
        for _ in range(args.reps):
            run()
        prof = [s for s in eng.profile_read() if s["launches"] and s["name"].startswith("rs_")]
        eng.profile(False)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"[call]   {what:15s} whole resample_dev + sync {np.median(ts):8.3f} ms ({min(ts):.3f}..{max(ts):.3f})", flush=True)
        for s in prof:
            ms, nbytes = s["total_ms"] / s["launches"], s["bytes"] / s["launches"]
            cp = copy_ms(nbytes, args.reps)
            print(f"[kernel] {what:15s} {s['name']:16s} {ms:8.3f} ms  {nbytes / 1e6:8.1f} MB  {nbytes / ms / 1e6:8.1f} GB/s;  "
                  f"copy of the same bytes {cp:8.3f} ms  {nbytes / cp / 1e6:8.1f} GB/s;  kernel / copy = {ms / cp:5.2f}", flush=True)
        res.free()
    vd.free()
    ld.free()
    eng.close()


if __name__ == "__main__":
    main()
