"""What a registration costs (lm_joint_hist_dev, lungmask_amd.registration) on the bench volume, the 300 x 512 x 512 int16 phantom
with spacing (1.25, 0.7, 0.7) mm against itself under a small rotation, 32 bins:

  1. one evaluation at the lattice steps of the 8, 4 and 2 mm levels and at step 1, unmasked and inside the lung-like labels dilated
     by 10 mm: the histogram kernel and the reduction separately (engine profiler, HIP events around each launch), and the whole
     call with its read-back of bins^2 + 4 integers (host clock);
  2. beside each, lm_resample_dev (linear, float32) writing the same number of output voxels under the same map: the same gather
     without the histogram;
  3. a whole default register(..., "rigid") of the pair: wall time, evaluations, and the share of it inside kernels.

Medians of `--reps` passes after two warm-up passes, in one process."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import registration as reg  # noqa: E402
from lungmask_amd import resample as rs  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

SPACING = (1.25, 0.7, 0.7)


def profiled(eng, run, reps, prefix):
    for _ in range(2):
        run()
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        run()
    prof = {s["name"]: s["total_ms"] / s["launches"] for s in eng.profile_read() if s["launches"] and s["name"].startswith(prefix)}
    eng.profile(False)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append((time.perf_counter() - t0) * 1e3)
    return prof, float(np.median(ts))


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
    rim = eng.morph(lab, "dilate", 10.0, spacing=SPACING)[0]
    grid = rs.Grid.of(vol, SPACING)
    centre = grid.index_to_physical([(e - 1) / 2.0 for e in grid.shape])
    small = rs.Affine.from_parameters("rigid", (1.0, -0.5, 1.5, 1.0, -2.0, 1.5), centre)
    A, b = rs.index_map(grid, grid, small)
    print(f"volume {n} x {h} x {w} int16, spacing {SPACING} mm, against itself under a rotation of (1, -0.5, 1.5) degrees; "
          f"{(rim > 0).mean() * 100:.1f} % inside the dilated labels; 32 bins; medians of {args.reps}", flush=True)
    vd, ld = eng.to_device(vol), eng.to_device(rim)
    out = eng.empty((32 * 32 + 4,), np.int64)
    for level in (8.0, 4.0, 2.0, None):
        step = (1, 1, 1) if level is None else reg._level_step(level, SPACING)
        dims = [(e + s - 1) // s for e, s in zip(vol.shape, step)]
        for what, labels in (("unmasked", None), ("lungs + 10 mm", ld)):
            def run():
                eng.joint_hist_dev(vd, vd, A, b, 32, step=step, labels=labels, out=out)
                eng.sync()
                return out.download()

            prof, call = profiled(eng, run, args.reps, "jh_")
            counts = eng.split_joint_hist(run(), 32)[1]
            print(f"[hist]     step {step} ({'step 1' if level is None else f'{level:g} mm'}) {what:14s} {counts['sampled']:9d} samples: "
                  f"jh_linear {prof.get('jh_linear', 0.0) * 1e3:8.1f} us, jh_reduce {prof.get('jh_reduce', 0.0) * 1e3:6.1f} us, "
                  f"call + read-back {call * 1e3:8.1f} us", flush=True)
        # the same gather without the histogram: the lattice as an output grid (A, b composed with o = step * k)
        res = eng.empty(dims, np.float32)
        As = A * np.asarray(step, np.float64)[None, :]

        def run_rs():
            eng.resample_dev(vd, As, b, dims, "linear", -1024, np.float32, out=res)
            eng.sync()

        prof, call = profiled(eng, run_rs, args.reps, "rs_")
        print(f"[resample] step {step}: {int(np.prod(dims)):9d} output voxels, linear float32: rs_linear {prof.get('rs_linear', 0.0) * 1e3:8.1f} us, "
              f"call {call * 1e3:8.1f} us", flush=True)
        res.free()
    out.free()
    ld.free()
    vd.free()
    # a whole registration: the moving volume is the phantom resampled under the small rotation
    moving = rs.resample_image(vol, grid, small.inverse(), order=1, dtype=np.int16, spacing=SPACING, engine=eng).array
    for labels, what in ((None, "unmasked"), (rim, "lungs + 10 mm")):
        ts, ks = [], []
        for rep in range(3):  # the wall time without the profiler's events, the kernels' share from a run with them
            t0 = time.perf_counter()
            r = reg.register(vol, moving, "rigid", labels=labels, spacing=SPACING, moving_spacing=SPACING, engine=eng)
            ts.append(time.perf_counter() - t0)
        eng.profile(True)
        eng.profile_reset()
        reg.register(vol, moving, "rigid", labels=labels, spacing=SPACING, moving_spacing=SPACING, engine=eng)
        ks.append(sum(s["total_ms"] for s in eng.profile_read() if s["name"].startswith("jh_")) / 1e3)
        eng.profile(False)
        d = np.linalg.norm(r.transform.apply(centre + 50.0 * np.eye(3)) - small.apply(centre + 50.0 * np.eye(3)), axis=1).max()
        print(f"[register] rigid, levels 8 / 4 / 2 mm, {what:14s}: {np.median(ts):6.3f} s wall (upload of both volumes included), "
              f"{r.evaluations} evaluations ({[lv['evaluations'] for lv in r.levels]} per level), {np.median(ks):6.3f} s inside kernels "
              f"= {100.0 * np.median(ks) / np.median(ts):4.1f} %; error 50 mm from the centre {d:.3f} mm", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
