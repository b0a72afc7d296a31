"""What deformable registration costs (lm_warp_dev, lm_demons_step_dev, lm_jacobian_dev, lungmask_amd.deformable) on the bench volume,
the 300 x 512 x 512 int16 phantom with spacing (1.25, 0.7, 0.7) mm against itself under a small rotation and a smooth field of 2 mm
amplitude:

  1. lm_resample_dev's linear gather (float32) of the 78.6 M voxels under the rotation: the yardstick, in the same run;
  2. lm_warp_dev through the field: one linear and one cubic gather (the cubic one on prefiltered coefficients);
  3. one demons step at every voxel and inside the lung-like labels dilated by 10 mm;
  4. one smoothing of the field (three separable Gaussians of one voxel, one per component);
  5. lm_jacobian_dev with its two counts;
  6. a whole default register_deformable (levels 8 / 4 / 2 mm, 60 / 40 / 20 iterations) of the pair: wall time, iterations, and the
     share of it inside kernels.

Kernel times come from the engine profiler (HIP events around each launch), call times from the host clock around call + sync.
Medians of `--reps` passes after two warm-up passes, in one process."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import deformable as dfm  # noqa: E402
from lungmask_amd import resample as rs  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

SPACING = (1.25, 0.7, 0.7)


def profiled(eng, run, reps, prefixes):
    for _ in range(2):
        run()
    eng.profile(True)
    eng.profile_reset()
    for _ in range(reps):
        run()
    prof = {s["name"]: s["total_ms"] / reps for s in eng.profile_read() if s["launches"] and s["name"].startswith(prefixes)}
    eng.profile(False)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append((time.perf_counter() - t0) * 1e3)
    return prof, float(np.median(ts))


def smooth_field(shape, amplitude_mm):
    """One sinusoid period per axis, zero at the border, `amplitude_mm` at the most."""
    n, h, w = shape
    z, y, x = (np.arange(e, dtype=np.float32) / max(e - 1, 1) for e in shape)
    env = (np.sin(np.pi * z)[:, None, None] * np.sin(np.pi * y)[None, :, None] * np.sin(np.pi * x)[None, None, :]).astype(np.float32)
    u = np.empty((3, n, h, w), np.float32)
    u[0] = env * np.sin(2 * np.pi * y)[None, :, None]
    u[1] = env * np.sin(2 * np.pi * x)[None, None, :]
    u[2] = env * np.sin(2 * np.pi * z)[:, None, None]
    u *= np.float32(amplitude_mm / np.abs(u).max())
    return u


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
    field = smooth_field(vol.shape, 2.0)
    total = vol.size
    print(f"volume {n} x {h} x {w} int16, spacing {SPACING} mm, against itself under a rotation of (1, -0.5, 1.5) degrees and a smooth field of "
          f"2 mm; {(rim > 0).mean() * 100:.1f} % inside the dilated labels; medians of {args.reps}", flush=True)
    vd, ld, fd = eng.to_device(vol), eng.to_device(rim), eng.to_device(field)
    res = eng.empty(vol.shape, np.float32)

    def report(tag, what, prof, call, names):
        parts = ", ".join(f"{k} {prof.get(k, 0.0) * 1e3:8.1f} us" for k in names)
        print(f"[{tag:8s}] {what:46s} {total:9d} voxels: {parts}, call {call * 1e3:8.1f} us", flush=True)

    def run_resample():
        eng.resample_dev(vd, A, b, vol.shape, "linear", -1024, np.float32, out=res)
        eng.sync()

    report("resample", "lm_resample_dev linear float32 (the yardstick)", *profiled(eng, run_resample, args.reps, ("rs_",)), ["rs_linear"])

    def run_warp_linear():
        eng.warp_dev(vd, fd, A, b, vol.shape, "linear", -1024, np.float32, SPACING, out=res)
        eng.sync()

    report("warp", "lm_warp_dev linear float32 through the field", *profiled(eng, run_warp_linear, args.reps, ("df_",)), ["df_linear"])
    coef = eng.spline_prefilter_dev(vd)
    eng.sync()

    def run_warp_cubic():
        eng.warp_dev(coef, fd, A, b, vol.shape, "cubic", -1024, np.float32, SPACING, out=res)
        eng.sync()

    report("warp", "lm_warp_dev cubic float32 (coefficients given)", *profiled(eng, run_warp_cubic, args.reps, ("df_",)), ["df_cubic"])
    coef.free()
    out, counts = eng.empty(field.shape, np.float32), eng.empty((5,), np.int64)
    inv_k2 = dfm.level_inv_k2(grid, None)
    for what, labels in (("every voxel", None), ("lungs + 10 mm", ld)):
        def run_step():
            eng.demons_step_dev(vd, vd, fd, out, counts, A, b, SPACING, inv_k2, dfm.DEN_MIN, labels)
            eng.sync()
            return counts.download()

        prof, call = profiled(eng, run_step, args.reps, ("df_",))
        c = run_step()
        report("demons", f"one step, {what} ({int(c[1])} contribute), + read-back", prof, call, ["df_demons"])
    taps = dfm.field_taps(grid, None)
    n_comp = field.nbytes // 3

    def run_smooth():
        for i in range(3):
            eng.filter_dev(out.view(i * n_comp, vol.shape), kind="separable", taps=taps, out=fd.view(i * n_comp, vol.shape))
        eng.sync()

    prof, call = profiled(eng, run_smooth, args.reps, ("filter", "sep", "flt"))
    print(f"[smooth  ] {'the field, three components, sigma 1 voxel':46s} {total:9d} voxels: kernels {sum(prof.values()) * 1e3:8.1f} us "
          f"({', '.join(sorted(prof))}), call {call * 1e3:8.1f} us", flush=True)
    fd.upload(field)
    jc = eng.empty((2,), np.int64)

    def run_jacobian():
        eng.jacobian_dev(fd, SPACING, out=res, counts=jc)
        eng.sync()
        return jc.download()

    prof, call = profiled(eng, run_jacobian, args.reps, ("df_",))
    c = run_jacobian()
    report("jacobian", f"lm_jacobian_dev ({int(c[0])} folded, {int(c[1])} NaN), + read-back", prof, call, ["df_jacobian"])
    for d in (jc, out, counts, res, fd, ld, vd):
        d.free()
    # a whole registration: the moving volume is the phantom warped through the field under the rotation
    moving = dfm.warp_image(vol, dfm.DisplacementField(field, grid, small.inverse()), order=1, dtype=np.int16, spacing=SPACING, engine=eng).array
    for labels, what in ((None, "every voxel"), (rim, "lungs + 10 mm")):
        ts = []
        for rep in range(3):  # the wall time without the profiler's events, the kernels' share from a run with them
            t0 = time.perf_counter()
            r = dfm.register_deformable(vol, moving, initial=small, labels=labels, spacing=SPACING, moving_spacing=SPACING, engine=eng)
            ts.append(time.perf_counter() - t0)
        eng.profile(True)
        eng.profile_reset()
        dfm.register_deformable(vol, moving, initial=small, labels=labels, spacing=SPACING, moving_spacing=SPACING, engine=eng)
        kernels = sum(s["total_ms"] for s in eng.profile_read()) / 1e3
        eng.profile(False)
        print(f"[register] demons, levels 8 / 4 / 2 mm, {what:14s}: {np.median(ts):6.3f} s wall (upload of both volumes and download of the "
              f"field included), iterations {[lv['iterations'] for lv in r.levels]} ({[lv['stopped'] for lv in r.levels]}), level shapes "
              f"{[lv['shape'] for lv in r.levels]}, {kernels:6.3f} s inside kernels = {100.0 * kernels / np.median(ts):4.1f} %; mean squared "
              f"difference {r.mean_squared(r.initial_metric):.1f} -> {r.mean_squared(r.final_metric):.1f}, {r.folding['folded']} folded voxels",
              flush=True)
    eng.close()


if __name__ == "__main__":
    main()
