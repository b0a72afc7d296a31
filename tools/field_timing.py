"""What the field kernel costs (lm_field_combine_dev, lungmask_amd.deformable.invert) on the bench volume's grid, 300 x 512 x 512
voxels with spacing (1.25, 0.7, 0.7) mm, with the smooth field of 2 mm amplitude of tools/deform_timing.py:

  1. lm_warp_dev's linear gather (int16 -> float32) through the field: the yardstick, in the same run -- it reads a 12-byte
     coordinate, gathers one int16 and writes 4 bytes per voxel;
  2. one lm_field_combine_dev call in the inversion pattern (coord = ref = w, src = u, beta = -1): 12 + 12 bytes read (ref is coord:
     one stream), three float32 components gathered, 12 bytes written;
  3. one call in the composition pattern (add = coord = u1, src = u2, a rotation and a small index map): the same streams;
  4. a whole `invert` of the field at the default tolerance: wall time with the upload and the download, iterations, and the part
     inside kernels.

Kernel times come from the engine profiler (HIP events around each launch), call times from the host clock around call + sync.
Medians of `--reps` passes after two warm-up passes, in one process; the host's load average is printed beside them."""
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
from tools.deform_timing import SPACING, profiled, smooth_field  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    n, h, w = args.n, args.hw, args.hw
    shape = (n, h, w)
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    grid = rs.Grid.of(vol, SPACING)
    centre = grid.index_to_physical([(e - 1) / 2.0 for e in grid.shape])
    small = rs.Affine.from_parameters("rigid", (1.0, -0.5, 1.5, 1.0, -2.0, 1.5), centre)
    A, b = rs.index_map(grid, grid, small)
    R = dfm.compose_rotation(grid, small, grid)
    field = smooth_field(shape, 2.0)
    total = vol.size
    print(f"grid {n} x {h} x {w}, spacing {SPACING} mm, a smooth field of 2 mm; medians of {args.reps} after two warm-ups, one process; "
          f"load average of the host {os.getloadavg()}, {os.cpu_count()} CPUs", flush=True)
    vd, ud = eng.to_device(vol), eng.to_device(field)
    wd = eng.to_device((-field).astype(np.float32))  # (close to the inverse: the coordinates of a late iteration)
    res, out, counts = eng.empty(shape, np.float32), eng.empty(field.shape, np.float32), eng.empty((4,), np.int64)
    times = {}

    def report(tag, what, prof, call, name, bytes_per_voxel):
        k = prof.get(name, 0.0)
        times[tag] = k
        print(f"[{tag:8s}] {what:58s} {total:9d} voxels: {name} {k * 1e3:8.1f} us, call {call * 1e3:8.1f} us; {bytes_per_voxel} B/voxel streamed = "
              f"{total * bytes_per_voxel / (k * 1e-3) / 1e12 if k else 0.0:5.2f} TB/s", flush=True)

    def run_warp():
        eng.warp_dev(vd, ud, A, b, shape, "linear", -1024, np.float32, SPACING, out=res)
        eng.sync()

    report("warp", "lm_warp_dev linear int16 -> float32 (the yardstick)", *profiled(eng, run_warp, args.reps, ("df_",)), "df_linear", 12 + 2 + 4)

    def run_inversion():
        eng.field_combine_dev(ud, shape, np.eye(3), np.zeros(3), None, coord=wd, ref=wd, beta=-1.0, spacing=SPACING, out=out, counts=counts)
        eng.sync()
        return counts.download()

    report("invert", "lm_field_combine_dev, inversion step, + read-back", *profiled(eng, run_inversion, args.reps, ("fc_",)), "fc_combine",
           12 + 12 + 12)

    def run_composition():
        eng.field_combine_dev(ud, shape, A, b, R, add=wd, coord=wd, spacing=SPACING, out=out, counts=counts)
        eng.sync()
        return counts.download()

    report("compose", "lm_field_combine_dev, composition, + read-back", *profiled(eng, run_composition, args.reps, ("fc_",)), "fc_combine",
           12 + 12 + 12)
    for d in (counts, out, res, wd, ud, vd):
        d.free()
    if times.get("warp"):
        print(f"[ratio   ] to the linear warp: inversion step {times['invert'] / times['warp']:.2f} x, composition "
              f"{times['compose'] / times['warp']:.2f} x (36 against 18 bytes per voxel streamed: 2.00 x)", flush=True)
    f = dfm.DisplacementField(field, grid)
    ts = []
    for _ in range(3):  # the wall time without the profiler's events, the kernels' part from a run with them
        t0 = time.perf_counter()
        inv, info = dfm.invert(f, engine=eng)
        ts.append(time.perf_counter() - t0)
    eng.profile(True)
    eng.profile_reset()
    dfm.invert(f, engine=eng)
    kernels = sum(s["total_ms"] for s in eng.profile_read()) / 1e3
    eng.profile(False)
    ic = dfm.inverse_consistency(f, inv, engine=eng)
    print(f"[whole   ] invert at {0.01} mm: {np.median(ts):6.3f} s wall (upload of the field and download of the inverse included), "
          f"{info['iterations']} iterations, converged {info['converged']}, residuals {[round(r, 4) for r in info['residuals']]} mm, "
          f"{kernels * 1e3:7.1f} ms inside kernels; inverse consistency {ic['max_mm']:.4f} mm at most, {ic['rms_mm']:.5f} mm RMS", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
