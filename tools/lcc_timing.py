"""What the local-correlation metric of the deformable registration costs (lm_local_moments_dev, lm_lcc_step_dev,
lungmask_amd.deformable with metric="lcc") on the bench volume, the 300 x 512 x 512 phantom with spacing (1.25, 0.7, 0.7) mm, at the
pyramid's 2 mm level and on the full grid, through the smooth field of 2 mm amplitude of tools/deform_timing.py.  In the same run,
per grid:

  1. lm_local_moments_dev alone, window radius 4 (the default), and its three passes;
  2. lm_lcc_step_dev alone, at every voxel;
  3. one whole "lcc" iteration (warp, window sums, step, three field smoothings, the read-back of six integers) beside
  4. one whole "ssd" iteration (demons step, three field smoothings, the read-back of five integers);
  5. lm_warp_dev's linear gather (float32 -> float32, NaN fill) and lm_filter_dev's separable Gaussian of one field component
     (sigma one voxel) as yardsticks.

Bytes per voxel, counted once per array a kernel streams (neighbours and halos come from cache or LDS): the x pass reads f and m
(8) and writes six float64 sums (48): 56; the y and the z pass read and write the six sums: 96 each, 248 for the call; the step
reads f, m, the six sums and the field and writes the field: 4 + 4 + 48 + 12 + 12 = 80; the warp reads the field and writes a
float32 (16) and gathers from a 4-byte volume: 20; a separable pass reads and writes a float32: 8, 24 for the three.

Kernel times come from the engine profiler (HIP events around each launch), call times from the host clock around call + sync.
Medians of `--reps` passes after two warm-up passes, in one process; the GPU's clocks and the host's load average are recorded."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import deformable as dfm  # noqa: E402
from lungmask_amd import resample as rs  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402
from tools.deform_timing import SPACING, profiled, smooth_field  # noqa: E402
from tools.vessel_timing import clock_lines  # noqa: E402

RADIUS = dfm.WINDOW_LEVEL_VOXELS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--levels", type=float, nargs="+", default=[2.0, 0.0], help="level spacings in mm; 0: the full grid")
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lcc_timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def out(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    n, h, w = args.n, args.hw, args.hw
    vol = syn.phantom(n, h, w)
    moving = np.ascontiguousarray(np.roll(vol, (1, 2, -3), (0, 1, 2)))
    grid = rs.Grid.of(vol, SPACING)
    eng = nat.Engine(0)
    out(f"grid {n} x {h} x {w}, spacing {SPACING} mm, a smooth field of 2 mm, window radius {RADIUS} voxels, every voxel selected; medians of "
        f"{args.reps} after two warm-ups, one process; load average of the host {os.getloadavg()}, {os.cpu_count()} CPUs")
    for ln in clock_lines():
        out("clock: " + ln)
    for mm in args.levels:
        level = dfm.level_grid(grid, mm) if mm > 0 else grid
        one_grid(eng, out, args.reps, vol, moving, grid, level, f"{mm:g} mm level" if mm > 0 else "full grid")
    eng.close()
    log.close()


def one_grid(eng, out, reps, vol, moving, grid, level, name):
    shape, sp, total = level.shape, dfm.spacing_zyx(level), int(np.prod(level.shape))
    out(f"---- {name}: {shape[0]} x {shape[1]} x {shape[2]} = {total} voxels, spacing {tuple(round(v, 4) for v in sp)} mm")
    times = {}

    def report(tag, what, prof, call, names, bytes_per_voxel):
        k = sum(prof.get(nm, 0.0) for nm in names)
        times[tag] = (k, call)
        rate = total * bytes_per_voxel / (k * 1e-3) / 1e12 if k else 0.0
        out(f"[{tag:9s}] {what:58s} kernels {k * 1e3:9.1f} us, call {call * 1e3:9.1f} us; {bytes_per_voxel:5.1f} B/voxel = {rate:5.2f} TB/s")
        for nm in names:
            if len(names) > 1:
                out(f"            {nm:20s} {prof.get(nm, 0.0) * 1e3:9.1f} us")

    with eng.scope() as dev:
        vd, md = dev.upload(vol), dev.upload(moving)
        f, m_src = dfm._to_level(eng, vd, grid, level, dev), dfm._to_level(eng, md, grid, level, dev)
        eng.sync()
        vd.free()
        md.free()
        A, b = rs.index_map(level, level, None)
        u = dev.upload(smooth_field(shape, 2.0))
        v = dev.empty((3,) + tuple(shape), np.float32)
        c5, c6 = dev.empty((5,), np.int64), dev.empty((6,), np.int64)
        taps, inv_k2 = dfm.field_taps(level, None), dfm.level_inv_k2(level, None)
        radius = dfm.level_window(level, None)
        lcc = dfm.LccLevel(eng, f, m_src, None, None, c6, A, b, level, radius, inv_k2, dfm.DEN_MIN, dfm.VAR_EPS, dfm.A_MAX, dev)
        uc, vc = dfm._components(u), dfm._components(v)

        def run_warp():
            eng.warp_dev(m_src, u, A, b, shape, "linear", float("nan"), np.float32, sp, out=lcc.warped)
            eng.sync()

        report("warp", "lm_warp_dev linear float32 -> float32 (yardstick)", *profiled(eng, run_warp, reps, ("df_",)), ["df_linear"], 20.0)

        def run_moments():
            eng.local_moments_dev(f, lcc.warped, radius, out=lcc.sums)
            eng.sync()

        report("moments", f"lm_local_moments_dev, radius {radius}", *profiled(eng, run_moments, reps, ("lcc_",)),
               ["lcc_moments_x", "lcc_moments_y", "lcc_moments_z"], 248.0)

        def run_step():
            eng.lcc_step_dev(f, lcc.warped, lcc.sums, u, v, c6, A, b, m_src.shape, sp, inv_k2, dfm.DEN_MIN, dfm.VAR_EPS, dfm.A_MAX)
            eng.sync()

        report("step", "lm_lcc_step_dev, every voxel", *profiled(eng, run_step, reps, ("lcc_",)), ["lcc_step"], 80.0)
        counts = [int(x) for x in c6.download()]

        def run_filter():
            eng.filter_dev(vc[0], kind="separable", taps=taps, out=uc[0])
            eng.sync()

        # (v -> u and back: u is restored from v's smoothing only in shape, its values do not matter to the timing that follows)
        report("filter", "lm_filter_dev separable, one component (yardstick)", *profiled(eng, run_filter, reps, ("sep_",)), ["sep_x", "sep_y", "sep_z"], 24.0)
        u.upload(smooth_field(shape, 2.0))

        def smooth():
            for src, dst in zip(vc, uc):
                eng.filter_dev(src, kind="separable", taps=taps, out=dst)

        def run_lcc():
            lcc.step(u, v)
            smooth()
            lcc.counts()

        def run_ssd():
            eng.demons_step_dev(f, m_src, u, v, c5, A, b, sp, inv_k2, dfm.DEN_MIN)
            smooth()
            dfm._counts(eng, c5)

        lcc_names = ["df_linear", "lcc_moments_x", "lcc_moments_y", "lcc_moments_z", "lcc_step", "sep_x", "sep_y", "sep_z"]
        report("lcc-iter", 'one "lcc" iteration', *profiled(eng, run_lcc, reps, ("df_", "lcc_", "sep_")), lcc_names,
               20.0 + 248.0 + 80.0 + 72.0)
        u.upload(smooth_field(shape, 2.0))
        report("ssd-iter", 'one "ssd" iteration', *profiled(eng, run_ssd, reps, ("df_", "sep_")), ["df_demons", "sep_x", "sep_y", "sep_z"], 32.0 + 72.0)
        lk, lc = times["lcc-iter"]
        sk, sc = times["ssd-iter"]
        if sk and sc:
            out(f"[ratio    ] an lcc iteration is {lk / sk:.2f} x an ssd iteration by kernel time, {lc / sc:.2f} x by call time; the window sums are "
                f"{times['moments'][0] / lk * 100:.0f} % of its kernel time, the step {times['step'][0] / lk * 100:.0f} %, the warp "
                f"{times['warp'][0] / lk * 100:.0f} %")
        out(f"[counts   ] the step alone: {counts[0]} selected, {counts[1]} contributed, {counts[2]} outside, {counts[3]} NaN; mean squared residual "
            f"{counts[4] / 16.0 / max(counts[1], 1):.1f}, mean squared local correlation {counts[5] / float(nat.LCC_Q) / max(counts[1], 1):.4f}")
        lcc.free()


if __name__ == "__main__":
    main()
