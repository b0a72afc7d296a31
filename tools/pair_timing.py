"""What the paired analysis costs (lm_pair_map_dev, lungmask_amd.pairs) on the bench volume's grid, 300 x 512 x 512 voxels with
spacing (1.25, 0.7, 0.7) mm, through the smooth field of 2 mm amplitude of tools/deform_timing.py, against the two calls it fuses,
in the same run:

  1. lm_pair_map_dev with the three maps, inside the model's labels of the phantom;
  2. the same with the table only (no map is written);
  3. the same as 1. with EVERY voxel labelled 1: the whole grid is analysed, which is the byte count below and the worst case for the
     table -- every lane of every wave holds the same label;
  4. lm_warp_dev's linear gather (int16 -> float32) through the field;
  5. lm_jacobian_dev of the field.

The comparison is 3. (and 1.) against 4. + 5.: what a caller ran before, ahead of any per-label arithmetic on the host.  By bytes
the fused call streams about 26 per voxel (2 fixed, 1 label, 12 field, a 2-byte gather, 9 written), the two separate calls 34
(12 + 2 + 4 and 12 + 4).

Kernel times come from the engine profiler (HIP events around each launch), call times from the host clock around call + sync.
Medians of `--reps` passes after two warm-up passes, in one process; the GPU's clocks and the host's load average are recorded."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402
from tools.deform_timing import SPACING, profiled, smooth_field  # noqa: E402
from tools.vessel_timing import clock_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pair_timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "w")

    def out(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    n, h, w = args.n, args.hw, args.hw
    shape = (n, h, w)
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    eng.load_state_dict(0, syn.synthetic_state_dict(3, head="lunglike"))
    lab = eng.apply(0, vol)
    moving = np.ascontiguousarray(np.roll(vol, (1, 2, -3), (0, 1, 2)))  # (another volume: the gather does not hit the fixed one's lines)
    field = smooth_field(shape, 2.0)
    total = vol.size
    out(f"grid {n} x {h} x {w}, spacing {SPACING} mm, a smooth field of 2 mm, {(lab > 0).mean() * 100:.1f} % of the voxels labelled; medians of "
        f"{args.reps} after two warm-ups, one process; load average of the host {os.getloadavg()}, {os.cpu_count()} CPUs")
    for ln in clock_lines():
        out("clock: " + ln)
    I, z = np.eye(3), np.zeros(3)
    fd, md, ud, ld = eng.to_device(vol), eng.to_device(moving), eng.to_device(field), eng.to_device(lab)
    ones = eng.to_device(np.ones(shape, np.uint8))
    cls, chg, jac = eng.empty(shape, np.uint8), eng.empty(shape, np.float32), eng.empty(shape, np.float32)
    table, counts = eng.empty((4, nat.LM_PAIR_COLS), np.int64), eng.empty((2,), np.int64)
    times = {}

    def report(tag, what, prof, call, name, bytes_per_voxel, voxels=total):
        k = prof.get(name, 0.0)
        times[tag] = k
        out(f"[{tag:8s}] {what:62s} {name} {k * 1e3:8.1f} us, call {call * 1e3:8.1f} us; {bytes_per_voxel:4.1f} B/voxel streamed = "
            f"{voxels * bytes_per_voxel / (k * 1e-3) / 1e12 if k else 0.0:5.2f} TB/s")

    def pair(labels, maps):
        def run():
            eng.pair_map_dev(fd, labels, md, ud, I, z, table, 4, spacing=SPACING, classes=cls if maps else None, change=chg if maps else None,
                             jacobian=jac if maps else None)
            eng.sync()
        return run

    frac = float((lab > 0).mean())
    report("pair", "lm_pair_map_dev, three maps, the model's labels", *profiled(eng, pair(ld, True), args.reps, ("pm_",)), "pm_pair",
           1 + 9 + frac * 16)
    rows = table.download()
    report("table", "lm_pair_map_dev, the table only, the model's labels", *profiled(eng, pair(ld, False), args.reps, ("pm_",)), "pm_pair",
           1 + frac * 16)
    report("pair-all", "lm_pair_map_dev, three maps, every voxel labelled 1", *profiled(eng, pair(ones, True), args.reps, ("pm_",)), "pm_pair", 26.0)
    report("tab-all", "lm_pair_map_dev, the table only, every voxel labelled 1", *profiled(eng, pair(ones, False), args.reps, ("pm_",)), "pm_pair",
           17.0)
    whole = table.download()

    def run_warp():
        eng.warp_dev(md, ud, I, z, shape, "linear", -1024, np.float32, SPACING, out=chg)
        eng.sync()

    report("warp", "lm_warp_dev linear int16 -> float32", *profiled(eng, run_warp, args.reps, ("df_",)), "df_linear", 18.0)

    def run_jacobian():
        eng.jacobian_dev(ud, SPACING, out=jac, counts=counts)
        eng.sync()

    report("jacobian", "lm_jacobian_dev", *profiled(eng, run_jacobian, args.reps, ("df_",)), "df_jacobian", 16.0)
    for d in (counts, table, jac, chg, cls, ones, ld, ud, md, fd):
        d.free()
    both = times["warp"] + times["jacobian"]
    if both and times["pair-all"]:
        out(f"[ratio   ] warp + Jacobian {both * 1e3:.1f} us; the fused call on the whole grid {times['pair-all'] / both:.2f} x of it (26 against 34 bytes "
            f"per voxel: 0.76 x), inside the model's labels {times['pair'] / both:.2f} x; the table only {times['tab-all'] / both:.2f} x and "
            f"{times['table'] / both:.2f} x")
    out(f"[table   ] the model's labels: " + "; ".join(f"label {k}: {int(r[0])} voxels, {int(r[1])} analysed, mean J {r[5] / 2 ** 20 / max(int(r[1]), 1):.4f}"
                                                      for k, r in enumerate(rows) if r[0]) +
        f"; every voxel: {int(whole[1][1])} analysed of {int(whole[1][0])}, {int(whole[1][2])} outside")
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
