"""What the vessel centrelines cost (lm_skeleton_dev, lm_calibre_dev, the whole vessel-tree device path) on the 300 x 512 x 512 int16
phantom of lungmask_amd.synthetic with its lung-like label volume (the phantom under the 'lunglike' head, as bench.py and
tools/vessel_timing.py), spacing (1.0, 0.7, 0.7) mm, the four default scales.

The phantom holds noise and no vessels: its vesselness stays below 0.01, and at the default threshold of 0.5 the vessel mask is empty.
`--threshold` (default 4e-4) is therefore set so that the mask holds a few per cent of the lung, what a vessel mask of a chest CT
holds -- as speckle, which is the harder input: many small components, many junctions, few long tubes.

  (a) skeleton_dev on the device-resident mask: |S|, |K|, the passes, the time per pass, per kernel (engine profiler, HIP events
      around every launch) and as a whole call; the same for the labels themselves as the object (thick: many passes);
  (b) calibre_dev (distance transform, classes, nearest class, counts) and skeleton_points_dev;
  (c) the whole device path of skeleton.vessel_tree on device-resident image and labels (filter, erosion, counts, mask, skeleton,
      classes, point list, downloads, the graph on the host), and its host part alone.

Medians of `--reps` calls after two warm-up calls."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import skeleton as sk  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402
from lungmask_amd import vessels as vs  # noqa: E402
from tools.filter_timing import kernels, median_ms  # noqa: E402
from tools.vessel_timing import SPACING, clock_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=4e-4)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "skeleton_timing.log"))
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
    edges = sk.calibre_edges_mm(sk.DEFAULT_CALIBRES_MM2)
    out(f"volume {n} x {h} x {w} {vol.dtype}, spacing {SPACING} mm, {(lab > 0).mean() * 100:.1f} % labelled; scales {sigmas_mm} mm; vessel "
        f"threshold {args.threshold:g}; class edges {[round(e, 4) for e in edges]} mm; medians of {args.reps} (min..max) after 2 warm-up calls")
    for ln in clock_lines():
        out("clock: " + ln)
    vd, ld = eng.to_device(vol), eng.to_device(lab)
    v, sc, eroded, _ = vs.analysis_dev(eng, vd, ld, sigmas_mm, args.threshold, 2.0, SPACING)
    mask = eng.vessel_mask_dev(v, eroded, args.threshold)
    for d in (v, sc, eroded):
        d.free()
    bb = eng.roi_plan_dev(mask)
    skel, info = eng.skeleton_dev(mask)
    eng.sync()
    codes = skel.download()
    out(f"vessel mask |S| = {info['selected']} voxels = {info['selected'] / max(1, int((lab > 0).sum())) * 100:.2f} % of the labelled voxels; its "
        f"box (zmin, zmax, ymin, ymax, xmin, xmax) {bb} = {(bb[1] - bb[0]) * (bb[3] - bb[2]) * (bb[5] - bb[4]) / vol.size * 100:.1f} % of the volume")
    out(f"skeleton |K| = {info['skeleton']} voxels in {info['passes']} passes (the last one empty): isolated {(codes == 1).sum()}, ends "
        f"{(codes == 2).sum()}, curve {(codes == 3).sum()}, junction {(codes >= 4).sum()}")

    def report(what, fn):
        call = median_ms(fn, args.reps)
        ks = kernels(eng, fn, args.reps)
        total = sum(x[0] for x in ks.values())
        out(f"{what:44s} whole call {call[0]:9.3f} ms ({call[1]:.3f}..{call[2]:.3f})   kernels {total:9.3f} ms")
        for k, (ms, b) in ks.items():
            out(f"{'':44s}   {k:18s} {ms:9.3f} ms" + (f"  {b / ms / 1e6:8.1f} GB/s" if ms > 0 and b > 0 else ""))
        return call[0], ks

    outk = eng.empty(vol.shape, np.uint8)

    def skeleton():
        eng.skeleton_dev(mask, out=outk)

    call, ks = report("(a) skeleton_dev", skeleton)
    per_pass = ks.get("skeleton_pass", (0.0, 0.0))[0] / info["passes"]
    out(f"(a) per pass: {per_pass:.3f} ms of kernels (48 launches), {call / info['passes']:.3f} ms of the whole call")

    # a thick object: the lungs themselves (every label >= 1), whose thinning takes as many passes as they are thick
    _, lung_info = eng.skeleton_dev(ld, out=outk)
    out(f"labels as the object: |S| = {lung_info['selected']}, |K| = {lung_info['skeleton']}, {lung_info['passes']} passes")

    def skeleton_lungs():
        eng.skeleton_dev(ld, out=outk)

    call, ks = report("(a) skeleton_dev of the labels", skeleton_lungs)
    out(f"(a) per pass: {ks.get('skeleton_pass', (0.0, 0.0))[0] / lung_info['passes']:.3f} ms of kernels (48 launches), "
        f"{call / lung_info['passes']:.3f} ms of the whole call")

    def calibre():
        cls, _, d2 = eng.calibre_dev(skel, mask, edges, spacing=SPACING, lab=ld, return_distance=True)
        cls.free()
        d2.free()

    report("(b) calibre_dev", calibre)
    d2 = eng.calibre_dev(skel, mask, edges, spacing=SPACING, lab=ld, return_distance=True)
    d2[0].free()

    def points():
        eng.skeleton_points_dev(skel, d2[2])

    report("(b) skeleton_points_dev (count, then list)", points)
    index, code, d2_points, _ = eng.skeleton_points_dev(skel, d2[2])
    d2[2].free()

    def tree():
        sk.tree_dev(eng, vd, ld, sk.DEFAULT_CALIBRES_MM2, SPACING, None, sigmas_mm=sigmas_mm, threshold=args.threshold, erode_mm=2.0)

    report("(c) vessel_tree device path, whole", tree)
    lab_points = lab.ravel()[index]
    counts = np.zeros((16, 9), np.int64)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        sk.finalize_tree(vol.shape, index, code, d2_points, lab_points, counts, sk.DEFAULT_CALIBRES_MM2, SPACING)
        ts.append((time.perf_counter() - t0) * 1e3)
    out(f"(c) of which the graph on the host ({index.size} points): {np.median(ts):.1f} ms")
    for d in (vd, ld, mask, skel, outk):
        d.free()
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
