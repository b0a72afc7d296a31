"""What the component analysis costs (lm_components_dev, lm_component_table_dev) on the lung-like 300 x 512 x 512 label volume and the
phantom of lungmask_amd.synthetic (the phantom under the 'lunglike' head, as bench.py):

  (a) hu < -950 inside the lungs, per label;
  (b) a deliberately noisy selection -- the phantom plus a fixed pseudo-random offset per voxel, thresholded at a low percentile of
      the lung's values (the first of 20, 30, 10, 40, 5 that gives >= 10^5 components; the count is reported): the many-root regime
      the engine's labelling was not written for;
  (c) per_label=False with an open range: one giant component.

Per case: whole calls (wall clock, the read-back of the table included) and the kernels from the engine profiler (HIP events), split
into select, ccl_label, ccl_rank and table.  Medians of `--reps` calls after two warm-up calls.  Where scipy is present (--no-scipy
skips it) scipy.ndimage.label + find_objects + sum run once on the same selection on this machine's CPU, for context.  Measured, not
tuned: the figures set no bar."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-scipy", action="store_true", help="skip the host figure (scipy.ndimage.label + find_objects + sum, one pass per case)")
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "components_timing.log"))
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
    out(f"labels {n} x {h} x {w}, {(lab > 0).mean() * 100:.1f} % labelled, labels {sorted(np.unique(lab).tolist())}, image {vol.dtype}; "
        f"medians of {args.reps} (min..max) after 2 warm-up calls")
    rng = np.random.default_rng(0)
    noisy = (vol.astype(np.int32) + rng.integers(-400, 401, vol.shape, dtype=np.int32)).astype(np.int16)
    ld = eng.to_device(lab)
    ids = eng.empty(lab.shape, np.int32)
    nd = eng.to_device(noisy)
    cut, pct, best = None, None, -1
    for q in (20, 30, 10, 40, 5):
        c = int(np.percentile(noisy[lab > 0], q))
        total = eng.components_dev(ld, nd, hu_range=(None, c - 1), out=ids)[1]
        if total > best:
            cut, pct, best = c, q, total
        if total >= 10 ** 5:
            break
    nd.free()
    out(f"(b): percentile {pct} of the noisy lung values, {best} components")
    cases = (("(a) hu < -950 per label", vol, dict(hu_range=(None, -951), per_label=True)),
             (f"(b) noisy, hu < {cut} per label", noisy, dict(hu_range=(None, cut - 1), per_label=True)),
             ("(c) open range, one region", vol, dict(hu_range=None, per_label=False)))
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for what, image, kw in cases:
        vd = eng.to_device(image)
        seen = {}

        def run():
            _, total, counts = eng.components_dev(ld, vd, out=ids, **kw)
            rows, _ = eng.component_table_dev(ids, ld, vd, cap=total)
            seen.update(total=total, selected=int(counts[2].sum()), largest=int(rows["voxels"].max()) if total else 0)

        call = median_ms(run, args.reps)
        ks = kernels_ms(eng, run, args.reps)
        parts = "  ".join(f"{k} {v:.3f}" for k, v in ks.items())
        out(f"{what:34s} components {seen['total']:8d}  selected {seen['selected']:9d}  largest {seen['largest']:9d}")
        out(f"{'':34s} whole calls {call[0]:8.3f} ms ({call[1]:.3f}..{call[2]:.3f})   kernels {sum(ks.values()):8.3f} ms:  {parts}")
        if ndimage is not None and not args.no_scipy:
            sel = lab > 0
            lo, hi = (None, None) if kw["hu_range"] is None else kw["hu_range"]
            if hi is not None:
                sel &= image <= hi
            t0 = time.perf_counter()
            if kw["per_label"]:
                tot = 0
                for k in np.unique(lab[lab > 0]):
                    li, c = ndimage.label(sel & (lab == k))
                    ndimage.find_objects(li)
                    ndimage.sum(image, li, np.arange(1, c + 1))
                    tot += c
            else:
                li, tot = ndimage.label(sel)
                ndimage.find_objects(li)
                ndimage.sum(image, li, np.arange(1, tot + 1))
            dt = time.perf_counter() - t0
            out(f"{'':34s} scipy.ndimage label + find_objects + sum on the CPU: {dt * 1e3:.0f} ms (one pass), {tot} components"
                f"{'' if tot == seen['total'] else '  (DIFFERENT COUNT)'}")
        vd.free()
    if ndimage is None:
        out("scipy is not installed: no host figure")
    for d in (ld, ids):
        d.free()
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
