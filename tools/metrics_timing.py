"""What the label agreement metrics cost (lm_label_agreement_dev, metrics.compare_labels) on a full-size pair, 300 x 512 x 512:
a = lung-like lobes (five labels), b = a shifted by (1, 2, 3) voxels with one lobe eroded.

  1. the kernels (engine profiler, HIP events) of one call, per kind;
  2. the whole call from device arrays (label_agreement_dev) and from host arrays (compare_labels), host clock, medians of
     `--reps` after two warm-up passes;
  3. with --scipy: one run of the CPU recipe (binary_erosion + distance_transform_edt per label and direction, on the union-box crop)
     for the same pair.
`--once`: a single label_agreement_dev call after one warm-up (the process to put under a kernel trace)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import metrics  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

SPACING = (2.5, 0.7421875, 0.7421875)


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # (every form returns once the result is on the host)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def scipy_recipe(a, b, n_labels):
    import scipy.ndimage as ndi

    fp = ndi.generate_binary_structure(3, 1)
    for k in range(n_labels):
        A, B = (a >= 1, b >= 1) if k == 0 else (a == k, b == k)
        if not (A | B).any():
            continue
        z, y, x = np.nonzero(A | B)
        box = (slice(z.min(), z.max() + 1), slice(y.min(), y.max() + 1), slice(x.min(), x.max() + 1))
        A, B = A[box], B[box]
        t0 = time.perf_counter()
        sa, sb = A ^ ndi.binary_erosion(A, fp), B ^ ndi.binary_erosion(B, fp)
        dab = ndi.distance_transform_edt(~sb, sampling=SPACING)[sa]
        dba = ndi.distance_transform_edt(~sa, sampling=SPACING)[sb]
        hd95 = np.percentile(np.hstack((dab, dba)), 95)
        print(f"[scipy]  row {k}: box {A.shape}, hausdorff {max(dab.max(), dba.max()):.4f} hd95 {hd95:.4f} "
              f"{(time.perf_counter() - t0) * 1e3:9.1f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    n, h, w = args.n, 512, 512
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    eng.load_state_dict(0, syn.synthetic_state_dict(3, head="lunglike"))
    lab = eng.apply(0, vol)
    a = np.minimum((lab * 2 + (np.arange(n)[:, None, None] > n // 2)) * (lab > 0), 5).astype(np.uint8)
    b = np.zeros_like(a)
    b[1:, 2:, 3:] = a[:-1, :-2, :-3]
    m = b == 4
    p = np.pad(m, 1)
    b[m & ~(p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])] = 0
    ad, bd = eng.to_device(a), eng.to_device(b)
    raw = eng.label_agreement_dev(ad, bd, 6, SPACING, (95,))
    if args.once:
        eng.label_agreement_dev(ad, bd, 6, SPACING, (95,))
        eng.close()
        return
    print(f"pair {n} x {h} x {w}, 6 rows, spacing {SPACING}; voxels_a {raw['voxels_a'].tolist()} surfaces_a {raw['surface_a'].tolist()}")
    print(f"boxes {raw['bbox'].tolist()}")
    eng.profile(True)
    eng.profile_reset()
    eng.label_agreement_dev(ad, bd, 6, SPACING, (95,))
    eng.sync()
    prof = sorted(eng.profile_read(), key=lambda s: -s["total_ms"])
    eng.profile(False)
    total = sum(s["total_ms"] for s in prof)
    for s in prof:
        print(f"[kernel] {s['name']:18s} {s['launches']:4d} launches {s['total_ms']:9.3f} ms  {s['total_ms'] / total * 100:5.1f} %")
    print(f"[kernel] all kinds {total:9.3f} ms")
    d = median_ms(lambda: eng.label_agreement_dev(ad, bd, 6, SPACING, (95,)), args.reps)
    print(f"[device] label_agreement_dev (6 rows)       {d[0]:9.2f} ms ({d[1]:.2f}..{d[2]:.2f}), median of {args.reps}")
    d3 = median_ms(lambda: eng.label_agreement_dev(ad, bd, 1, SPACING, (95,)), args.reps)
    print(f"[device] label_agreement_dev (lung only)    {d3[0]:9.2f} ms ({d3[1]:.2f}..{d3[2]:.2f})")
    c = median_ms(lambda: metrics.compare_labels(a, b, spacing=SPACING, n_labels=6, engine=eng), args.reps)
    print(f"[host]   compare_labels from numpy arrays   {c[0]:9.2f} ms ({c[1]:.2f}..{c[2]:.2f})")
    fd = eng.to_device((a > 0).astype(np.uint8))
    out = eng.empty(a.shape, np.float32)

    def edt():
        eng.edt_dev(fd, SPACING, out=out)
        eng.sync()

    e = median_ms(edt, args.reps)
    print(f"[device] edt_dev, whole volume, features = lung {e[0]:9.2f} ms ({e[1]:.2f}..{e[2]:.2f})")
    ad.free(), bd.free(), fd.free(), out.free()
    if args.scipy:
        t0 = time.perf_counter()
        scipy_recipe(a, b, 6)
        print(f"[scipy]  the same six rows on the host: {(time.perf_counter() - t0):.1f} s (one run)")
    eng.close()


if __name__ == "__main__":
    main()
