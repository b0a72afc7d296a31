"""What the surface mesh costs (lm_mesh_plan_dev + lm_mesh_dev) on the bench workload, 300 x 512 x 512 with lung-like labels: the
whole lung and one label alone, smooth 0 and 10.  Per case: V, Q, the bytes the passes must move (the labels of the box read twice,
the cell -> vertex map and the outputs written once, per smoothing pass the vertices read and written), each pass's time from the
engine profiler (HIP events) with its share, achieved GB/s against the 8 TB/s HBM peak, and the whole mesh_dev call on the host clock
(the box and count read-backs, two allocations, the launches, the synchronise).  Medians of `--reps` passes after two warm-up passes.
Synthetic weights (lungmask_amd.synthetic, head 'lunglike' as bench.py)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

PEAK = 8.0e12  # HBM3E peak, bytes/s
PASSES = ("mask_bbox", "roi_keepmask", "mesh_count", "mesh_scan", "mesh_emit", "mesh_quad_ids", "mesh_smooth")


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
    print(f"labels {n} x {h} x {w}: {(lab > 0).mean() * 100:.1f} % labelled, label values {sorted(int(v) for v in np.unique(lab))}; "
          f"medians of {args.reps}")
    ld = eng.to_device(lab)
    for what, keep in (("whole lung", None), ("label 1", [1])):
        for smooth in (0, 10):
            def run():
                verts, quads, info = eng.mesh_dev(ld, keep=keep, smooth=smooth)
                eng.sync()
                verts.free()
                quads.free()
                return info

            for _ in range(2):
                info = run()
            eng.profile(True)
            eng.profile_reset()
            for _ in range(args.reps):
                run()
            prof = {s["name"]: s for s in eng.profile_read()}
            eng.profile(False)
            ms = {k: prof[k]["total_ms"] / args.reps for k in PASSES if k in prof}
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                run()
                ts.append((time.perf_counter() - t0) * 1e3)
            b = info["bbox"]
            box = (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4])
            cells = (b[1] - b[0] + 1) * (b[3] - b[2] + 1) * (b[5] - b[4] + 1)
            nv, nq = info["n_vertices"], info["n_quads"]
            must = {"mesh_count": box, "mesh_emit": box + 4 * cells + 12 * nv + 16 * nq, "mesh_quad_ids": 32 * nq,
                    "mesh_smooth": smooth * 2 * 24 * nv}
            total = sum(ms.values())
            print(f"[{what}, smooth {smooth}] box {b} ({box / 1e6:.1f} M voxels, {cells / 1e6:.1f} M cells)  V {nv}  Q {nq}  "
                  f"read {(2 * box) / 1e6:.1f} MB  written {(4 * cells + 12 * nv + 16 * nq) / 1e6:.1f} MB")
            for k in PASSES:
                if k in ms:
                    rate = f"  {must[k] / 1e6:7.1f} MB -> {must[k] / ms[k] / 1e6:7.1f} GB/s = {must[k] / ms[k] * 1e3 / PEAK * 100:4.1f} % of 8 TB/s" \
                        if must.get(k) else ""
                    print(f"    {k:14s} {ms[k] * 1e3:8.1f} us  {ms[k] / total * 100:5.1f} %{rate}")
            print(f"    device passes {total * 1e3:.1f} us; whole mesh_dev call {np.median(ts):.3f} ms ({min(ts):.3f}..{max(ts):.3f})", flush=True)
    t0 = time.perf_counter()
    z, y, x = np.nonzero(lab)
    print(f"[host] np.nonzero of the labels alone (what a host mesher starts from): {(time.perf_counter() - t0) * 1e3:.0f} ms")
    ld.free()
    eng.close()


if __name__ == "__main__":
    main()
