"""What the per-label statistics cost (lm_label_stats_dev, LMInferer.apply_with_stats) on the bench workload, 300 x 512 x 512:

  1. the kernels alone (engine profiler, HIP events): label_stats (one read of labels + volume, LDS histograms) and
     label_stats_reduce (slab reduction), for R231 labels (2 histogram labels) and LTRCLobes labels (5: two label groups), int16
     and float32 volumes; algorithmic bytes (labels + volume read once) per second against the 8 TB/s HBM peak;
  2. the whole call (host clock: launches, the copy of the result to the host, the stream synchronise);
  3. lm_apply_dev on the same volume, for scale; LMInferer.apply against apply_with_stats host to host.

Medians of `--reps` passes after two warm-up passes.  Synthetic weights (lungmask_amd.synthetic, head 'lunglike' as bench.py)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import LMInferer  # noqa: E402
from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402

PEAK = 8.0e12  # HBM3E peak, bytes/s


def median_ms(fn, reps, sync):
    for _ in range(2):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    n, h, w = args.n, 512, 512
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    print(f"volume {n} x {h} x {w}, medians of {args.reps} (min..max)")
    eng.load_state_dict(0, syn.synthetic_state_dict(3, head="lunglike"))
    lab3 = eng.apply(0, vol)
    # LTRCLobes-like labels: label 2 of R231 split in two along z (lobes 1, 2), label 1 in three (lobes 3, 4, 5)
    z = np.arange(n)[:, None, None]
    lab6 = np.where(lab3 == 2, 1 + (z >= n // 2), np.where(lab3 == 1, 3 + (z >= n // 3) + (z >= (2 * n) // 3), 0)).astype(np.uint8)
    for what, lab, k in (("R231", lab3, 3), ("LTRCLobes", lab6, 6)):
        counts = np.bincount(lab.ravel(), minlength=k)
        print(f"{what}: voxels per label {counts.tolist()} ({(lab > 0).mean() * 100:.1f} % labelled)")
        ld = eng.to_device(lab)
        for dt in (np.int16, np.float32):
            vd = eng.to_device(vol.astype(dt))
            eng.label_stats_dev(ld, vd, k)
            eng.profile(True)
            eng.profile_reset()
            for _ in range(args.reps):
                eng.label_stats_dev(ld, vd, k)
            eng.sync()
            prof = {s["name"]: s for s in eng.profile_read()}
            eng.profile(False)
            main_ms = prof["label_stats"]["total_ms"] / prof["label_stats"]["launches"]
            red_ms = prof["label_stats_reduce"]["total_ms"] / prof["label_stats_reduce"]["launches"]
            nbytes = vol.size * (1 + np.dtype(dt).itemsize)
            call = median_ms(lambda: eng.label_stats_dev(ld, vd, k), args.reps, lambda: None)
            print(f"[kernel] {what:9s} {np.dtype(dt).name:7s} label_stats {main_ms * 1e3:7.1f} us  reduce {red_ms * 1e3:6.1f} us  "
                  f"{nbytes / 1e6:6.1f} MB read once -> {nbytes / main_ms / 1e9:5.2f} TB/s = {nbytes / main_ms / 1e9 / (PEAK / 1e12) * 100:5.1f} % "
                  f"of 8 TB/s;  whole call {call[0]:.3f} ms ({call[1]:.3f}..{call[2]:.3f})")
            vd.free()
        ld.free()
    vd = eng.to_device(vol)
    out = eng.empty(vol.shape, np.uint8)
    base = median_ms(lambda: eng.apply_dev(0, vd, out), args.reps, eng.sync)
    print(f"[device] R231      lm_apply_dev {base[0]:8.2f} ms ({base[1]:.2f}..{base[2]:.2f})")
    vd.free()
    out.free()
    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=eng)
    a = median_ms(lambda: inf.apply(vol), max(3, args.reps // 2), lambda: None)
    b = median_ms(lambda: inf.apply_with_stats(vol), max(3, args.reps // 2), lambda: None)
    print(f"[host]   R231      LMInferer.apply            {a[0]:8.2f} ms ({a[1]:.2f}..{a[2]:.2f})")
    print(f"[host]   R231      LMInferer.apply_with_stats {b[0]:8.2f} ms ({b[1]:.2f}..{b[2]:.2f})  +{b[0] - a[0]:.2f} ms")
    t0 = time.perf_counter()
    lab = inf.apply(vol)
    for k in (1, 2):  # what users do today: numpy on the host
        v = vol[lab == k]
        np.bincount(np.clip(v.astype(np.int64), -1024, 3071) + 1024, minlength=4096)
        np.percentile(v, 15)
    print(f"[host]   numpy per-label histogram + percentile on the host after apply: {(time.perf_counter() - t0) * 1e3:.1f} ms (one pass)")
    inf.close()
    eng.close()


if __name__ == "__main__":
    main()
