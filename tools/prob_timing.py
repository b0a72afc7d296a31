"""What the probability maps cost (LMInferer.apply_probabilities / lm_apply_probs_dev) on the bench workload, 300 x 512 x 512:

  1. device-resident: lm_apply_dev against lm_apply_probs_dev, R231 (3 classes) and LTRCLobes (6 classes), f32 and f16 maps;
  2. host to host: LMInferer.apply against LMInferer.apply_probabilities (maps copied back into page-locked memory);
  3. the un-crop kernel alone (lm_uncrop_probs_dev on the whole volume's log-probabilities, HIP events): time, and its algorithmic
     bytes (maps written + log-probabilities read, from the shapes) per second against the 8 TB/s HBM peak.

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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    args = ap.parse_args()
    n, h, w = args.n, 512, 512
    vol = syn.phantom(n, h, w)
    eng = nat.Engine(0)
    print(f"volume {n} x {h} x {w} int16, batch {args.batch}, medians of {args.reps} (min..max)")
    vd = eng.to_device(vol)
    lab = eng.empty(vol.shape, np.uint8)
    _, xf, bbox, _ = eng.preprocess(vol)
    for name, c in (("R231", 3), ("LTRCLobes", 6)):
        eng.load_state_dict(0, syn.synthetic_state_dict(c, head="lunglike"))
        base = median_ms(lambda: eng.apply_dev(0, vd, lab, batch_size=args.batch), args.reps, eng.sync)
        print(f"[device] {name:9s} lm_apply_dev                {base[0]:8.2f} ms ({base[1]:.2f}..{base[2]:.2f})")
        for dt in (np.float32, np.float16):
            pd = eng.empty((c,) + vol.shape, dt)
            t = median_ms(lambda: eng.apply_probs_dev(0, vd, pd, lab, batch_size=args.batch), args.reps, eng.sync)
            print(f"[device] {name:9s} lm_apply_probs_dev {np.dtype(dt).name:7s}  {t[0]:8.2f} ms ({t[1]:.2f}..{t[2]:.2f})  "
                  f"+{t[0] - base[0]:.2f} ms over labels only")
            pd.free()
        # the un-crop kernel alone on the whole volume's log-probabilities
        _, logp = eng.forward(0, xf)
        ld = eng.to_device(logp)
        bd = eng.to_device(bbox)
        for dt in (np.float32, np.float16):
            pd = eng.empty((c,) + vol.shape, dt)
            eng.uncrop_probs_dev(ld, bd, pd)
            eng.sync()
            eng.profile(True)
            eng.profile_reset()
            for _ in range(args.reps):
                eng.uncrop_probs_dev(ld, bd, pd)
            eng.sync()
            st = [s for s in eng.profile_read() if s["name"] == "uncrop_probs"][0]
            eng.profile(False)
            ms = st["total_ms"] / st["launches"]
            nbytes = st["bytes"] / st["launches"]
            wr = c * n * h * w * np.dtype(dt).itemsize
            print(f"[kernel] {name:9s} uncrop_probs {np.dtype(dt).name:7s} {ms * 1e3:8.1f} us  {nbytes / 1e6:7.1f} MB "
                  f"({wr / 1e6:.1f} written)  {nbytes / ms / 1e9:6.2f} TB/s = {nbytes / ms / 1e9 / (PEAK / 1e12) * 100:5.1f} % of 8 TB/s")
            pd.free()
        ld.free()
        bd.free()
    vd.free()
    lab.free()
    # host to host through LMInferer (page-locked result blocks)
    for name, c in (("R231", 3), ("LTRCLobes", 6)):
        inf = LMInferer(state_dict=syn.synthetic_state_dict(c, head="lunglike"), engine=eng, batch_size=args.batch)
        base = median_ms(lambda: inf.apply(vol), max(3, args.reps // 2), lambda: None)
        print(f"[host]   {name:9s} LMInferer.apply                       {base[0]:8.2f} ms ({base[1]:.2f}..{base[2]:.2f})")
        for dt in (np.float32, np.float16):
            keep = []

            def run():
                keep[:] = [inf.apply_probabilities(vol, dtype=dt)]  # (the previous result goes back to the pool first)

            t = median_ms(run, max(3, args.reps // 2), lambda: None)
            gb = c * vol.size * np.dtype(dt).itemsize / 1e9
            print(f"[host]   {name:9s} LMInferer.apply_probabilities {np.dtype(dt).name:7s} {t[0]:8.2f} ms ({t[1]:.2f}..{t[2]:.2f})  "
                  f"maps {gb:.2f} GB, +{t[0] - base[0]:.1f} ms")
            keep.clear()
        inf.close()
    eng.close()


if __name__ == "__main__":
    main()
