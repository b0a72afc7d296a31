"""What the airway flood costs (lm_seed_cost_dev, lm_airway_mask_dev) on the 300 x 512 x 512 int16 phantom of lungmask_amd.synthetic
with a synthetic airway tree written into it (`write_tree`: a trachea from the top slice and six generations of forks with radius
8 x 0.75^g voxels, walls of 2 voxels at -100 HU, of 1.5 voxels at -750 HU below a radius of 3, lumen from -990 to -870 HU by
generation, N(0, 20) noise), spacing (1.0, 0.7, 0.7) mm, labelled by the 'lunglike' head as in bench.py.

  (a) seed_cost_dev from find_trachea's seed at cap_hu = -800: the rounds, the time per round, the share of the bricks active per
      round (from the profiler's byte count of the round kernels: 12 800 bytes loaded per active brick), the kernels;
  (b) airway_mask_dev at the rule's threshold;
  (c) in the same run, what the flood replaces: ONE components_dev labelling of HU <= T on the same volume, times the (cap - start) /
      step = 15 thresholds a host-side explosion scan would label;
  (d) the worst case: cap_hu = -700 lets the thin walls (-750 HU) pass, so both lungs flood from the tree;
  (e) segment_airways' device path as a whole (trachea, flood, rule, mask, tree).

One process; medians of `--reps` calls after two warm-up calls; the clocks and the load as the system tool reports them."""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from lungmask_amd import _native as nat  # noqa: E402
from lungmask_amd import airways as aw  # noqa: E402
from lungmask_amd import synthetic as syn  # noqa: E402
from tools.filter_timing import kernels, median_ms  # noqa: E402
from tools.vessel_timing import SPACING, clock_lines  # noqa: E402

RADIUS = [8.0 * 0.75 ** g for g in range(7)]
LENGTH = [118.0, 70.0, 50.0, 36.0, 26.0, 18.0, 12.0]
LUMEN_HU = [-990, -975, -955, -935, -915, -890, -870]
BRICK_LOAD_BYTES = (2048 + 1152) * 4  # xenc and cost, int16 each, of the brick and its six face halos


def load_lines():
    """The GPU's load as the system tool reports it (read only); empty when the tool is missing."""
    try:
        r = subprocess.run(["rocm-smi", "--showuse", "-d", "0"], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in r.stdout.splitlines() if "use" in ln.lower() and "%" in ln]
    except (OSError, subprocess.SubprocessError):
        return []


def branches():
    out = []

    def grow(g, start, direction):
        end = start + direction * LENGTH[g]
        out.append((g, start, end))
        if g == len(RADIUS) - 1:
            return
        axis = 2 if g % 2 == 0 else 1
        for sign in (-1.0, 1.0):
            a = np.deg2rad(40.0) * sign
            d = direction.copy()
            d[0] = direction[0] * np.cos(a) - direction[axis] * np.sin(a)
            d[axis] = direction[0] * np.sin(a) + direction[axis] * np.cos(a)
            grow(g + 1, end, d / np.linalg.norm(d))

    grow(0, np.array([-4.0, 256.0, 256.0]), np.array([1.0, 0.0, 0.0]))
    return out


def write_tree(vol, seed=7):
    """Writes the tube tree into `vol` (walls first, then the lumina, each branch inside its own box) -> the number of lumen voxels."""
    rng = np.random.default_rng(seed)
    lumen = np.zeros(vol.shape, bool)
    for wall in (True, False):
        for g, a, b in branches():
            r = RADIUS[g] + ((2.0 if RADIUS[g] >= 3.0 else 1.5) if wall else 0.0)
            lo = np.maximum(np.floor(np.minimum(a, b) - r - 1).astype(int), 0)
            hi = np.minimum(np.ceil(np.maximum(a, b) + r + 2).astype(int), vol.shape)
            if (hi <= lo).any():
                continue
            grid = np.stack(np.meshgrid(*(np.arange(l, h, dtype=np.float64) for l, h in zip(lo, hi)), indexing="ij"), axis=-1)
            ab = b - a
            t = np.clip(((grid - a) @ ab) / (ab @ ab), 0.0, 1.0)
            inside = np.linalg.norm(grid - (a + t[..., None] * ab), axis=-1) <= r
            box = tuple(slice(l, h) for l, h in zip(lo, hi))
            if wall:
                inside &= ~lumen[box]
                vol[box][inside] = np.rint((-100.0 if RADIUS[g] >= 3.0 else -750.0) + rng.normal(0, 20, int(inside.sum()))).astype(vol.dtype)
            else:
                inside &= ~lumen[box]  # (a voxel of two lumina keeps the earlier generation's value)
                vol[box][inside] = np.rint(LUMEN_HU[g] + rng.normal(0, 20, int(inside.sum()))).astype(vol.dtype)
                lumen[box] |= inside
    return int(lumen.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "airway_timing.log"))
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
    lumen = write_tree(vol)
    lab = eng.apply(0, vol)
    bricks, brick = eng.seed_cost_bricks(vol.shape)
    out(f"volume {n} x {h} x {w} {vol.dtype}, spacing {SPACING} mm, {(lab > 0).mean() * 100:.1f} % labelled; tree lumen {lumen} voxels; "
        f"{bricks} bricks of {brick}; medians of {args.reps} (min..max) after 2 warm-up calls")
    for ln in clock_lines():
        out("clock: " + ln)
    for ln in load_lines():
        out("load: " + ln)
    vd, ld = eng.to_device(vol), eng.to_device(lab)
    trachea = aw.trachea_dev(eng, vd, ld, spacing=SPACING)
    seed = [tuple(trachea["index"])]
    out(f"trachea: seed {seed[0]}, component {trachea['component']} of {trachea['components']}, {len(trachea['candidates'])} candidate(s), "
        f"rejected {trachea['rejected']}")
    cost = eng.empty(vol.shape, np.int16)
    mask = eng.empty(vol.shape, np.uint8)

    def report(what, fn):
        call = median_ms(fn, args.reps)
        ks = kernels(eng, fn, args.reps)
        total = sum(x[0] for x in ks.values())
        out(f"{what:44s} whole call {call[0]:9.3f} ms ({call[1]:.3f}..{call[2]:.3f})   kernels {total:9.3f} ms")
        for k, (ms, b) in ks.items():
            out(f"{'':44s}   {k:18s} {ms:9.3f} ms" + (f"  {b / ms / 1e6:8.1f} GB/s" if ms > 0 and b > 0 else ""))
        return call[0], ks

    def flood_report(tag, cap):
        _, curve, info = eng.seed_cost_dev(vd, seed, cap, out=cost)
        out(f"{tag} cap_hu {cap}: {info['rounds']} rounds, {info['reached']} voxels reached = {info['reached'] / vol.size * 100:.2f} % of the volume")
        call, ks = report(f"{tag} seed_cost_dev, cap_hu {cap}", lambda: eng.seed_cost_dev(vd, seed, cap, out=cost))
        ms, b = ks.get("seed_round", (0.0, 0.0))
        rounds = max(1, info["rounds"])
        active = b / BRICK_LOAD_BYTES / rounds
        out(f"{tag} per round: {ms / rounds * 1e3:.1f} us of kernel, {call / rounds * 1e3:.1f} us of the whole call (launch, 4-byte read-back, "
            f"wait); {active:.1f} bricks active per round on average = {active / bricks * 100:.3f} % of {bricks}; the round kernels load "
            f"{b / 1e6:.2f} MB in all = {b / max(1, info['reached']):.1f} bytes per reached voxel (a brick streams 6.25 bytes per voxel it "
            f"owns per round it runs, and writes at most 2)")
        return curve, info, call

    curve, info, flood_ms = flood_report("(a)", -800)
    chosen = aw.choose_threshold(curve, float(np.prod(SPACING)) / 1000.0)
    out(f"(a) the rule: threshold {chosen['threshold']}, first leaking {chosen['first_leaking']}, {chosen['voxels']} voxels = "
        f"{chosen['volume_ml']:.1f} ml; curve {chosen['curve']}")
    t = chosen["threshold"] if chosen["threshold"] is not None else -900
    report("(b) airway_mask_dev with labels", lambda: eng.airway_mask_dev(cost, t, lab=ld, out=mask))

    zeros = eng.to_device(np.zeros(vol.shape, np.uint8))
    ids = eng.empty(vol.shape, np.int32)

    def labelling():
        eng.components_dev(zeros, vd, hu_range=(None, t), keep=[0], per_label=False, connectivity=6, out=ids)

    one, _ = report(f"(c) components_dev of HU <= {t}, once", labelling)
    steps = (-800 - aw.RULE_DEFAULTS["start_hu"]) // aw.RULE_DEFAULTS["step_hu"]
    out(f"(c) a host-side explosion scan labels {steps} thresholds: {steps} x {one:.3f} = {steps * one:.3f} ms against the flood's "
        f"{flood_ms:.3f} ms: the flood is {steps * one / flood_ms:.2f} x as fast" if flood_ms > 0 else "(c) no flood time")
    zeros.free()
    ids.free()

    flood_report("(d)", -700)

    def whole():
        aw.airways_dev(eng, vd, ld, spacing=SPACING)

    res = aw.airways_dev(eng, vd, ld, spacing=SPACING)
    out(f"(e) segment_airways: threshold {res.threshold}, {res.analysis['voxels']} voxels, {res.analysis['volume_ml']:.1f} ml, by label "
        f"{ {k: v['voxels'] for k, v in res.analysis['by_label'].items()} }, tree {res.tree['totals']}, segments per generation "
        f"{[g['segments'] for g in res.tree['generations']]}")
    call = median_ms(whole, max(2, args.reps // 3))
    out(f"(e) segment_airways device path, whole       {call[0]:9.3f} ms ({call[1]:.3f}..{call[2]:.3f})")
    for d in (vd, ld, cost, mask):
        d.free()
    eng.close()
    log.close()


if __name__ == "__main__":
    main()
