"""Shared parity checks of the network forward against the oracle at shapes a square 256 x 256 input does not reach -- used by
the emulator (CPU) and the GPU test modules so the two suites read the same.

lm_forward_dev takes any batch and any h, w that are multiples of 16.  The split-f16 path picks a conv kernel per U-Net level
(level i is (H >> i, W >> i)) from the level's shape: the 32-wide persistent kernel where W % 32 == 0, the 16-wide persistent
geometry where W == 16 and H is even, the simple 4-wave kernel anywhere else.  SHAPES has one input per thing that
varies below that choice.

Bars (none of them comes from what the engine gives):
* TOL = 1e-3 on the log-probabilities against uo.forward, every value finite, labels equal to the oracle's argmax wherever the
  oracle's top-2 margin exceeds 2 * TOL (BASELINE.json north star);
* the pixels that rule exempts are at most 0.1 % of a case, counted on the ORACLE's margins (with these seeds the share is at most
  0.041 %: 5 of 12288 pixels at (3, 16, 256), C = 3);
* exact-fp32 kernels: |engine - forward_f64| <= 2 N with N = |forward - forward_f64|, the reference's own rounding noise on that
  input (the project holds these kernels to 1.5 N at 256 x 256; the factor 2 allows for a maximum over far fewer pixels);
* split-f16: |split - exact-fp32 of the same engine| <= 5e-4, the accuracy guard's own limit.  Nothing is asserted about split-f16
  in units of N (the project's factor 2.5 was set at 256 x 256 with wide logit ranges and does not transfer).
"""
import numpy as np
import torch

from oracle import unet_oracle as uo

TOL = 1e-3             # BASELINE.json north_star: pre-argmax log-probs within 1e-3
NEAR_TIE_CAP = 1e-3    # share of a case's pixels that the near-tie rule may exempt
F32_NOISE_FACTOR = 2.0  # exact-fp32 kernels vs float64, in units of the reference's own fp32 noise
SPLIT_TO_EXACT = 5e-4  # the accuracy guard's limit (nn_engine.hip: model_probe)

# (B, H, W) and what it reaches that a square 256 input does not
SHAPES = [
    (1, 16, 256),  # 32-wide tiles of 8, 4 and 2 rows; a 1 x 16 level (odd height: the simple kernel, not the 16-wide geometry)
    (3, 16, 256),  # the same with an odd batch
    (2, 48, 256),  # a 3 x 16 level; three row tiles at level 0 (decode's division path); a 16 + 8 row split at (24, 128)
    (3, 48, 64),   # 16-wide at (12, 16) with a pooled output and rows 12..15 outside the image, odd batch; simple kernel at (6, 8), (3, 4)
    (2, 32, 96),   # three column tiles (division path); simple kernel from (16, 48) down
    (1, 256, 16),  # 16-wide at level 0: Cin = 64, pooled output, 16 row tiles, a half-empty slice pair; stand-alone first conv and head
    (1, 512, 32),  # 32 row tiles at level 0; 16-wide with a pooled output at (256, 16)
    (3, 16, 16),   # 16-wide at level 0, then the simple kernel down to a 1 x 1 level; the bilinear x2 from 1 x 1
    (2, 16, 512),  # 16 column tiles; a 1 x 32 level on the 32-wide kernel, every pixel both top and bottom border
    (2, 80, 48),   # the simple kernel with clipped tiles at every level, non-square
]

_REF = {}  # (C, shape) -> reference(): computed once, shared, never written to


def case_input(C, shape):
    B, H, W = shape
    return np.random.default_rng(1000 * C + 7 * B + 3 * H + W).random(shape, dtype=np.float32)


def reference(C, shape, slices=None, f64=True):
    """The oracle's side of a case: input, fp32 and float64 log-probabilities, labels, top-2 margins, N and the near-tie share.
    `slices`: evaluate the oracle on these slices of the input only (every slice is computed on its own)."""
    key = (C, tuple(shape), None if slices is None else tuple(slices), f64)
    if key not in _REF:
        sd = uo.synthetic_state_dict(C)
        x = case_input(C, shape)
        xs = x if slices is None else x[list(slices)]
        xt = torch.from_numpy(np.ascontiguousarray(xs[:, None]))
        with torch.inference_mode():
            ref = uo.forward(sd, xt).numpy()
            ref64 = uo.forward_f64(sd, xt).numpy() if f64 else None
        if C > 1:
            srt = np.sort(ref, axis=1)
            margin = srt[:, -1] - srt[:, -2]
        else:
            margin = np.full(ref[:, 0].shape, np.inf, np.float32)
        r = dict(x=x, ref=ref, ref64=ref64, lab=ref.argmax(1).astype(np.uint8), margin=margin,
                 noise=float(np.abs(ref - ref64).max()) if f64 else None, tie_share=float((margin <= 2 * TOL).mean()))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def check_result(r, lab, logp, precision, exact=None, what=""):
    """The bars of the module docstring on one result; `exact`: the log-probabilities of the same engine's exact-fp32 kernels.
    -> the measured numbers (printed by the callers)."""
    assert np.isfinite(logp).all(), what
    err = float(np.abs(logp - r["ref"]).max())
    bad = lab != r["lab"]
    out = dict(err32=err, noise=r["noise"], tie_share=r["tie_share"], mismatches=int(bad.sum()))
    if r["ref64"] is not None:
        out["err64"] = float(np.abs(logp - r["ref64"]).max())
    if exact is not None:
        out["split_to_exact"] = float(np.abs(logp - exact).max())
    assert r["tie_share"] <= NEAR_TIE_CAP, (what, r["tie_share"])  # on the oracle's margins: the label rule below exempts few pixels
    assert err < TOL, (what, out)
    assert not np.any(bad & (r["margin"] > 2 * TOL)), (what, out, "labels differ away from near-ties")
    if precision == "f32" and r["ref64"] is not None:
        out["ratio"] = out["err64"] / r["noise"] if r["noise"] > 0 else (0.0 if out["err64"] == 0 else float("inf"))  # (one class: N = 0)
        assert out["err64"] <= F32_NOISE_FACTOR * r["noise"], (what, out)
    if precision == "split_f16" and exact is not None:
        assert out["split_to_exact"] <= SPLIT_TO_EXACT, (what, out)
    return out


def exact_log_probabilities(eng, C, shape, x):
    """The exact-fp32 kernels' log-probabilities of this engine on the case (run once per engine and case; the loaded model stays)."""
    cache = eng.__dict__.setdefault("_forward_cases_exact", {})
    key = (C, tuple(shape))
    if key not in cache:
        eng.set_precision("f32")
        try:
            cache[key] = eng.forward(0, x)[1]
        finally:
            eng.set_precision("split_f16")
    return cache[key]


def check_forward(eng, C, shape, precision, fusion=11, dirty=None, load=True):
    """One forward of uo.synthetic_state_dict(C) on the seeded input of `shape` through `eng`, held to the bars of the module
    docstring.  Leaves the engine on `precision` and `fusion` (the callers restore the defaults in a `finally`).  `dirty`: a byte
    for lm_debug_fill_workspaces right before the forward -- the result must not depend on what the workspaces held.  `load=False`
    when the caller knows that slot 0 already holds the model.  -> the measured numbers, with the result under "lab" / "logp"."""
    r = reference(C, shape)
    what = f"C={C} {tuple(shape)} {precision} fusion {fusion} dirty {dirty}"
    if load:
        eng.load_state_dict(0, uo.synthetic_state_dict(C))
        eng.__dict__.pop("_forward_cases_exact", None)
    exact = exact_log_probabilities(eng, C, shape, r["x"]) if precision == "split_f16" else None
    eng.set_precision(precision)
    eng.set_fusion(fusion)
    if dirty is not None:
        eng.debug_fill_workspaces(dirty)
    lab, logp = eng.forward(0, r["x"])
    if precision == "f32":
        eng.__dict__.setdefault("_forward_cases_exact", {}).setdefault((C, tuple(shape)), logp)
    if precision == "split_f16":
        # the range guard has no reason to trip on this model (stale workspace rows once tripped it on the emulator)
        assert eng.model_precision(0) == "split_f16", what
    out = check_result(r, lab, logp, precision, exact, what)
    out.update(lab=lab, logp=logp, what=what)
    return out


def fmt(out):
    s = f"{out['what']}: |engine-ref32| {out['err32']:.2e}"
    if "err64" in out:
        s += f"  |engine-ref64| {out['err64']:.2e}  N {out['noise']:.2e}"
    if "ratio" in out:
        s += f"  ratio {out['ratio']:.2f}"
    if "split_to_exact" in out:
        s += f"  |split-exact| {out['split_to_exact']:.2e}"
    return s + f"  near-tie share {100 * out['tie_share']:.3f} %  label mismatches {out['mismatches']}"
