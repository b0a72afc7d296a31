"""GPU parity of the network forward (lm_forward_dev) at every kind of shape it accepts, against the oracle.

tests/test_gpu_forward.py holds the forward to the oracle at square 32, 48, 64 and 256 inputs.  A square input has full 16-row
tiles and power-of-two tile counts, meets the 16-wide geometry only at a 16 x 16 level with 512 or 1024 input channels, and never
splits a launch into sub-batches.  The cases of tests/forward_cases.py (shapes, bars and their reasons are listed there) reach the
rest: row tiles of 8, 4, 2 and 1 rows, three row or column tiles, 16-wide levels of odd height (routed to the simple kernel, the
16-wide epilogue stores rows in pairs), of height 12 with a pooled output, at level 0; odd batches on slice pairs; the 1 x 1 level;
launches cut below 2 GiB.

Measured on an MI355X over test_forward_shapes and test_class_counts: |exact-fp32 kernels - float64| / N is 0.80 .. 1.25 (the
largest at (1, 512, 32), C = 3; bar 2), N 1.8e-5 .. 5.2e-5; split-f16 at most 1.24e-4 from the fp32 oracle and 1.18e-4 from the
exact-fp32 kernels (bar 5e-4); near-tie share at most 0.041 %.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import forward_cases as fc
from oracle import unet_oracle as uo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restore(eng):
    eng.set_fusion(11)
    eng.set_precision("split_f16")


def _clean_and_dirty(eng, C, shape, precision, fusion=11):
    """The case on the workspace as it stands and after lm_debug_fill_workspaces(0xA5): both within the bars, and the same bytes."""
    a = fc.check_forward(eng, C, shape, precision, fusion, load=False)
    b = fc.check_forward(eng, C, shape, precision, fusion, dirty=0xA5, load=False)
    print(fc.fmt(a))
    assert np.array_equal(a["lab"], b["lab"]) and np.array_equal(a["logp"], b["logp"]), (a["what"], "depends on what the workspace held")
    return a


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_shapes(gpu_engine, shape, C):
    """Every shape of forward_cases.SHAPES: the exact-fp32 kernels, and the split-f16 ones with fusion masks 11 (the default), 0
    (stand-alone first conv and head, single-chain 1x1) and 15 (all fusions, split-K 1x1)."""
    try:
        gpu_engine.load_state_dict(0, uo.synthetic_state_dict(C))
        gpu_engine.__dict__.pop("_forward_cases_exact", None)
        _clean_and_dirty(gpu_engine, C, shape, "f32")
        for mask in (11, 0, 15):
            _clean_and_dirty(gpu_engine, C, shape, "split_f16", mask)
    finally:
        _restore(gpu_engine)


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
@pytest.mark.parametrize("C", [1, 2, 8])
def test_class_counts(gpu_engine, C, precision):
    """1, 2 and kMaxClasses = 8 classes at (3, 48, 64).  One class: the log-softmax of a single logit is exactly 0, the label 0."""
    try:
        out = fc.check_forward(gpu_engine, C, (3, 48, 64), precision)
        print(fc.fmt(out))
        assert out["logp"].shape == (3, C, 48, 64)
        if C == 1:
            assert not out["logp"].any() and not out["lab"].any()
    finally:
        _restore(gpu_engine)
        gpu_engine.load_state_dict(0, uo.synthetic_state_dict(3))


def test_nine_classes_are_refused(gpu_engine):
    from lungmask_amd import _native as nat

    try:
        with pytest.raises(nat.LMError):
            gpu_engine.load_state_dict(0, uo.synthetic_state_dict(9))
    finally:
        gpu_engine.load_state_dict(0, uo.synthetic_state_dict(3))


@pytest.mark.parametrize("shape", [(3, 16, 32), (3, 48, 64)], ids=lambda s: "x".join(map(str, s)))
def test_batch_composition(gpu_engine, shape):
    """nn_engine.hip: "every slice is computed on its own" -- slice b forwarded alone gives the label and log-probability bytes of
    slice b of the batch (odd batch: the last slice pair of the 16-wide geometry is half empty, alone every pair is)."""
    gpu_engine.load_state_dict(0, uo.synthetic_state_dict(3))
    x = fc.case_input(3, shape)
    lab, logp = gpu_engine.forward(0, x)
    for b in range(shape[0]):
        lab1, logp1 = gpu_engine.forward(0, x[b : b + 1])
        assert np.array_equal(lab1[0], lab[b]) and np.array_equal(logp1[0], logp[b]), (shape, b)


def test_sub_batches():
    """(128, 256, 256): launch_conv_h3_t cuts every launch whose input tensor reaches 2 GiB -- the cstride-128 launches of level 0
    into 62 + 62 + 4 slices, the cstride-64 ones (among them the one with the fused first layer and the one with the fused head)
    and the level-1 concat into 126 + 2.  Slices on both sides of every cut against the oracle; all 128 slices byte for byte
    against the same engine run in batches of 20 (one launch each); the same for the labels of the exact-fp32 kernels, which have
    no sub-batches but tensors beyond 4 GiB.  An engine of its own: ~14 GB of workspace that must not stay with the session's."""
    from lungmask_amd import _native as nat

    C, shape, idx = 3, (128, 256, 256), (0, 61, 62, 123, 124, 125, 126, 127)
    r = fc.reference(C, shape, slices=idx, f64=False)
    x = r["x"]
    eng = nat.Engine(0)
    try:
        eng.load_state_dict(0, uo.synthetic_state_dict(C))
        lab, logp = eng.forward(0, x)
        assert eng.model_precision(0) == "split_f16"
        out = fc.check_result(r, lab[list(idx)], logp[list(idx)], "split_f16", what=f"{shape} slices {idx}")
        print(f"{shape} split-f16, slices {idx}: |engine-ref32| {out['err32']:.2e}  near-tie share {100 * out['tie_share']:.3f} %  "
              f"label mismatches {out['mismatches']}")
        for b0 in range(0, shape[0], 20):
            lab20, logp20 = eng.forward(0, x[b0 : b0 + 20])
            assert np.array_equal(lab20, lab[b0 : b0 + 20]) and np.array_equal(logp20, logp[b0 : b0 + 20]), f"slices from {b0}"
        del logp, logp20
        eng.set_precision("f32")
        lab_f = eng.forward(0, x, want_logp=False)[0]
        bad = lab_f[list(idx)] != r["lab"]
        assert not np.any(bad & (r["margin"] > 2 * fc.TOL))
        for b0 in range(0, shape[0], 20):
            assert np.array_equal(eng.forward(0, x[b0 : b0 + 20], want_logp=False)[0], lab_f[b0 : b0 + 20]), f"fp32, slices from {b0}"
    finally:
        eng.close()


_SCHEDULE_SHAPES = ((3, 48, 256), (2, 32, 96))


@pytest.mark.parametrize("env", [{"LM_H3_ORDER": "0"}, {"LM_H3_ORDER": "1"}, {"LM_H3_KSPLIT_K": "1152", "LM_ACC_GUARD": "0"}],
                         ids=["order0", "order1", "ksplit1152"])
def test_forced_schedules_at_small_shapes(env):
    """LM_H3_ORDER forces one work-item order on every layer, LM_H3_KSPLIT_K the split-K 3x3 form: at 256 x 256 the padded index
    space of the pixel-tile-major order and the split-K parts only ever see power-of-two tile counts.  Here: 3 row tiles x 8 column
    tiles x 3 slices, the 3 x 16 level on the simple kernel beside it, 3 column tiles.  The variables are read once per process: a
    fresh child per setting runs the forwards (split-f16 and exact fp32), this process holds them to the oracle."""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from lungmask_amd import _native as nat\n"
        "from oracle import unet_oracle as uo\n"
        "import forward_cases as fc\n"
        "e = nat.Engine(0); e.load_state_dict(0, uo.synthetic_state_dict(3)); out = {}\n"
        "for i, shape in enumerate(%r):\n"
        "    x = fc.case_input(3, shape)\n"
        "    out['lab%%d' %% i], out['logp%%d' %% i] = e.forward(0, x)\n"
        "    assert e.model_precision(0) == 'split_f16'\n"
        "    out['exact%%d' %% i] = fc.exact_log_probabilities(e, 3, shape, x)\n"
        "e.close(); np.savez(sys.argv[1], **out)\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), _SCHEDULE_SHAPES)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "out.npz")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = dict(np.load(f))
    for i, shape in enumerate(_SCHEDULE_SHAPES):
        what = f"{env} C=3 {shape} split_f16"
        out = fc.check_result(fc.reference(3, shape), got[f"lab{i}"], got[f"logp{i}"], "split_f16", got[f"exact{i}"], what)
        out["what"] = what
        print(fc.fmt(out))
