"""Fields as operands on the MI355X: lm_field_combine_dev bit for bit against the numpy restatement of tests/test_field_emu.py (its
cases, plus (9, 130, 301) for several workgroups, twice with the workspaces overwritten in between), `invert` against the loop
written with the oracle, the round trip and `compose`, and LMInferer.apply_deformable(inverse=True) on the synthetic lung-like
volume: the labels carried onto the moving grid through the inverse, against carrying them with the affine's inverse alone."""
import numpy as np
import pytest

from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from tests import test_field_emu as cases
from tests.test_deform_emu import SHAPES, SPACING, rot_scale, same_bits
from tests.test_field_emu import FIELDS, ROT, check_combine, rand_field

pytestmark = pytest.mark.gpu


def test_combine_cases(gpu_engine):
    for shapes in SHAPES:
        for kind in FIELDS:
            cases.run_combine_cases(gpu_engine, shapes, kind)
        cases.run_pointer_patterns(gpu_engine, shapes)
    cases.run_nan_inputs(gpu_engine)
    cases.run_cap(gpu_engine)
    cases.run_dirty_outputs(gpu_engine)


def test_exact_properties(gpu_engine):
    cases.run_properties(gpu_engine)


def test_several_workgroups_and_dirty_workspaces(gpu_engine):
    eng = gpu_engine
    shape = (9, 130, 301)
    A, b = rot_scale()
    src, add, ref = rand_field(shape, 40, SPACING), rand_field(shape, 41, SPACING), rand_field(shape, 42, SPACING)
    coord = cases.make_field("special", shape, 43, SPACING)
    kw = dict(R=ROT, add=add, coord=coord, ref=ref, alpha=0.75, beta=-1.25, spacing=SPACING)
    first = check_combine(eng, src, shape, A, b, **kw)
    eng.debug_fill_workspaces(0xA5)  # (the call keeps no workspace: nothing changes)
    again = check_combine(eng, src, shape, A, b, **kw)
    assert same_bits(first[0], again[0]) and first[1] == again[1] and first[1][0] > 0 and first[1][2] > 2 ** 32
    check_combine(eng, src, shape, np.eye(3), np.zeros(3), coord=add, ref=add, beta=-1.0, spacing=SPACING)


def test_invert_equals_the_oracle_loop(gpu_engine):
    cases.run_invert_constant(gpu_engine)
    cases.run_invert_smooth(gpu_engine)
    cases.run_invert_folded(gpu_engine)


def test_round_trip_and_compose(gpu_engine):
    cases.run_round_trip(gpu_engine)
    cases.run_compose(gpu_engine)


SP = (2.0, 0.75, 0.75)
REG_KW = dict(levels_mm=(8.0,), max_evaluations=200)
DEF_KW = dict(levels_mm=(8.0, 4.0), iterations=(10, 5))


def known_field(grid):
    """A smooth in-plane field, millimetres: one bump of 6 mm along x over the first lung, one of -5 mm along y over the other
    (sigma 40 mm)."""
    sp = dfm.spacing_zyx(grid)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) * s for n, s in zip(grid.shape, sp)], indexing="ij")
    h, w = (grid.shape[1] - 1) * sp[1], (grid.shape[2] - 1) * sp[2]
    bump = lambda cy, cx: np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * 40.0 ** 2))  # noqa: E731
    return np.stack([np.zeros(grid.shape), -5.0 * bump(0.5 * h, 0.7 * w), 6.0 * bump(0.5 * h, 0.3 * w)]).astype(np.float32)


def mean_dice(a, b):
    labels = [k for k in np.unique(b) if k > 0]
    return float(np.mean([2.0 * ((a == k) & (b == k)).sum() / max(1, (a == k).sum() + (b == k).sum()) for k in labels]))


def test_apply_deformable_inverse(gpu_engine):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(20, 512, 512)
    grid = rs.Grid.of(vol, SP)
    known = dfm.DisplacementField(known_field(grid), grid)
    moving = dfm.warp_image(vol, known, 1, dtype=np.int16, engine=gpu_engine, spacing=SP)
    moving = moving.array if hasattr(moving, "array") else moving
    labels, r = inf.apply_deformable(vol, moving, spacing=SP, moving_spacing=SP, register_kw=REG_KW, inverse=True, **DEF_KW)
    assert (labels > 0).sum() > 10 ** 4 and np.array_equal(labels, inf.apply(vol))
    assert r.inverse_field.grid.shape == moving.shape and r.labels_on_moving.shape == moving.shape and r.labels_on_moving.dtype == np.uint8
    want = dfm.warp_labels(labels, r.inverse_field, "linear", engine=gpu_engine, spacing=SP)
    want = want.array if hasattr(want, "array") else want
    assert same_bits(r.labels_on_moving, want)
    inv, info = dfm.invert(r.field, onto=rs.Grid.of(moving, SP), engine=gpu_engine)
    assert same_bits(inv.array, r.inverse_field.array) and info == r.inverse_info == r.meta()["inverse"]
    assert set(info) == {"iterations", "converged", "residual_max_mm", "residual_rms_mm", "residuals", "outside", "nonfinite"}
    assert info["converged"] and info["nonfinite"] == 0 and r.folding["folded"] == 0
    # the true labels of the moving image, and what the affine's inverse alone carries there
    truth = dfm.warp_labels(labels, known, "linear", engine=gpu_engine, spacing=SP)
    truth = truth.array if hasattr(truth, "array") else truth
    alone = dfm.warp_labels(labels, dfm.DisplacementField.zeros(r.inverse_field.grid, r.inverse_field.affine), "linear", engine=gpu_engine,
                            spacing=SP)
    alone = alone.array if hasattr(alone, "array") else alone
    d_field, d_affine = mean_dice(r.labels_on_moving, truth), mean_dice(alone, truth)
    ic = dfm.inverse_consistency(r.field, r.inverse_field, engine=gpu_engine)
    print(f"apply_deformable(inverse=True): Dice on the moving grid {d_field:.4f} through the inverse field, {d_affine:.4f} through the affine's "
          f"inverse alone; {info['iterations']} iterations to {info['residual_max_mm']:.4f} mm; inverse consistency {ic['max_mm']:.3f} mm at most, "
          f"{ic['rms_mm']:.4f} mm RMS, {ic['outside']} voxels outside")
    assert d_field > d_affine
