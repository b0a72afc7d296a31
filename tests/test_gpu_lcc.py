"""The local-correlation metric on the MI355X: lm_local_moments_dev and lm_lcc_step_dev bit for bit against the numpy restatements
of tests/test_lcc_emu.py (its cases, plus (9, 130, 301) for several workgroups, lines longer than one tile of the x pass and of the
line passes, and a repeat on dirty workspaces), the five-iteration loop, the two quality pairs with a field that equals the
emulator's bit for bit, and LMInferer.apply_deformable(metric="lcc") on the synthetic lung-like volume against the emulator."""
import numpy as np
import pytest

from lungmask_amd import deformable as dfm
from lungmask_amd import morphology
from lungmask_amd import registration as reg
from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from tests import test_lcc_emu as cases
from tests.test_deform_emu import make_field, rot_scale, same_bits

pytestmark = pytest.mark.gpu


def test_emulator_cases(gpu_engine):
    for shape, radius in cases.SHAPE_CASES:
        cases.run_shape_case(gpu_engine, shape, radius)
    cases.run_nan_and_labels(gpu_engine)
    cases.run_outside(gpu_engine)
    cases.run_special_windows(gpu_engine)


def test_several_workgroups_and_dirty_workspaces(gpu_engine):
    eng = gpu_engine
    shape = (9, 130, 301)  # rows of 301 > 256: two chunks of the x pass; lines of 130 > 64: three tiles of the y pass
    A, b = rot_scale()
    f, m = cases.pair(shape, 70)
    m = m.copy()
    m[np.random.default_rng(71).random(shape) < 0.01] = np.nan  # voxels the warp would have found outside
    labels = np.random.default_rng(72).integers(0, 4, shape).astype(np.uint8)
    u = make_field("random", shape, 73, cases.SPACING)
    kw = dict(A=A, b=b, moving_shape=shape, spacing=cases.SPACING, inv_k2=0.25, labels=labels, keep=(1, 3))
    first = cases.check_step(eng, f, m, (3, 8, 8), u, **kw)
    assert first[1][1] > 0 and first[1][2] > 0 and first[1][3] > 0
    eng.debug_fill_workspaces(0xA5)  # (the sums between the passes are a workspace the engine keeps)
    again = cases.check_step(eng, f, m, (3, 8, 8), u, **kw)
    assert same_bits(first[0], again[0]) and first[1] == again[1] and same_bits(first[2], again[2])
    cases.check_moments(eng, f, m, (0, 5, 2))  # one line pass: the x pass writes the workspace
    cases.check_moments(eng, f, m, (1, 0, 0))


def test_five_iterations_equal_the_restated_loop(gpu_engine):
    cases.run_five_iterations(gpu_engine)


@pytest.mark.parametrize("s", [1.6, 1.0])
def test_quality_and_bit_equality_with_the_emulator(gpu_engine, emu_engine, s):
    got = cases.check_quality(gpu_engine, s, "gpu")
    want = cases.quality_run(emu_engine, s, "lcc", "emu")
    assert same_bits(got.field.array, want.field.array) and got.levels == want.levels
    assert (got.initial_metric, got.final_metric, got.folding) == (want.initial_metric, want.final_metric, want.folding)
    ssd, ssd_emu = cases.quality_run(gpu_engine, s, "ssd", "gpu"), cases.quality_run(emu_engine, s, "ssd", "emu")
    assert same_bits(ssd.field.array, ssd_emu.field.array)


SP = (2.0, 0.75, 0.75)
REG_KW = dict(levels_mm=(8.0,), max_evaluations=200)
DEF_KW = dict(levels_mm=(8.0, 4.0), iterations=(10, 5), metric="lcc", window_mm=12.0)


def test_apply_deformable_with_the_local_correlation_metric(gpu_engine, emu_engine):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(20, 512, 512)
    grid = rs.Grid.of(vol, SP)
    truth = rs.Affine.from_parameters("rigid", (0.0, 0.0, 2.0, 3.0, -2.0, 0.0), grid.index_to_physical((9.5, 255.5, 255.5)))
    moving = rs.resample_image(grid.like(vol), grid, truth.inverse(), order=1, dtype=np.int16, engine=gpu_engine).array
    moving = (-1000.0 + (moving.astype(np.float64) + 1000.0) * 1.3).astype(np.int16)  # another density: what the metric is for
    labels, r = inf.apply_deformable(vol, moving, spacing=SP, moving_spacing=SP, register_kw=REG_KW, **DEF_KW)
    assert (labels > 0).sum() > 10 ** 4
    rim = morphology.dilate(labels, 10.0, spacing=SP, engine=gpu_engine)
    first = reg.register(vol, moving, "rigid", labels=rim, spacing=SP, moving_spacing=SP, engine=gpu_engine, **REG_KW)
    want = dfm.register_deformable(vol, moving, initial=first, labels=rim, spacing=SP, moving_spacing=SP, engine=emu_engine, **DEF_KW)
    assert r.affine_registration.parameters == first.parameters and r.levels == want.levels and r.folding == want.folding
    assert same_bits(r.field.array, want.field.array) and r.field.array.shape == (3,) + vol.shape
    assert (r.initial_metric, r.final_metric) == (want.initial_metric, want.final_metric)
    meta = r.meta()
    assert meta["metric"] == "lcc" and meta["window_voxels"] == [lv["window_voxels"] for lv in r.levels] and max(meta["window_voxels"][1]) <= 4
    assert 0 < r.levels[-1]["metric"][0][1] < vol.size // 8 and r.folding["folded"] == 0
    print(f"apply_deformable lcc: mean squared residual {r.mean_squared(r.initial_metric):.1f} -> {r.mean_squared(r.final_metric):.1f}, local correlation "
          f"{meta['initial_local_correlation']:.4f} -> {meta['final_local_correlation']:.4f}")
