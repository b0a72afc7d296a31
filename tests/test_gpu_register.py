"""Registration on the MI355X: lm_joint_hist_dev bit for bit against the numpy restatement of tests/test_register_emu.py (its cases,
plus (9, 130, 301) once per mode for several workgroups), a whole registration -- sub-voxel, and with exactly the parameters and
evaluations the emulation library gives --, LMInferer.apply_registered (R231, LTRCLobes, the fused mode, a non-LPS Volume, after
lm_debug_fill_workspaces) and the CLI round trip."""
import json

import numpy as np
import pytest
import torch

from lungmask_amd import morphology
from lungmask_amd import registration as reg
from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_register_emu import (AFFINE_CASE, DTYPES, MAPS, Q, REG_SPACING, RIGID_CASES, SHAPES, TRE_BOUND_MM, check, joint_hist_oracle,
                                     lung_classes, registration_case, run, target_registration_error, volume)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_maps_shapes_steps_and_bins(gpu_engine, mode):
    for shapes in SHAPES:
        fixed, moving = volume(shapes[0], np.int16, 1), volume(shapes[1], np.int16, 2)
        for name, (A, b) in sorted(MAPS.items()):
            hist, counts = check(gpu_engine, fixed, moving, A, b, mode=mode)
            if name == "outside":
                assert counts[1] == 0 and not hist.any()
    fixed, moving = volume((5, 37, 130), np.int16, 3), volume((4, 30, 131), np.int16, 4)
    A, b = MAPS["rotation"]
    for start, step in (((0, 0, 0), (1, 1, 1)), ((1, 2, 3), (2, 3, 4)), ((0, 1, 0), (9, 50, 200)), ((5, 0, 0), (1, 1, 1))):
        check(gpu_engine, fixed, moving, A, b, start=start, step=step, mode=mode)
    for bins in (2, 32, 64):
        width = -(-2048 // bins)
        check(gpu_engine, volume((5, 7, 9), np.int16, 5), volume((4, 6, 11), np.int16, 6), A, b, bins, (-1024, width), (-1000, width + 1), mode=mode)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_every_dtype_pair(gpu_engine, mode):
    A, b = MAPS["rotation"]
    for fdtype in DTYPES:
        for mdtype in DTYPES:
            fixed, moving = volume((5, 7, 9), fdtype, 7), volume((4, 6, 11), mdtype, 8)
            check(gpu_engine, fixed, moving, A, b, 32, (0, 1) if fdtype == np.uint8 else (-1024, 64), (0, 1) if mdtype == np.uint8 else (-1024, 64),
                  mode=mode)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_several_workgroups(gpu_engine, mode):
    shape = (9, 130, 301)
    fixed, moving = volume(shape, np.float32, 30), volume(shape, np.int16, 31)
    labels = np.random.default_rng(32).integers(0, 4, shape).astype(np.uint8)
    for name in ("rotation", "shift", "permute_flip"):
        check(gpu_engine, fixed, moving, *MAPS[name], mode=mode)
    check(gpu_engine, fixed, moving, *MAPS["rotation"], labels=labels, keep=(1, 3), start=(1, 0, 2), step=(1, 2, 1), mode=mode)


def test_properties(gpu_engine):
    eng = gpu_engine
    vol = np.full((41, 41, 41), -700, np.int16)  # 68 921 samples of weight 65 536 in one bin: more than 2^32
    for mode in ("linear", "nearest"):
        hist, counts = check(eng, vol, vol, *MAPS["identity"], 32, (-1024, 64), (-1024, 1), mode=mode)
        assert counts[1] == 68921 and hist[5, 31] == 68921 * Q and np.count_nonzero(hist) == 1
    fixed = volume((5, 37, 130), np.int16, 14)
    moving = np.random.default_rng(15).integers(-20, 40, (6, 30, 128)).astype(np.int16)
    A, b = MAPS["shift"]
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
               for x, y in zip(run(eng, fixed, moving, A, b, 64, (-1024, 32), (-20, 1), mode="linear"),
                               run(eng, fixed, moving, A, b, 64, (-1024, 32), (-20, 1), mode="nearest")))
    fixed, moving = volume((3, 37, 130), np.int16, 16), volume((3, 37, 130), np.float32, 17)
    A, b = MAPS["rotation"]
    want, wc = joint_hist_oracle(fixed, moving, A, b, 32, (-1024, 64), (-1024, 64))
    with eng.scope() as dev:
        fd, md = dev.upload(fixed), dev.upload(moving)
        out = dev.empty((32 * 32 + 4,), np.int64)
        results = []
        for _ in range(2):
            eng.joint_hist_dev(fd, md, A, b, out=out)
            eng.sync()
            results.append(out.download())
            assert eng.debug_fill_workspaces(0xA5) > 0
    for got in results:
        assert np.array_equal(got[:1024].reshape(32, 32), want) and list(got[1024:]) == wc


@pytest.mark.parametrize("case", sorted(RIGID_CASES))
def test_rigid_registration_is_sub_voxel_and_equals_the_emulator(gpu_engine, emu_engine, case):
    fixed, moving, truth = registration_case("rigid", RIGID_CASES[case])
    r = reg.register(fixed, moving, "rigid", moving_spacing=REG_SPACING, engine=gpu_engine)  # levels 8, 4 and 2 mm
    mean, worst, before = target_registration_error(r.transform, truth, fixed)
    print(f"rigid {case}: TRE mean {mean:.4f} mm, max {worst:.4f} mm (before: {before:.2f} mm), {r.evaluations} evaluations, "
          f"levels {[lv['evaluations'] for lv in r.levels]}")
    assert mean < TRE_BOUND_MM
    assert [lv["step"] for lv in r.levels] == [[4, 5, 5], [2, 3, 3], [1, 1, 1]]
    e = reg.register(fixed, moving, "rigid", moving_spacing=REG_SPACING, engine=emu_engine)
    assert r.parameters == e.parameters and r.evaluations == e.evaluations and r.counts == e.counts and r.levels == e.levels


def test_affine_and_label_driven_registration(gpu_engine, emu_engine):
    fixed, moving, truth = registration_case("affine", AFFINE_CASE)
    kw = dict(levels_mm=(4.0,), moving_spacing=REG_SPACING)
    r = reg.register(fixed, moving, "affine", engine=gpu_engine, **kw)
    mean, worst, _ = target_registration_error(r.transform, truth, fixed)
    print(f"affine: TRE mean {mean:.4f} mm, max {worst:.4f} mm, {r.evaluations} evaluations")
    assert mean < TRE_BOUND_MM
    e = reg.register(fixed, moving, "affine", engine=emu_engine, **kw)
    assert r.parameters == e.parameters and r.evaluations == e.evaluations
    fixed, moving, truth = registration_case("rigid", RIGID_CASES["a"])
    kw = dict(mode="nearest", bins=4, hu_range=(0, 3), levels_mm=(2.0,), moving_spacing=REG_SPACING)
    r = reg.register(fixed.like(lung_classes(fixed.array)), lung_classes(moving), "rigid", engine=gpu_engine, **kw)
    mean, worst, _ = target_registration_error(r.transform, truth, fixed)
    print(f"labels: TRE mean {mean:.4f} mm, max {worst:.4f} mm, {r.evaluations} evaluations")
    assert mean < TRE_BOUND_MM
    e = reg.register(fixed.like(lung_classes(fixed.array)), lung_classes(moving), "rigid", engine=emu_engine, **kw)
    assert r.parameters == e.parameters and r.evaluations == e.evaluations


# ------------------------------------------------------------------------------------------------ LMInferer.apply_registered
SP = (2.0, 0.75, 0.75)
REG_KW = dict(levels_mm=(8.0, 4.0), max_evaluations=1000)
COARSE_BOUND_MM = 0.5 * max(SP)  # the levels stop at a sampling distance of 4 mm: half of the slice spacing


def moved(vol, grid, transform, eng):
    """`vol` under `transform` on its own grid (linear, int16): a second acquisition of the same anatomy."""
    return rs.resample_image(grid.like(vol), grid, transform, order=1, dtype=np.int16, engine=eng).array


def same_registration(a, b):
    return (a.parameters == b.parameters and a.evaluations == b.evaluations and a.counts == b.counts and a.centre == b.centre and
            np.array_equal(a.transform.matrix, b.transform.matrix) and np.array_equal(a.transform.translation_vector, b.transform.translation_vector))


@pytest.mark.parametrize("model", ["R231", "LTRCLobes", "LTRCLobes_R231"])
def test_apply_registered_models(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    fused = model == "LTRCLobes_R231"
    c = 3 if model == "R231" else 6
    kw = dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(c, head="lunglike"),
              fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)
    inf = LMInferer(engine=gpu_engine, **kw)
    vol = syn.phantom(20, 512, 512)
    grid = rs.Grid.of(vol, SP)
    truth = rs.Affine.from_parameters("rigid", (0.0, 0.0, 2.0, 3.0, -2.0, 0.0), grid.index_to_physical((9.5, 255.5, 255.5)))
    moving = moved(vol, grid, truth.inverse(), gpu_engine)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 4
    labels, r = inf.apply_registered(vol, moving, spacing=SP, moving_spacing=SP, **REG_KW)
    assert np.array_equal(labels, expect)
    rim = morphology.dilate(expect, 10.0, spacing=SP, engine=gpu_engine)
    want = reg.register(vol, moving, "rigid", labels=rim, spacing=SP, moving_spacing=SP, engine=gpu_engine, **REG_KW)
    assert same_registration(r, want)
    assert np.array_equal(r.image, want.resample(moving, moving_spacing=SP, engine=gpu_engine).array)
    assert 0 < r.counts["sampled"] == int((rim[::2, ::5, ::5] > 0).sum())  # the last level: 4 mm
    pts = np.array([grid.index_to_physical(i) for i in np.argwhere(expect > 0)[::997]])
    tre = float(np.linalg.norm(r.transform.apply(pts) - truth.apply(pts), axis=1).mean())
    print(f"{model}: TRE mean {tre:.4f} mm, {r.evaluations} evaluations, parameters {np.round(r.parameters, 3)}")
    assert tre < COARSE_BOUND_MM
    gpu_engine.debug_fill_workspaces(0xA5)  # the partial histograms are workspace: a dirty one changes nothing
    labels2, r2 = inf.apply_registered(vol, moving, spacing=SP, moving_spacing=SP, **REG_KW)
    assert np.array_equal(labels2, labels) and same_registration(r2, r) and np.array_equal(r2.image, r.image)


def test_apply_registered_non_lps_volume(gpu_engine):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)  # permuted and flipped
    axes, flips = volume_io.lps_transform(direction)
    arr = np.ascontiguousarray(volume_io.apply_transform(syn.phantom(20, 512, 512), *volume_io.inverse_transform(axes, flips)))
    img = volume_io.Volume(arr, (0.75, 0.75, 2.0), (-12.0, 30.0, 4.5), direction)
    grid = rs.Grid.of(img)
    truth = rs.Affine.translation((2.0, -3.0, 1.0))
    moving = grid.like(moved(arr, grid, truth.inverse(), gpu_engine))
    expect = inf.apply(img).copy()
    labels, r = inf.apply_registered(img, moving, "translation", **REG_KW)
    assert np.array_equal(labels, expect) and (expect > 0).any()
    want = reg.register(img, moving, "translation", labels=morphology.dilate(img.like(expect), 10.0, engine=gpu_engine), engine=gpu_engine, **REG_KW)
    assert same_registration(r, want) and np.array_equal(r.image, want.resample(moving, engine=gpu_engine).array)
    assert np.abs(r.transform.translation_vector - truth.translation_vector).max() < COARSE_BOUND_MM


def test_cli_registration_round_trip(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.75, 0.75, 2.0), (1.0, 2.0, 3.0))
    grid = rs.Grid.of(img)
    moving = grid.like(moved(img.array, grid, rs.Affine.translation((-2.0, 3.0, 0.0)), gpu_engine))
    ip, mp = tmp_path / "in.nii.gz", tmp_path / "moving.nii.gz"
    volume_io.write_nifti(str(ip), img)
    volume_io.write_nifti(str(mp), moving)
    loaded, loaded_moving = volume_io.load_input_image(str(ip)), volume_io.load_input_image(str(mp))
    ref_labels, ref = LMInferer(modelpath=str(wp), engine=gpu_engine).apply_registered(loaded, loaded_moving, transform="translation")
    rp, jp = tmp_path / "r.nii.gz", tmp_path / "t.json"
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--register-moving", str(mp), "--registered", str(rp),
                 "--registration", str(jp), "--register-transform", "translation"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    assert json.load(open(jp)) == json.loads(json.dumps(ref.meta()))
    back = volume_io.load_input_image(str(rp))
    assert back.array.dtype == np.float32 and np.array_equal(np.ascontiguousarray(back.array), ref.image)
    np.testing.assert_allclose(back.spacing, loaded.spacing, atol=1e-6)
    # beside --stats: from the labels it returned
    assert main([str(ip), str(tmp_path / "out2.npy"), "--modelpath", str(wp), "--noprogress", "--register-moving", str(mp), "--registration",
                 str(tmp_path / "t2.json"), "--register-transform", "translation", "--stats", str(tmp_path / "s.json")]) == 0
    assert json.load(open(tmp_path / "t2.json"))["parameters"] == ref.parameters
