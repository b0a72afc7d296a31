"""Resampling on the MI355X: lm_resample_dev / lm_spline_prefilter_dev bit for bit against the numpy restatement of
tests/test_resample_emu.py (its shapes, plus (9, 130, 301) once per mode), LMInferer.apply_resampled (R231, LTRCLobes, the fused mode, a
non-LPS Volume, several engines), the result after lm_debug_fill_workspaces, and the CLI's --resampled round trip."""
import numpy as np
import pytest
import torch

from lungmask_amd import resample as rs
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_resample_emu import SHAPES, check, check_shape, labels_for, maps_for, prefilter
from tests.test_roi_emu import same_bits, volume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES)
def test_every_mode_dtype_and_map(gpu_engine, shape):
    check_shape(gpu_engine, shape)
    vol = volume(shape, np.float32, 6)
    assert same_bits(gpu_engine.spline_prefilter(vol), prefilter(vol))


@pytest.mark.parametrize("mode", ["nearest", "linear", "cubic", "label_linear"])
def test_several_workgroups_and_tiles(gpu_engine, mode):
    shape = (9, 130, 301)  # five x-pass tiles, the last one partial; three bands of lines per slice, the last one partial
    src = labels_for(shape, 1) if mode == "label_linear" else volume(shape, np.float32 if mode == "linear" else np.int16, 2, special=True)
    for name in ("scale", "rotate", "permute"):
        A, b, dims = maps_for(shape)[name]
        check(gpu_engine, src, A, b, dims, mode, name, fill=3)


def _same(a, b):
    return same_bits(a.image, b.image) and np.array_equal(a.labels, b.labels) and a.meta() == b.meta()


def _expected(eng, image, labels, grid, order=3, label_mode="linear", spacing=None, **kw):
    img = rs.resample_image(image, grid, order=order, spacing=spacing, engine=eng, **kw)
    lab = rs.resample_labels(labels, grid, mode=label_mode, spacing=spacing, engine=eng)
    return rs.Resampled(img.array, lab.array, grid, order, label_mode, True)


@pytest.mark.parametrize("model", ["R231", "LTRCLobes", "LTRCLobes_R231"])
def test_apply_resampled_models(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    fused = model == "LTRCLobes_R231"
    c = 3 if model == "R231" else 6
    kw = dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(c, head="lunglike"),
              fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)
    inf = LMInferer(engine=gpu_engine, **kw)
    vol = syn.phantom(20, 512, 512)
    sp = (2.0, 0.75, 0.75)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 4
    labels, res = inf.apply_resampled(vol, spacing=sp)  # 1 mm isotropic, cubic, label-linear
    assert np.array_equal(labels, expect)
    grid = rs.Grid.isotropic(vol, 1.0, spacing=sp)
    assert res.image.shape == grid.shape == (39, 384, 384) and res.image.dtype == np.float32
    assert _same(res, _expected(gpu_engine, vol, expect, grid, spacing=sp))
    assert set(np.unique(res.labels)) <= set(np.unique(expect))
    gpu_engine.debug_fill_workspaces(0xA5)  # the spline coefficients are workspace: a dirty one changes nothing
    labels2, res2 = inf.apply_resampled(vol, spacing=sp)
    assert np.array_equal(labels2, labels) and _same(res2, res)
    _, lin = inf.apply_resampled(vol, spacing=sp, spacing_out=(2.0, 1.5, 1.5), order=1, label_mode="nearest", dtype=np.int16)
    assert _same(lin, _expected(gpu_engine, vol, expect, rs.Grid.isotropic(vol, (2.0, 1.5, 1.5), spacing=sp), 1, "nearest", spacing=sp, dtype=np.int16))


def test_apply_resampled_non_lps_volume(gpu_engine):
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)  # permuted and flipped
    axes, flips = volume_io.lps_transform(direction)
    arr = np.ascontiguousarray(volume_io.apply_transform(syn.phantom(20, 512, 512), *volume_io.inverse_transform(axes, flips)))
    img = volume_io.Volume(arr, (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), direction)
    expect = inf.apply(img).copy()
    labels, res = inf.apply_resampled(img, spacing_out=1.5)
    assert np.array_equal(labels, expect) and (expect > 0).any()
    grid = rs.Grid.isotropic(img, 1.5)
    assert _same(res, _expected(gpu_engine, img, img.like(expect), grid))
    v = res.as_volume()
    assert v.origin == img.origin and np.array_equal(v.direction, img.direction) and v.spacing == (1.5, 1.5, 1.5)
    # onto an axis-aligned LPS grid covering the same box: the map is a permutation with a flip
    corners = np.array([img.index_to_physical(c) for c in ((0, 0, 0), tuple(s - 1 for s in img.GetSize()))])
    lo, hi = corners.min(0), corners.max(0)
    lps = rs.Grid(tuple(int(v) for v in np.floor((hi - lo)[::-1] / 2.0) + 1), (2.0, 2.0, 2.0), tuple(lo))
    _, onto = inf.apply_resampled(img, like=lps, order=1)
    assert _same(onto, _expected(gpu_engine, img, img.like(expect), lps, order=1)) and (onto.labels > 0).any()


def test_apply_resampled_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(20, 512, 512)
    single = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, r1 = single.apply_resampled(vol, spacing=(2.0, 0.8, 0.8), spacing_out=1.2)
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, r2 = inf.apply_resampled(vol, spacing=(2.0, 0.8, 0.8), spacing_out=1.2)
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and _same(r2, r1)


def test_cli_resampled(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.7, 0.7, 2.0), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    loaded = volume_io.load_input_image(str(ip))
    ref_labels, ref = LMInferer(modelpath=str(wp), engine=gpu_engine).apply_resampled(loaded, spacing_out=1.4)
    rp, lp = tmp_path / "r.nii.gz", tmp_path / "l.nii.gz"
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--resampled", str(rp), "--resampled-labels", str(lp),
                 "--resample-spacing", "1.4"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    for path, want in ((rp, ref.as_volume()), (lp, ref.labels_volume())):
        back = volume_io.load_input_image(str(path))
        assert back.array.dtype == want.array.dtype and same_bits(np.ascontiguousarray(back.array), want.array)
        np.testing.assert_allclose(back.spacing, (1.4, 1.4, 1.4), atol=1e-6)
        np.testing.assert_allclose(back.origin, loaded.origin, atol=1e-4)
        np.testing.assert_allclose(back.direction, loaded.direction, atol=1e-6)
    # beside --stats, onto the grid of another image, linear
    like = volume_io.Volume(np.zeros((10, 100, 120), np.int16), (2.5, 2.5, 3.0), (20.0, 30.0, 5.0))
    volume_io.write_nifti(str(tmp_path / "like.nii.gz"), like)
    assert main([str(ip), str(tmp_path / "out2.npy"), "--modelpath", str(wp), "--noprogress", "--resampled", str(tmp_path / "r2.npy"),
                 "--resample-like", str(tmp_path / "like.nii.gz"), "--resample-order", "1", "--stats", str(tmp_path / "s.json")]) == 0
    grid = rs.Grid.of(volume_io.load_input_image(str(tmp_path / "like.nii.gz")))
    assert same_bits(np.load(tmp_path / "r2.npy"), rs.resample_image(loaded, grid, order=1, engine=gpu_engine).array)
    assert (tmp_path / "s.json").exists()
