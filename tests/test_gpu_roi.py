"""The lung ROI on the MI355X: lm_roi_dev bit for bit against the numpy oracle of tests/test_roi_emu.py (random volumes of every
dtype, the full 300 x 512 x 512 phantom with lung-like labels as a crop and at 1 mm isotropic), LMInferer.apply_roi (R231, LTRCLobes,
the fused mode, a non-LPS Volume, several engines) and the CLI's --roi / --roi-spacing round trip."""
import numpy as np
import pytest
import torch

from lungmask_amd import roi as lmroi
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_roi_emu import blobs, check, same_bits, volume

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64, np.float32, np.float64])
def test_roi_dev_random_volumes(gpu_engine, dtype):
    sp = (2.5, 0.7, 0.8)
    for shape, seed in (((11, 37, 45), 1), ((24, 96, 128), 2), ((9, 130, 301), 3)):
        vol, lab = volume(shape, dtype, seed, special=True), blobs(shape, seed + 10, n_labels=3)
        check(gpu_engine, vol, lab, ("crop", shape), spacing=sp, margin_mm=2.0)
        check(gpu_engine, vol, lab, ("iso", shape), spacing=sp, spacing_out=1.0, margin_mm=3.0)
        check(gpu_engine, vol, lab, ("aniso", shape), spacing=sp, spacing_out=(1.3, 1.9, 0.5), margin_mm=1.0, keep=[1, 3])
        check(gpu_engine, vol, lab, ("f16 window", shape), spacing=sp, spacing_out=1.0, window=(-1000.0, 400.0), dtype=np.float16)
        check(gpu_engine, vol, lab, ("dilate", shape), spacing=sp, spacing_out=(1.25, 1.0, 1.0), margin_mm=4.0, dilate_mm=3.0)
        check(gpu_engine, vol, lab, ("unmasked", shape), spacing=sp, spacing_out=0.9, mask_outside=False)
        if np.dtype(dtype).kind == "i":
            check(gpu_engine, vol, lab, ("i16", shape), spacing=sp, spacing_out=1.0, dtype=np.int16, fill=-2000)


def _lunglike_labels(gpu_engine, vol, classes=3):
    gpu_engine.load_state_dict(0, syn.synthetic_state_dict(classes, head="lunglike"))
    return gpu_engine.apply(0, vol)


def test_roi_dev_full_phantom(gpu_engine):
    """300 x 512 x 512 with the lung-like head: the crop form and the 1 mm isotropic form."""
    vol = syn.phantom(300, 512, 512)
    lab = _lunglike_labels(gpu_engine, vol)
    assert (lab == 1).sum() > 10 ** 6 and (lab == 2).sum() > 10 ** 6
    sp = (1.25, 0.7, 0.7)
    img, out_lab, info = check(gpu_engine, vol, lab, "phantom crop", spacing=sp)
    b = info["bbox"]
    assert np.array_equal(out_lab, lab[b[0]:b[1], b[2]:b[3], b[4]:b[5]])
    img, out_lab, info = check(gpu_engine, vol, lab, "phantom 1 mm", spacing=sp, spacing_out=1.0)
    assert info["spacing_mm"] == [1.0, 1.0, 1.0] and img.shape[0] > b[1] - b[0] and img.shape[2] < b[5] - b[4]
    check(gpu_engine, vol, lab, "phantom 1 mm dilated f16", spacing=sp, spacing_out=1.0, dilate_mm=3.0, dtype=np.float16)


def _same_roi(a, b):
    return same_bits(a.image, b.image) and np.array_equal(a.labels, b.labels) and a.meta() == b.meta()


@pytest.mark.parametrize("model", ["R231", "LTRCLobes", "LTRCLobes_R231"])
def test_apply_roi_models(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    fused = model == "LTRCLobes_R231"
    c = 3 if model == "R231" else 6
    kw = dict(modelname="LTRCLobes" if fused else model, state_dict=syn.synthetic_state_dict(c, head="lunglike"),
              fillmodel="R231" if fused else None, fill_state_dict=syn.synthetic_state_dict(3, head="lunglike") if fused else None)
    inf = LMInferer(engine=gpu_engine, **kw)
    vol = syn.phantom(60, 512, 512)
    expect = inf.apply(vol).copy()
    assert (expect > 0).sum() > 10 ** 5
    args = dict(spacing=(2.0, 0.75, 0.75), spacing_out=1.0, window=(-1000.0, 400.0))
    labels, roi = inf.apply_roi(vol, **args)
    assert np.array_equal(labels, expect)
    assert _same_roi(roi, lmroi.extract_roi(vol, expect, engine=gpu_engine, **args))
    assert roi.image.shape == roi.labels.shape and set(np.unique(roi.labels)) <= set(np.unique(expect))
    labels2, roi2 = inf.apply_roi(vol, **args)  # two identical calls, identical results
    assert np.array_equal(labels2, labels) and _same_roi(roi2, roi)
    labels3, crop = inf.apply_roi(vol)  # no spacing: a pure crop with the margin in voxels
    assert np.array_equal(labels3, expect) and _same_roi(crop, lmroi.extract_roi(vol, expect, engine=gpu_engine))
    with pytest.raises(ValueError, match="no voxel"):
        inf.apply_roi(vol, keep=[200])


def test_apply_roi_non_lps_volume(gpu_engine):
    """The ROI of a non-LPS Volume is in the caller's index order and its physical space."""
    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(40, 512, 512)
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)  # permuted and flipped
    axes, flips = volume_io.lps_transform(direction)
    arr = np.ascontiguousarray(volume_io.apply_transform(vol, *volume_io.inverse_transform(axes, flips)))
    img = volume_io.Volume(arr, (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), direction)
    expect = inf.apply(img).copy()
    labels, roi = inf.apply_roi(img, spacing_out=1.0, dilate_mm=2.0)
    assert np.array_equal(labels, expect)
    assert _same_roi(roi, lmroi.extract_roi(img, expect, spacing_out=1.0, dilate_mm=2.0, engine=gpu_engine))
    z, y, x = np.nonzero(expect)
    m = [2, 7, 8]  # ceil(5 / (2.5, 0.8, 0.7))
    want = [max(int(z.min()) - m[0], 0), min(int(z.max()) + 1 + m[0], arr.shape[0]), max(int(y.min()) - m[1], 0),
            min(int(y.max()) + 1 + m[1], arr.shape[1]), max(int(x.min()) - m[2], 0), min(int(x.max()) + 1 + m[2], arr.shape[2])]
    assert roi.bbox == want and roi.spacing_mm == [1.0, 1.0, 1.0] and roi.source_step == [1 / 2.5, 1 / 0.8, 1 / 0.7]
    v = roi.as_volume()
    np.testing.assert_allclose(v.origin, img.index_to_physical([want[4], want[2], want[0]]), atol=1e-9)
    assert np.array_equal(v.direction, img.direction) and v.spacing == (1.0, 1.0, 1.0)


def test_apply_roi_several_engines(gpu_engine):
    from lungmask_amd.mask import LMInferer

    sd = syn.synthetic_state_dict(3, head="lunglike")
    vol = syn.phantom(25, 512, 512)
    single = LMInferer(state_dict=sd, engine=gpu_engine)
    lab1, r1 = single.apply_roi(vol, spacing=(2.0, 0.8, 0.8), spacing_out=1.2)
    inf = LMInferer(state_dict=sd, device_ids=[0, 0])
    try:
        lab2, r2 = inf.apply_roi(vol, spacing=(2.0, 0.8, 0.8), spacing_out=1.2)
    finally:
        inf.close()
    assert np.array_equal(lab2, lab1) and _same_roi(r2, r1)


def test_cli_roi(gpu_engine, tmp_path):
    from lungmask_amd import LMInferer
    from lungmask_amd.__main__ import main

    sd = syn.synthetic_state_dict(3, head="lunglike")
    wp = tmp_path / "w.pth"
    torch.save(sd, wp)
    img = volume_io.Volume(syn.phantom(20, 512, 512), (0.7, 0.7, 2.0), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    loaded = volume_io.load_input_image(str(ip))
    ref_labels, ref = LMInferer(modelpath=str(wp), engine=gpu_engine).apply_roi(loaded, spacing_out=1.0)
    rp = tmp_path / "roi.nii.gz"
    assert main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(wp), "--noprogress", "--roi", str(rp), "--roi-spacing", "1.0"]) == 0
    assert np.array_equal(np.load(tmp_path / "out.npy"), ref_labels)
    back = volume_io.load_input_image(str(rp))
    assert back.array.dtype == np.float32 and same_bits(np.ascontiguousarray(back.array), ref.image)
    want = ref.as_volume()
    np.testing.assert_allclose(back.spacing, (1.0, 1.0, 1.0), atol=1e-6)
    np.testing.assert_allclose(back.origin, want.origin, atol=1e-4)
    np.testing.assert_allclose(back.origin, loaded.index_to_physical([ref.bbox[4], ref.bbox[2], ref.bbox[0]]), atol=1e-4)
    np.testing.assert_allclose(back.direction, loaded.direction, atol=1e-6)
    # beside --stats and --probabilities, as a crop, into the other containers
    assert main([str(ip), str(tmp_path / "out2.npy"), "--modelpath", str(wp), "--noprogress", "--roi", str(tmp_path / "roi.mha"),
                 "--stats", str(tmp_path / "s.json"), "--probabilities", str(tmp_path / "p.npy")]) == 0
    crop = lmroi.extract_roi(loaded, ref_labels, engine=gpu_engine)
    mha = volume_io.load_input_image(str(tmp_path / "roi.mha"))
    assert same_bits(np.ascontiguousarray(mha.array), crop.image) and (tmp_path / "s.json").exists()
    np.testing.assert_allclose(mha.spacing, loaded.spacing, atol=1e-6)
    assert main([str(ip), str(tmp_path / "out3.npy"), "--modelpath", str(wp), "--noprogress", "--roi", str(tmp_path / "roi.npy")]) == 0
    assert same_bits(np.load(tmp_path / "roi.npy"), crop.image)
