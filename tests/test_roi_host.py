"""The Python layer of the lung ROI (lungmask_amd.roi) on the emulator engine: geometry of the result for numpy, Volume and non-LPS
Volume input, the argument errors, the JSON form of the meta data, and the CLI's --roi / --roi-spacing refusals."""
import json

import numpy as np
import pytest

from lungmask_amd import roi as lmroi
from lungmask_amd import volume_io


def _case(shape=(9, 30, 36)):
    rng = np.random.default_rng(5)
    vol = rng.integers(-1200, 800, shape).astype(np.int16)
    lab = np.zeros(shape, np.uint8)
    lab[2:7, 6:22, 9:30] = 1
    lab[3:6, 8:12, 12:20] = 2
    return vol, lab


def test_numpy_input_fields_and_meta(emu_engine):
    vol, lab = _case()
    r = lmroi.extract_roi(vol, lab, spacing=(2.0, 1.0, 0.5), spacing_out=1.0, margin_mm=2.0, engine=emu_engine)
    assert r.bbox == [1, 8, 4, 24, 5, 34]  # grown by ceil(2 / s_i) = 1, 2, 4 voxels
    assert r.spacing_mm == [1.0, 1.0, 1.0] and r.source_step == [0.5, 1.0, 2.0]
    assert r.image.dtype == np.float32 and r.labels.dtype == np.uint8 and r.image.shape == r.labels.shape == (13, 20, 15)
    assert set(np.unique(r.labels)) == {0, 1, 2} and np.all(r.image[r.labels == 0] == -1024)
    m = r.meta()
    assert json.loads(json.dumps(m)) == m
    assert m == {"shape": [13, 20, 15], "dtype": "float32", "bbox": r.bbox, "spacing_mm": [1.0, 1.0, 1.0], "source_step": [0.5, 1.0, 2.0]}
    with pytest.raises(ValueError, match="geometry"):
        r.as_volume()
    crop = lmroi.extract_roi(vol, lab, margin_mm=1, keep=[2], mask_outside=False, dtype=np.int16, engine=emu_engine)  # no spacing at all
    assert crop.bbox == [2, 7, 7, 13, 11, 21] and crop.spacing_mm is None and crop.source_step == [1.0, 1.0, 1.0]
    assert np.array_equal(crop.image, vol[2:7, 7:13, 11:21]) and np.array_equal(crop.labels, lab[2:7, 7:13, 11:21])
    assert json.loads(json.dumps(crop.meta()))["spacing_mm"] is None


@pytest.mark.parametrize("direction", [None, (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)])
def test_volume_geometry(emu_engine, direction):
    """as_volume(): the origin is index_to_physical of the box's first voxel, the direction the input's (no LPS re-orientation)."""
    vol, lab = _case()
    img = volume_io.Volume(vol, (0.5, 1.0, 2.0), (-12.0, 30.0, 4.5), direction)  # spacing in (x, y, z) order
    r = lmroi.extract_roi(img, lab, spacing_out=(1.0, 1.5, 0.75), margin_mm=2.0, engine=emu_engine)
    assert r.bbox == [1, 8, 4, 24, 5, 34] and r.spacing_mm == [1.0, 1.5, 0.75]
    v = r.as_volume()
    assert v.array is r.image and v.spacing == (0.75, 1.5, 1.0)
    np.testing.assert_allclose(v.origin, img.index_to_physical([5, 4, 1]), rtol=0, atol=1e-12)
    assert np.array_equal(v.direction, img.direction)
    # a voxel of the ROI lies where its source coordinate lies
    o = np.array([3, 2, 4])  # (z, y, x) in the ROI
    src_index = np.array(r.bbox[::2]) + o * np.array(r.source_step)
    np.testing.assert_allclose(v.index_to_physical(o[::-1]), img.index_to_physical(src_index[::-1]), rtol=0, atol=1e-9)
    lv = r.as_volume(r.labels)
    assert lv.array is r.labels and lv.origin == v.origin
    same = lmroi.extract_roi(img, volume_io.Volume(lab, img.spacing, img.origin, direction), spacing_out=(1.0, 1.5, 0.75), margin_mm=2.0,
                             engine=emu_engine)
    assert np.array_equal(same.image, r.image) and same.bbox == r.bbox
    arr = lmroi.extract_roi(vol, lab, spacing=(2.0, 1.0, 0.5), spacing_out=(1.0, 1.5, 0.75), margin_mm=2.0, engine=emu_engine)
    assert np.array_equal(arr.image, r.image) and np.array_equal(arr.labels, r.labels)  # the same grid from the bare array


def test_argument_errors(emu_engine):
    vol, lab = _case()
    img = volume_io.Volume(vol, (0.5, 1.0, 2.0))
    with pytest.raises(ValueError, match="spacing is taken from the image"):
        lmroi.extract_roi(img, lab, spacing=(1.0, 1.0, 1.0), engine=emu_engine)
    with pytest.raises(ValueError, match="spacing_out needs the source spacing"):
        lmroi.extract_roi(vol, lab, spacing_out=1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="spacing_out"):
        lmroi.extract_roi(vol, lab, spacing=(1.0, 1.0, 1.0), spacing_out=(1.0, 2.0), engine=emu_engine)
    with pytest.raises(ValueError, match="spacing_out"):
        lmroi.extract_roi(vol, lab, spacing=(1.0, 1.0, 1.0), spacing_out=-1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="one value per array axis"):
        lmroi.extract_roi(vol, lab, spacing=(1.0, 1.0), engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        lmroi.extract_roi(vol, lab[1:], engine=emu_engine)
    with pytest.raises(ValueError, match="dilate_mm"):
        lmroi.extract_roi(vol, lab, margin_mm=1.0, dilate_mm=1.5, engine=emu_engine)
    with pytest.raises(ValueError, match="dilate_mm"):
        lmroi.extract_roi(vol, lab, dilate_mm=-1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="1..255"):
        lmroi.extract_roi(vol, lab, keep=[0, 1], engine=emu_engine)
    with pytest.raises(ValueError, match="window"):
        lmroi.extract_roi(vol, lab, window=(400, -1000), engine=emu_engine)
    with pytest.raises(TypeError, match="dtype"):
        lmroi.extract_roi(vol, lab, dtype=np.float64, engine=emu_engine)
    with pytest.raises(ValueError, match="int16"):
        lmroi.extract_roi(vol.astype(np.float32), lab, dtype=np.int16, engine=emu_engine)
    with pytest.raises(ValueError, match="no voxel"):
        lmroi.extract_roi(vol, lab, keep=[7], engine=emu_engine)
    with pytest.raises(ValueError, match="0..255"):
        lmroi.extract_roi(vol, lab.astype(np.int32) * 300, engine=emu_engine)


def test_other_input_dtypes_are_widened(emu_engine):
    vol, lab = _case()
    u8 = (vol & 0xFF).astype(np.uint8)
    r = lmroi.extract_roi(u8, lab.astype(np.int64), margin_mm=0, mask_outside=False, engine=emu_engine)
    assert np.array_equal(r.image, u8[2:7, 6:22, 9:30].astype(np.float32))


def test_cli_roi_arguments(tmp_path):
    from lungmask_amd.__main__ import build_parser, main

    ip = tmp_path / "in.npy"
    np.save(ip, np.zeros((2, 4, 4), np.int16))
    out = str(tmp_path / "out.nii")
    args = build_parser().parse_args([str(ip), out, "--roi", "r.nii.gz", "--roi-spacing", "1.5"])
    assert args.roi == "r.nii.gz" and args.roi_spacing == 1.5
    assert build_parser().parse_args([str(ip), out]).roi is None
    for bad in ("roi.txt", "roi.json", "roi.nrrd"):
        with pytest.raises(SystemExit, match="--roi"):  # before any model is loaded (no GPU needed to get here)
            main([str(ip), out, "--roi", str(tmp_path / bad)])
    with pytest.raises(SystemExit, match="--roi-spacing"):
        main([str(ip), out, "--roi-spacing", "1.0"])
    with pytest.raises(SystemExit, match="--roi-spacing"):
        main([str(ip), out, "--roi", str(tmp_path / "r.npy"), "--roi-spacing", "0"])
    for m in ("R231", "LTRCLobes", "LTRCLobes_R231", "R231CovidWeb"):  # every model name parses with the flags
        assert build_parser().parse_args([str(ip), out, "--modelname", m, "--roi", "r.mha", "--stats", "s.json"]).roi == "r.mha"
    assert not (tmp_path / "out.nii").exists()
