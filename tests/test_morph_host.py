"""The Python layer of the label morphology (lungmask_amd.morphology) on the emulator engine: argument handling, the spacing of a
Volume, array orientation, the errors, and the CLI's --closed / --close-mm parsing."""
import numpy as np
import pytest

from lungmask_amd import morphology as morph
from lungmask_amd import volume_io
from tests.test_morph_emu import oracle_morph, oracle_nearest


def _labels(shape=(6, 14, 20)):
    lab = np.zeros(shape, np.uint8)
    lab[1:5, 3:11, 4:9] = 1
    lab[1:5, 3:11, 11:17] = 2  # a cleft of two columns between the two labels
    lab[2, 6, 6] = 0           # a hole
    lab[0, 0, 19] = 3
    return lab


def test_functions_match_the_oracle(emu_engine):
    lab, sp = _labels(), (2.0, 1.0, 0.5)
    for fn, op in ((morph.dilate, "dilate"), (morph.erode, "erode"), (morph.open_, "open"), (morph.close, "close")):
        got = fn(lab, 1.5, spacing=sp, keep=[1, 2], engine=emu_engine)
        assert got.dtype == np.uint8 and got.shape == lab.shape
        assert np.array_equal(got, oracle_morph(lab, op, 1.5, sp, [1, 2])[0]), op
        assert np.array_equal(fn(lab.astype(np.int64), 1.5, spacing=sp, keep=[1, 2], engine=emu_engine), got), op  # any integer dtype
    closed = morph.close(lab, 1.5, spacing=sp, keep=[1, 2], engine=emu_engine)
    assert closed[2, 6, 6] == 1 and closed[0, 0, 19] == 3 and (closed != lab).sum() > 1
    assert np.array_equal(morph.close(lab, 1.5, spacing=sp, keep=[1, 2], into=(), engine=emu_engine), lab)  # nothing may be overwritten
    assert np.array_equal(morph.close(lab, 0.0, engine=emu_engine), lab)


def test_nearest_label_and_propagate(emu_engine):
    lab, sp = _labels(), (2.0, 1.0, 0.5)
    d2, want = oracle_nearest(lab, [1, 2], sp)
    near = morph.nearest_label(lab, spacing=sp, keep=[1, 2], engine=emu_engine)
    assert near.dtype == np.uint8 and np.array_equal(near, want)
    near2, dist = morph.nearest_label(lab, spacing=sp, keep=[1, 2], return_distance=True, engine=emu_engine)
    assert np.array_equal(near2, want) and dist.dtype == np.float32 and np.array_equal(dist, np.sqrt(d2))
    assert not morph.nearest_label(np.zeros((2, 3, 4), np.uint8), engine=emu_engine).any()
    everywhere = morph.propagate(lab, keep=[1, 2], into=(0, 3), spacing=sp, engine=emu_engine)
    assert np.array_equal(everywhere, want)  # kept voxels are their own nearest label
    assert np.array_equal(morph.propagate(lab, keep=[1, 2], spacing=sp, engine=emu_engine), np.where(lab == 0, want, lab))
    near_by = morph.propagate(lab, keep=[1, 2], max_mm=1.0, spacing=sp, engine=emu_engine)
    assert np.array_equal(near_by, oracle_morph(lab, "dilate", 1.0, sp, [1, 2])[0])


def test_volume_brings_its_spacing(emu_engine):
    lab = _labels()
    img = volume_io.Volume(lab, (0.5, 1.0, 2.0), (-12.0, 30.0, 4.5))  # spacing in (x, y, z) order
    want = morph.close(lab, 1.5, spacing=(2.0, 1.0, 0.5), engine=emu_engine)
    got = morph.close(img, 1.5, engine=emu_engine)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert not np.array_equal(got, morph.close(lab, 1.5, engine=emu_engine))  # (the spacing matters here)
    with pytest.raises(ValueError, match="spacing"):
        morph.close(img, 1.5, spacing=(2.0, 1.0, 0.5), engine=emu_engine)
    with pytest.raises(ValueError, match="spacing"):
        morph.nearest_label(img, spacing=(2.0, 1.0, 0.5), engine=emu_engine)


def test_permuted_image_keeps_the_callers_orientation(emu_engine):
    """A Volume with a permuted, flipped direction: the result is indexed like its array (no LPS re-orientation), and the spacing
    follows the array's axes -- the erosion of the transposed array with the permuted spacing is the transposed erosion."""
    lab = _labels()
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)
    img = volume_io.Volume(lab, (0.5, 1.0, 2.0), (0.0, 0.0, 0.0), direction)
    want = morph.erode(lab, 1.0, spacing=(2.0, 1.0, 0.5), engine=emu_engine)
    assert np.array_equal(morph.erode(img, 1.0, engine=emu_engine), want)
    perm = np.ascontiguousarray(lab.transpose(2, 0, 1))
    back = morph.erode(perm, 1.0, spacing=(0.5, 2.0, 1.0), engine=emu_engine).transpose(1, 2, 0)
    assert np.array_equal(back, want)  # (powers of two: every distance is exact, whatever the order of the passes)


def test_errors(emu_engine):
    lab = _labels()
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="radius_mm"):
            morph.close(lab, bad, engine=emu_engine)
    with pytest.raises(ValueError, match="max_mm"):
        morph.propagate(lab, max_mm=-1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="keep"):
        morph.dilate(lab, 1.0, keep=[0], engine=emu_engine)
    with pytest.raises(ValueError, match="into"):
        morph.dilate(lab, 1.0, into=[300], engine=emu_engine)
    with pytest.raises(ValueError, match="no voxel"):
        morph.dilate(lab, 1.0, keep=[9], engine=emu_engine)
    from lungmask_amd import _native as nat

    with pytest.raises(nat.NoKeptVoxel):  # (the ValueError apply_closed tells from every other one)
        emu_engine.morph(lab, "close", 1.0, keep=[9])
    with pytest.raises(nat.LMError, match="1e15"):
        emu_engine.morph(lab, "close", 1e15)
    with pytest.raises(ValueError, match="3-D"):
        morph.dilate(lab[0], 1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="integer"):
        morph.dilate(lab.astype(np.float32), 1.0, engine=emu_engine)
    with pytest.raises(ValueError, match="0..255"):
        morph.dilate(lab.astype(np.int32) * 200, 1.0, engine=emu_engine)
    for sp in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, np.inf, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            morph.dilate(lab, 1.0, spacing=sp, engine=emu_engine)


def test_cli_flags(tmp_path):
    from lungmask_amd.__main__ import build_parser, main

    inp = tmp_path / "in.npy"
    np.save(inp, np.zeros((2, 8, 8), np.int16))
    p = build_parser()
    a = p.parse_args([str(inp), "out.nii.gz"])
    assert a.closed is None and a.close_mm is None
    assert (a.modelname, a.batchsize, a.nopostprocess, a.stats, a.roi, a.mesh, a.texture, a.probabilities) == \
        ("R231", 20, False, None, None, None, None, None)  # the old defaults are untouched
    a = p.parse_args([str(inp), "out.nii.gz", "--closed", "c.nii.gz", "--close-mm", "7.5", "--modelname", "LTRCLobes_R231"])
    assert a.closed == "c.nii.gz" and a.close_mm == 7.5
    with pytest.raises(SystemExit, match="--closed"):
        main([str(inp), "out.npy", "--close-mm", "5"])
    for bad in ("-1", "inf", "nan"):
        with pytest.raises(SystemExit, match="--close-mm"):
            main([str(inp), "out.npy", "--closed", "c.npy", "--close-mm", bad])
