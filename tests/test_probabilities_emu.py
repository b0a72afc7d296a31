"""Probability maps un-cropped to the input volume (lm_uncrop_probs_dev) on the g++ emulation of the kernel sources, against the
recipe written in include/lungmask_hip.h: exp of the log-softmax, scipy.ndimage.zoom(order=1) into each slice's box, background
fill outside it -- and the 4-D NIfTI writer of the channel stack (volume_io.write_nifti_channels)."""
import gzip
import struct

import numpy as np
import pytest
import scipy.ndimage as ndi

from lungmask_amd import volume_io


def random_logp(rng, n, c, mh=256, mw=256):
    z = rng.normal(0.0, 3.0, size=(n, c, mh, mw)).astype(np.float32)
    m = z.max(axis=1, keepdims=True)
    return (z - (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))).astype(np.float32)


def oracle_probs(logp, boxes, h, w):
    """The recipe: exp, ndimage.zoom(order=1) to the box, paste; background fill outside the box and where zoom's coordinate lands
    beyond the last source row / column (scipy's cval 0 in every class there, reshape_mask's label 0)."""
    n, c, mh, mw = logp.shape
    out = np.zeros((c, n, h, w), np.float32)
    out[0] = 1.0
    for z in range(n):
        r0, c0, r1, c1 = (int(v) for v in boxes[z])
        zf = ((r1 - r0) / mh, (c1 - c0) / mw)
        inside_ok = ndi.zoom(np.ones((mh, mw), np.float32), zf, order=1) > 0.5
        assert inside_ok.shape == (r1 - r0, c1 - c0)
        for k in range(c):
            p = np.exp(logp[z, k])
            ins = ndi.zoom(p, zf, order=1)
            assert ins.dtype == np.float32
            out[k, z, r0:r1, c0:c1] = np.where(inside_ok, ins, np.float32(1.0 if k == 0 else 0.0))
    return out


CASES = [
    # (C, h, w, boxes): full frame, tiny 1 x k / k x 1, odd sizes, boxes on every edge; w % 4 == 0 and != 0; n == 1
    (3, 40, 36, [(0, 0, 40, 36), (0, 5, 1, 30), (3, 0, 33, 1), (7, 9, 38, 35)]),
    (6, 37, 30, [(0, 0, 37, 30), (12, 17, 25, 30), (36, 0, 37, 29), (1, 1, 2, 2)]),
    (3, 1, 1, [(0, 0, 1, 1)]),
    (6, 300, 277, [(11, 23, 298, 270)]),
    (3, 64, 512, [(2, 0, 64, 512), (0, 3, 63, 509)]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_uncrop_probs_matches_recipe(emu_engine, case):
    C, h, w, boxes = CASES[case]
    rng = np.random.default_rng(100 + case)
    n = len(boxes)
    logp = random_logp(rng, n, C)
    bb = np.asarray(boxes, np.int32)
    got = emu_engine.uncrop_probs(logp, bb, (h, w), np.float32)
    ref = oracle_probs(logp, bb, h, w)
    assert got.shape == (C, n, h, w) and got.dtype == np.float32
    assert float(np.abs(got - ref).max()) <= 1e-6  # expf against np.exp only
    for z, (r0, c0, r1, c1) in enumerate(boxes):
        outside = np.ones((h, w), bool)
        outside[r0:r1, c0:c1] = False
        assert np.all(got[0, z][outside] == 1.0)
        assert np.all(got[1:, z][:, outside] == 0.0)
    assert float(np.abs(got.astype(np.float64).sum(axis=0) - 1.0).max()) <= 1e-6
    g16 = emu_engine.uncrop_probs(logp, bb, (h, w), np.float16)
    assert g16.dtype == np.float16
    assert np.array_equal(g16.view(np.uint16), got.astype(np.float16).view(np.uint16))


def test_uncrop_probs_box_sizes_with_zoom_overshoot(emu_engine):
    """Box sizes for which ndimage.zoom's last coordinate rounds beyond the source (e.g. 12, 14, 23 rows): the fill is written there,
    so the maps still sum to one."""
    sizes = [s for s in range(2, 80) if ndi.zoom(np.ones((256, 1), np.float32), (s / 256, 1), order=1).min() == 0.0]
    assert sizes, "expected some box sizes with scipy's edge overshoot"
    s = sizes[0]
    rng = np.random.default_rng(7)
    logp = random_logp(rng, 2, 3)
    bb = np.asarray([(0, 0, s, 40), (1, 2, 40, 2 + s)], np.int32)
    got = emu_engine.uncrop_probs(logp, bb, (41, 44), np.float32)
    ref = oracle_probs(logp, bb, 41, 44)
    assert float(np.abs(got - ref).max()) <= 1e-6
    assert float(np.abs(got.astype(np.float64).sum(axis=0) - 1.0).max()) <= 1e-6
    assert np.all(got[0, 0, s - 1] == 1.0)


def test_uncrop_probs_refuses_bad_arguments(emu_engine):
    from lungmask_amd import _native as nat

    eng = emu_engine
    logp = eng.to_device(np.zeros((1, 3, 8, 300), np.float32))
    bb = eng.to_device(np.asarray([[0, 0, 4, 4]], np.int32))
    out = eng.empty((3, 1, 4, 4), np.float32)
    try:
        with pytest.raises(nat.LMError, match="mw <= 256"):
            eng.uncrop_probs_dev(logp, bb, out)  # wider than the network resolution
        rc = eng.L.lib.lm_uncrop_probs_dev(eng.h, logp.ptr, bb.ptr, 1, 3, 8, 256, 4, 4, 3, out.ptr)  # LM_F64 output
        assert rc == -1
    finally:
        for d in (logp, bb, out):
            d.free()


def _parse_nifti(path):
    buf = gzip.open(path).read() if path.endswith(".gz") else open(path, "rb").read()
    hdr = dict(
        sizeof_hdr=struct.unpack_from("<i", buf, 0)[0],
        dim=struct.unpack_from("<8h", buf, 40),
        datatype=struct.unpack_from("<h", buf, 70)[0],
        bitpix=struct.unpack_from("<h", buf, 72)[0],
        pixdim=struct.unpack_from("<8f", buf, 76),
        vox_offset=struct.unpack_from("<f", buf, 108)[0],
        codes=struct.unpack_from("<2h", buf, 252),
        quatern=struct.unpack_from("<6f", buf, 256),
        srow=struct.unpack_from("<12f", buf, 280),
        magic=buf[344:348],
    )
    return hdr, buf


@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
def test_write_nifti_channels_header_and_data(tmp_path, ext):
    rng = np.random.default_rng(3)
    n, h, w, c = 5, 7, 9, 3
    d = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    geo = volume_io.Volume(np.zeros((n, h, w), np.int16), spacing=(0.7, 0.8, 2.5), origin=(-10.0, 20.0, 30.0), direction=d)
    stack = rng.random((c, n, h, w), dtype=np.float32)
    p4 = str(tmp_path / ("p" + ext))
    p3 = str(tmp_path / ("m" + ext))
    volume_io.write_nifti_channels(p4, geo, stack)
    volume_io.write_nifti(p3, geo.like(np.zeros((n, h, w), np.uint8)))
    h4, b4 = _parse_nifti(p4)
    h3, _ = _parse_nifti(p3)
    assert h4["sizeof_hdr"] == 348 and h4["magic"] == b"n+1\0"
    assert h4["dim"] == (4, w, h, n, c, 1, 1, 1)
    assert h4["datatype"] == 16 and h4["bitpix"] == 32  # NIFTI_TYPE_FLOAT32
    for k in ("pixdim", "codes", "quatern", "srow", "vox_offset"):
        assert h4[k] == h3[k], k
    data = np.frombuffer(b4, dtype="<f4", count=c * n * h * w, offset=int(h4["vox_offset"])).reshape(c, n, h, w)
    assert np.array_equal(data, stack)
    with pytest.raises(ValueError):
        volume_io.write_nifti_channels(p4, geo, stack[:, :, :, :-1])  # not the geometry's shape


@pytest.mark.parametrize("args", [["--probabilities", "p.mha"], ["--modelname", "LTRCLobes_R231", "--probabilities", "p.npy"]])
def test_cli_probabilities_refused_before_the_model_runs(tmp_path, args):
    from lungmask_amd.__main__ import main

    ip = tmp_path / "in.npy"
    np.save(ip, np.zeros((1, 8, 8), np.int16))
    args = [a if not a.startswith("p.") else str(tmp_path / a) for a in args]
    with pytest.raises(SystemExit) as ex:
        main([str(ip), str(tmp_path / "out.npy"), "--modelpath", str(tmp_path / "missing.pth")] + args)
    assert "--probabilities" in str(ex.value.code)
    assert not (tmp_path / "out.npy").exists()


def test_apply_probabilities_exists_and_apply_is_unchanged():
    import inspect

    from lungmask_amd import LMInferer

    sig = inspect.signature(LMInferer.apply_probabilities)
    assert list(sig.parameters) == ["self", "image", "dtype"] and sig.parameters["dtype"].default is np.float32
    assert list(inspect.signature(LMInferer.apply).parameters) == ["self", "image", "out"]
