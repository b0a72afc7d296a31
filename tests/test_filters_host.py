"""The Python layer of the image filters (lungmask_amd.filters) on the emulator engine: the Gaussian taps, the unmasked filters against
scipy.ndimage, the properties of the masked forms and of the low-attenuation map, geometry and dtype plumbing, and the command line."""
import json

import numpy as np
import pytest
from scipy import ndimage

from lungmask_amd import components as cp
from lungmask_amd import filters as flt
from lungmask_amd import stats as lmstats
from lungmask_amd import volume_io
from tests.cli_fake import FakeInferer
from tests.test_components_host import cubes_volume
from tests.test_filters_emu import assert_same_bits, lung_labels, volume

EPS = 2.0 ** -24


def test_gaussian_taps():
    for s in (0.3, 0.7, 1.0, 2.5, 8.0):
        t0, t1, t2 = (flt.gaussian_taps(s, order) for order in (0, 1, 2))
        r = int(4.0 * s + 0.5)
        assert t0.dtype == np.float32 and t0.shape == t1.shape == t2.shape == (2 * r + 1,)
        assert abs(float(t0.astype(np.float64).sum()) - 1.0) <= (2 * r + 1) * EPS  # each tap is rounded once
        assert np.array_equal(t0, t0[::-1]) and np.array_equal(t2, t2[::-1]) and np.array_equal(t1, -t1[::-1])
        assert t1[r] == 0 and (t1[r + 1:] >= 0).all() and t0.argmax() == r
    assert flt.gaussian_taps(0).tolist() == [1.0] and flt.gaussian_taps(0.1).tolist() == [1.0]
    assert flt.gaussian_taps(1.0, truncate=2.0).size == 5 and flt.gaussian_taps(8.12).size == 65
    for bad in (dict(sigma_vox=0, order=1), dict(sigma_vox=-1.0), dict(sigma_vox=1.0, order=3), dict(sigma_vox=1.0, truncate=0)):
        with pytest.raises(ValueError):
            flt.gaussian_taps(**bad)
    with pytest.raises(ValueError, match="limit is 32"):
        flt.gaussian_taps(8.2)


def test_gaussian_against_scipy(emu_engine):
    x = volume((12, 40, 70), np.int16, 5)
    peak = float(np.abs(x).max())
    for sigma in (1.0, 2.0):
        r = int(4 * sigma + 0.5)
        got = flt.gaussian(x, sigma, engine=emu_engine)
        want = ndimage.gaussian_filter(x.astype(np.float64), sigma, mode="nearest", truncate=4)
        # a-priori bound of sequential float32 summation per pass: (2 r + 2) 2^-24 max|x| (2 r + 1 products and the tap's rounding, sum of
        # taps 1); three passes; the bar is twice the bound
        assert got.dtype == np.float32 and np.abs(got - want).max() <= 6 * (2 * r + 2) * EPS * peak
    # sigma in millimetres: one value over an anisotropic spacing = three sigmas in voxels
    sp = (2.0, 1.0, 0.5)
    got = flt.gaussian(x.astype(np.float32), 2.0, spacing=sp, engine=emu_engine)
    want = ndimage.gaussian_filter(x.astype(np.float64), (1.0, 2.0, 4.0), mode="nearest", truncate=4)
    assert np.abs(got - want).max() <= 2 * sum(2 * r + 2 for r in (4, 8, 16)) * EPS * peak
    assert_same_bits(flt.gaussian(x, (1.0, 2.0, 4.0), engine=emu_engine), flt.gaussian(x, 2.0, spacing=sp, engine=emu_engine))
    assert_same_bits(flt.gaussian(x, 0, engine=emu_engine), x.astype(np.float32))  # sigma 0: the conversion alone


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gaussian_derivatives(emu_engine, axis):
    shape = [6, 7, 9]
    shape[axis] = 70
    i = np.arange(70, dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
    sigma, trunc = 1.5, 6.0  # truncate 6: the discrete operator equals the derivative to 1e-7, far below the bar
    r = int(trunc * sigma + 0.5)
    sig = [sigma if a == axis else 0.0 for a in range(3)]
    inner = [slice(r, 70 - r) if a == axis else slice(None) for a in range(3)]
    for order, fn, want in ((1, 3.0 * i - 50.0, 3.0), (1, 20.0 - 2.0 * i, -2.0), (2, 0.5 * i * i, 1.0), (2, 100.0 - 0.25 * i * i, -0.5)):
        x = np.broadcast_to(fn, shape).astype(np.float32)
        assert np.array_equal(x, np.broadcast_to(fn, shape))  # exact in float32
        got = flt.gaussian(x, sig, order=[order if a == axis else 0 for a in range(3)], truncate=trunc, engine=emu_engine)[tuple(inner)]
        bar = 6 * (2 * r + 2) * EPS * float(np.abs(x).max()) * float(np.abs(flt.gaussian_taps(sigma, order, trunc)).sum())
        assert np.sign(got).min() == np.sign(got).max() == np.sign(want)
        assert np.abs(got - want).max() <= bar, (order, np.abs(got - want).max(), bar)


def test_median_against_scipy(emu_engine):
    for dtype in (np.int16, np.int32):
        x = volume((6, 33, 70), dtype, 8)
        for size in (3, 5, (1, 3, 3), (5, 1, 3)):
            got = flt.median(x, size, engine=emu_engine)
            assert got.dtype == x.dtype and np.array_equal(got, ndimage.median_filter(x, size=size, mode="nearest"))


def test_masked_forms_stop_at_the_pleura(emu_engine):
    lab = np.zeros((6, 30, 40), np.uint8)
    lab[1:5, 3:27, 2:20] = 1
    lab[1:5, 3:27, 21:38] = 2
    x = np.full(lab.shape, 1000, np.int16)  # chest wall and mediastinum
    x[lab > 0] = -512  # a constant lung (a power of two: num = c * den exactly, so num / den is exact)
    inside = lab > 0
    g = flt.gaussian(x, 1.5, labels=lab, engine=emu_engine)
    assert (g[inside] == -512.0).all() and (g[~inside] == 1000.0).all()
    plain = flt.gaussian(x, 1.5, engine=emu_engine)
    assert (plain[inside] > -511.0).any()  # without the labels the wall leaks into the lung
    m = flt.median(x, 5, labels=lab, engine=emu_engine)
    assert np.array_equal(m, x) and (flt.median(x, 5, engine=emu_engine)[inside] == 1000).any()
    one = flt.gaussian(x, 1.5, labels=lab, keep=(1,), fill=-7.0, engine=emu_engine)
    assert (one[lab == 1] == -512.0).all() and (one[lab != 1] == -7.0).all()
    assert (flt.median(x, 3, labels=lab, fill=-1024, engine=emu_engine)[~inside] == -1024).all()
    with pytest.raises(ValueError, match="order 0"):
        flt.gaussian(x, 1.5, order=1, labels=lab, engine=emu_engine)
    for fn in (lambda: flt.gaussian(x, 1.0, labels=np.zeros_like(lab), engine=emu_engine),
               lambda: flt.median(x, 3, labels=lab, keep=(5,), engine=emu_engine),
               lambda: flt.low_attenuation_map(x, np.zeros_like(lab), engine=emu_engine)):
        with pytest.raises(ValueError, match="no voxel"):
            fn()


def test_low_attenuation_map(emu_engine):
    shape = (6, 33, 70)
    lab = lung_labels(shape, 4)
    sel = lab > 0
    for dtype in (np.int16, np.float32):
        x = volume(shape, dtype, 6)
        m = flt.low_attenuation_map(x, lab, sigma_mm=2.0, spacing=(2.0, 1.0, 1.0), engine=emu_engine)
        assert m.dtype == np.float32 and (m[~sel] == 0).all() and m[sel].min() >= 0 and m[sel].max() <= 1
        assert 0 < m[sel].mean() < 1
    low = np.full(shape, -1000, np.int16)
    assert (flt.low_attenuation_map(low, lab, sigma_mm=1.5, engine=emu_engine)[sel] == 1.0).all()  # num == den bit for bit
    assert not flt.low_attenuation_map(low, lab, threshold=-1000, sigma_mm=1.5, engine=emu_engine).any()  # hu < threshold is strict
    hi = flt.low_attenuation_map(low, lab, hu_range=(-1000, None), sigma_mm=1.5, engine=emu_engine)
    assert (hi[sel] == 1.0).all() and (hi[~sel] == 0).all()
    # sigma 0: the indicator itself -- the voxels that the statistics count in below[-950]
    x = volume(shape, np.int16, 6)
    m0 = flt.low_attenuation_map(x, lab, sigma_mm=0, engine=emu_engine)
    assert np.array_equal(m0, (sel & (x < -950)).astype(np.float32))
    st = lmstats.label_statistics(x, (lab > 0).astype(np.uint8), engine=emu_engine)
    assert m0[sel].mean(dtype=np.float64) == pytest.approx(st["labels"]["1"]["below"]["-950"], rel=1e-12)
    with pytest.raises(ValueError, match="threshold"):
        flt.low_attenuation_map(x, lab, threshold=-950.5, engine=emu_engine)
    with pytest.raises(ValueError, match="limit is 32"):
        flt.low_attenuation_map(x, lab, sigma_mm=5.0, spacing=(0.5, 0.5, 0.5), engine=emu_engine)


def test_geometry_and_dtypes(emu_engine):
    shape = (5, 20, 33)
    x = volume(shape, np.int16, 9)
    lab = lung_labels(shape, 9)
    sp = (2.5, 0.8, 0.7)  # z, y, x
    want = flt.gaussian(x, 1.5, spacing=sp, labels=lab, engine=emu_engine)
    d = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    img = volume_io.Volume(x, sp[::-1], (10.0, 20.0, 30.0), d)  # brings its spacing (x, y, z); the result stays in ITS array order
    assert_same_bits(flt.gaussian(img, 1.5, labels=img.like(lab), engine=emu_engine), want)
    assert_same_bits(flt.low_attenuation_map(img, lab, sigma_mm=2.0, engine=emu_engine),
                     flt.low_attenuation_map(x, lab, sigma_mm=2.0, spacing=sp, engine=emu_engine))
    assert np.array_equal(flt.median(img, 3, labels=lab, engine=emu_engine), flt.median(x, 3, labels=lab, engine=emu_engine))
    with pytest.raises(ValueError, match="spacing"):
        flt.gaussian(img, 1.5, spacing=sp, engine=emu_engine)
    with pytest.raises(ValueError, match="spacing"):
        flt.gaussian(x, 1.5, spacing=(1.0, 2.0), engine=emu_engine)
    with pytest.raises(ValueError, match="same shape"):
        flt.gaussian(x, 1.5, labels=lab[:, :, :5], engine=emu_engine)
    with pytest.raises(ValueError, match="one value or three"):
        flt.gaussian(x, (1.0, 2.0), engine=emu_engine)
    # dtypes: int64 within the int32 range is narrowed, the result keeps the caller's dtype
    m16 = flt.median(x, 3, engine=emu_engine)
    for dtype in (np.int64, np.int32, np.int8, np.uint16):
        xv = (x // 16).astype(dtype) if np.dtype(dtype).itemsize == 1 else (x + 2000).astype(dtype)
        got = flt.median(xv, 3, engine=emu_engine)
        assert got.dtype == dtype and np.array_equal(got, ndimage.median_filter(xv, size=3, mode="nearest"))
    assert np.array_equal(flt.median(x.astype(np.int64), 3, engine=emu_engine), m16.astype(np.int64))
    big = x.astype(np.int64)
    big[0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match="cast the image to float32"):
        flt.median(big, 3, engine=emu_engine)
    with pytest.raises(ValueError, match="cast the image to float32"):
        flt.median(x.astype(np.float64), 3, engine=emu_engine)
    with pytest.raises(ValueError, match="fill"):
        flt.median(x, 3, labels=lab, fill=0.5, engine=emu_engine)
    assert_same_bits(flt.gaussian(big, 1.0, engine=emu_engine), flt.gaussian(big.astype(np.float32), 1.0, engine=emu_engine))


def test_cli_denoise(emu_engine, tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli

    arr, lab = cubes_volume()
    arr = (arr + np.random.default_rng(1).integers(-60, 60, arr.shape)).astype(np.int16)
    img = volume_io.Volume(arr, (0.7, 0.8, 2.5), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    FakeInferer.engine, FakeInferer.labels = emu_engine, lab
    monkeypatch.setattr(cli, "LMInferer", FakeInferer)
    monkeypatch.setattr(emu_engine, "n_classes", lambda slot: 3, raising=False)  # (no model is loaded into the emulated engine)
    loaded = volume_io.load_input_image(str(ip))
    names = lmstats.label_names("R231", 3)
    kw = dict(names=names, engine=emu_engine)
    t = lambda name: str(tmp_path / name)  # noqa: E731
    # without the new flags: the files are what they were
    assert cli.main([str(ip), t("o.npy"), "--noprogress", "--stats", t("s.json"), "--clusters", t("c.json")]) == 0
    assert json.load(open(t("s.json"))) == json.loads(json.dumps(lmstats.label_statistics(loaded, lab, n_labels=3, **kw)))
    assert json.load(open(t("c.json"))) == json.loads(json.dumps(cp.cluster_analysis(loaded, lab, **kw)))
    assert np.array_equal(np.load(t("o.npy")), lab)
    # median: the statistics, the clusters and the ROI measure the filtered image
    assert cli.main([str(ip), t("o2.npy"), "--noprogress", "--denoise", "median", "--stats", t("s2.json"), "--clusters", t("c2.json"),
                     "--denoised", t("d.npy"), "--roi", t("r.npy"), "--laa-map", t("l.nii.gz"), "--laa-sigma", "2",
                     "--cluster-threshold", "-900"]) == 0
    filtered = flt.median(loaded, 3, labels=lab, engine=emu_engine)
    assert np.array_equal(np.load(t("o2.npy")), lab) and np.array_equal(np.load(t("d.npy")), filtered) and not np.array_equal(filtered, arr)
    meta = {"method": "median", "size": 3, "masked": True}
    want = lmstats.label_statistics(loaded.like(filtered), lab, n_labels=3, **kw)
    assert json.load(open(t("s2.json"))) == json.loads(json.dumps(dict(want, denoise=meta)))
    assert want["lung"]["std"] < lmstats.label_statistics(loaded, lab, n_labels=3, **kw)["lung"]["std"]
    wantc = cp.cluster_analysis(loaded.like(filtered), lab, threshold=-900, **kw)
    assert json.load(open(t("c2.json"))) == json.loads(json.dumps(dict(wantc, denoise=meta)))
    from lungmask_amd import roi as lmroi

    assert np.array_equal(np.load(t("r.npy")), lmroi.extract_roi(loaded.like(filtered), lab, engine=emu_engine).image)
    laa = volume_io.load_input_image(t("l.nii.gz"))
    assert laa.array.dtype == np.float32
    assert_same_bits(np.asarray(laa.array), flt.low_attenuation_map(loaded, lab, threshold=-900, sigma_mm=2.0, engine=emu_engine))
    np.testing.assert_allclose(laa.spacing, loaded.spacing, atol=1e-6)
    # gaussian, into an image container; the map alone with its defaults' threshold
    assert cli.main([str(ip), t("o3.npy"), "--noprogress", "--denoise", "gaussian:1.5", "--stats", t("s3.json"), "--denoised", t("d.mha"),
                     "--texture", t("t.json")]) == 0
    g = flt.gaussian(loaded, 1.5, labels=lab, engine=emu_engine)
    assert_same_bits(np.asarray(volume_io.load_input_image(t("d.mha")).array), g)
    meta = {"method": "gaussian", "sigma_mm": 1.5, "masked": True}
    assert json.load(open(t("s3.json"))) == json.loads(json.dumps(dict(lmstats.label_statistics(loaded.like(g), lab, n_labels=3, **kw), denoise=meta)))
    assert json.load(open(t("t.json")))["denoise"] == meta
    assert cli.main([str(ip), t("o4.npy"), "--noprogress", "--laa-map", t("l.npy"), "--laa-sigma", "1.5"]) == 0
    assert_same_bits(np.load(t("l.npy")), flt.low_attenuation_map(loaded, lab, sigma_mm=1.5, engine=emu_engine))
    # no labelled voxel: nothing is filtered, the map is empty
    FakeInferer.labels = np.zeros_like(lab)
    monkeypatch.setattr(FakeInferer, "apply_denoised", lambda self, image, **k: (self.labels.copy(), None))
    assert cli.main([str(ip), t("o5.npy"), "--noprogress", "--denoise", "median:5", "--denoised", t("d5.npy"), "--laa-map", t("l5.npy"),
                     "--laa-sigma", "1.5"]) == 0
    assert np.array_equal(np.load(t("d5.npy")), arr) and not np.load(t("l5.npy")).any()
    out = t("o6.npy")
    for bad in (["--denoise", "mean"], ["--denoise", "median:4"], ["--denoise", "gaussian"], ["--denoise", "gaussian:-1"],
                ["--denoised", "d.npy"], ["--denoise", "median", "--denoised", "d.txt"]):
        with pytest.raises(SystemExit, match="--denoise"):  # refused before anything is loaded
            cli.main([str(ip), out] + bad)
    for bad in (["--laa-sigma", "2"], ["--laa-map", "l.txt"], ["--laa-map", "l.npy", "--laa-sigma", "0"]):
        with pytest.raises(SystemExit, match="--laa"):
            cli.main([str(ip), out] + bad)
    a = cli.build_parser().parse_args([str(ip), out, "--denoise", "median:5", "--laa-map", "l.npy", "--modelname", "LTRCLobes_R231",
                                       "--stats", "s.json", "--closed", "c.npy", "--probabilities", "p.npy"])
    assert a.denoise == "median:5" and a.denoised is None and a.laa_sigma is None
