"""Per-label statistics (lm_label_stats_dev, Engine.label_stats) on the g++ emulation of the kernel sources, against a numpy
oracle that applies the semantics of include/lungmask_hip.h directly to the arrays: bit for bit on every integer field and on the
histogram."""
import numpy as np
import pytest

from lungmask_amd import _native as nat

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


def oracle_hu(vol: np.ndarray):
    """(hu int64, nan mask): integers as they are, floats rint (half to even) saturated to int32."""
    if vol.dtype.kind == "f":
        nan = np.isnan(vol)
        r = np.rint(vol.astype(np.float64))
        r = np.clip(np.where(nan, 0.0, r), I32_MIN, I32_MAX)
        return r.astype(np.int64), nan
    return vol.astype(np.int64), np.zeros(vol.shape, bool)


def oracle_stats(lab: np.ndarray, vol: np.ndarray, n_labels: int) -> dict:
    hu, nan = oracle_hu(vol)
    out = {f: np.zeros(n_labels, np.int64) for f in ("voxels", "nonfinite", "clipped_low", "clipped_high", "hu_min", "hu_max")}
    out["index_sum"] = np.zeros((n_labels, 3), np.int64)
    out["bbox"] = np.full((n_labels, 6), -1, np.int32)
    out["hist"] = np.zeros((n_labels, 4096), np.int64)
    out["voxels"][0] = int((lab == 0).sum())
    out["other"] = int((lab >= n_labels).sum())
    for k in range(1, n_labels):
        m = lab == k
        out["voxels"][k] = int(m.sum())
        if not m.any():
            continue
        out["nonfinite"][k] = int((m & nan).sum())
        f = m & ~nan
        v = hu[f]
        out["clipped_low"][k] = int((v < -1024).sum())
        out["clipped_high"][k] = int((v > 3071).sum())
        if v.size:
            out["hu_min"][k], out["hu_max"][k] = int(v.min()), int(v.max())
        out["hist"][k] = np.bincount(np.clip(v, -1024, 3071) + 1024, minlength=4096)
        z, y, x = np.nonzero(m)
        out["index_sum"][k] = (int(z.sum()), int(y.sum()), int(x.sum()))
        out["bbox"][k] = (z.min(), z.max() + 1, y.min(), y.max() + 1, x.min(), x.max() + 1)
    return out


def assert_stats_equal(got: dict, want: dict, what=""):
    for f in ("voxels", "nonfinite", "clipped_low", "clipped_high", "hu_min", "hu_max", "index_sum", "bbox", "hist"):
        assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (what, f, got[f], want[f])
    assert got["other"] == want["other"], (what, got["other"], want["other"])


def random_labels(rng, shape, n_labels, extra=0):
    lab = rng.integers(0, n_labels + extra, shape).astype(np.uint8)
    return lab


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64, np.float32, np.float64])
def test_label_stats_dtypes(emu_engine, dtype):
    rng = np.random.default_rng(1)
    shape = (3, 21, 48)
    lab = random_labels(rng, shape, 3, extra=1)
    vol = rng.integers(-1500, 3500, shape).astype(dtype)
    if np.dtype(dtype).kind == "f":
        vol = vol + rng.choice([0.0, 0.25, 0.5, -0.5, 1.5], shape).astype(dtype)
    assert_stats_equal(emu_engine.label_stats(lab, vol, 3), oracle_stats(lab, vol, 3), dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_label_stats_float_specials(emu_engine, dtype):
    """.5 ties (half to even), NaN, +-inf and values beyond the int32 range."""
    rng = np.random.default_rng(2)
    shape = (2, 9, 37)
    lab = random_labels(rng, shape, 4)
    specials = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -950.5, -949.5, 3071.5, -1024.5, np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483647.0,
                         -2147483648.0, 2147483520.0, 1e300 if dtype == np.float64 else 3e38], dtype=np.float64)
    vol = rng.choice(specials, shape).astype(dtype)
    vol[0, 0, :5] = np.nan
    assert_stats_equal(emu_engine.label_stats(lab, vol, 4), oracle_stats(lab, vol, 4), dtype)


@pytest.mark.parametrize("shape", [(1, 16, 16), (1, 5, 7), (2, 3, 33), (4, 13, 50), (3, 11, 64), (1, 1, 1)])
def test_label_stats_shapes(emu_engine, shape):
    """n == 1, w not a multiple of 4 or 16, odd shapes: the scalar tail path and the 16-byte path."""
    rng = np.random.default_rng(3)
    lab = random_labels(rng, shape, 3, extra=2)
    vol = rng.integers(-1100, 3100, shape).astype(np.int16)
    assert_stats_equal(emu_engine.label_stats(lab, vol, 3), oracle_stats(lab, vol, 3), shape)


def test_label_stats_label_extents(emu_engine):
    """An empty label, a single-voxel label, a label that fills the volume, labels >= n_labels."""
    rng = np.random.default_rng(4)
    shape = (3, 20, 32)
    vol = rng.integers(-1024, 600, shape).astype(np.int32)
    lab = np.where(rng.random(shape) < 0.5, 1, 4).astype(np.uint8)
    lab[2, 19, 31] = 3  # single voxel in the last position; label 2 empty
    assert_stats_equal(emu_engine.label_stats(lab, vol, 4), oracle_stats(lab, vol, 4), "mixed")
    full = np.ones(shape, np.uint8)
    assert_stats_equal(emu_engine.label_stats(full, vol, 2), oracle_stats(full, vol, 2), "full")
    one = np.zeros(shape, np.uint8)
    one[1, 7, 5] = 1
    assert_stats_equal(emu_engine.label_stats(one, vol, 3), oracle_stats(one, vol, 3), "single")
    assert_stats_equal(emu_engine.label_stats(full * 9, vol, 3), oracle_stats(full * 9, vol, 3), "all other")


@pytest.mark.parametrize("n_labels", [1, 3, 6, 16])
def test_label_stats_label_groups(emu_engine, n_labels):
    """n_labels 1, 3, 6 and 16: one group, two groups of 3 (R231 / LTRCLobes), four groups of 4."""
    rng = np.random.default_rng(5 + n_labels)
    shape = (2, 17, 48)
    lab = random_labels(rng, shape, n_labels, extra=2)
    vol = rng.normal(-800, 300, shape).astype(np.float32)
    assert_stats_equal(emu_engine.label_stats(lab, vol, n_labels), oracle_stats(lab, vol, n_labels), n_labels)


def test_label_stats_without_histogram(emu_engine):
    rng = np.random.default_rng(6)
    lab = random_labels(rng, (2, 8, 16), 3)
    vol = rng.integers(-1024, 100, lab.shape).astype(np.int16)
    got = emu_engine.label_stats(lab, vol, 3, hist=False)
    want = oracle_stats(lab, vol, 3)
    assert got["hist"] is None
    for f in ("voxels", "hu_min", "index_sum", "bbox"):
        assert np.array_equal(got[f], want[f])


def test_label_stats_invalid_arguments(emu_engine):
    lab = np.zeros((2, 4, 4), np.uint8)
    vol = np.zeros((2, 4, 4), np.int16)
    for k in (0, 17, -1):
        with pytest.raises(nat.LMError, match="lm_label_stats_dev"):
            emu_engine.label_stats(lab, vol, k)
    for dt in (np.uint8, np.uint16):  # dtypes apply widens before the engine: not accepted here
        with pytest.raises(nat.LMError, match="lm_label_stats_dev"):
            emu_engine.label_stats(lab, vol.astype(dt), 2)
    with pytest.raises(nat.LMError):
        emu_engine.label_stats(lab, np.zeros((2, 4, 5), np.int16), 2)
    with pytest.raises(nat.LMError):
        emu_engine.label_stats(lab, vol.astype(np.complex64), 2)
    # a volume beyond the bin width (n * h * w >= 2^31): refused before anything is read
    ld = nat.DeviceView.__new__(nat.DeviceView)
    ld.eng, ld.shape, ld.dtype, ld.ptr, ld.nbytes = emu_engine, (2048, 1024, 1024), np.dtype(np.uint8), 16, 0
    vd = nat.DeviceView.__new__(nat.DeviceView)
    vd.eng, vd.shape, vd.dtype, vd.ptr, vd.nbytes = emu_engine, (2048, 1024, 1024), np.dtype(np.int16), 16, 0
    with pytest.raises(nat.LMError, match="too large"):
        emu_engine.label_stats_dev(ld, vd, 3)
