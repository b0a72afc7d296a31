"""Label agreement metrics (lm_edt_dev, lm_label_agreement_dev) on the g++ emulation of the kernel sources, against numpy oracles
that apply the definitions of include/lungmask_hip.h literally: the float32 min-plus passes of the distance transform, surfaces
and counts straight from the arrays.  Bit for bit on everything but the float64 sums of roots (1e-9 relative: the worst case
n * 2^-53 of a float64 sum of n < 2^23 positive terms in any order)."""
import math

import numpy as np
import pytest

from lungmask_amd import _native as nat

SPACINGS = [None, (2.5, 0.7421875, 0.7421875), (0.625, 0.71, 0.83)]


def oracle_edt(feat: np.ndarray, spacing=None) -> np.ndarray:
    """d2 of lm_edt_dev: the three float32 min-plus passes, broadcast."""
    sp = (1.0, 1.0, 1.0) if spacing is None else spacing
    wz, wy, wx = (np.float32(float(s) * float(s)) for s in sp)
    n, h, w = feat.shape
    ix, iy, iz = np.arange(w), np.arange(h), np.arange(n)
    cx = wx * ((ix[:, None] - ix[None, :]) ** 2).astype(np.float32)  # [x][x']
    cy = wy * ((iy[:, None] - iy[None, :]) ** 2).astype(np.float32)  # [y][y']
    cz = wz * ((iz[:, None] - iz[None, :]) ** 2).astype(np.float32)  # [z][z']
    g = np.empty((n, h, w), np.float32)
    out = np.empty((n, h, w), np.float32)
    for z in range(n):  # (slice by slice: the broadcast of a whole volume would not fit)
        g1 = np.where(feat[z][:, None, :] != 0, cx[None], np.float32(np.inf)).min(axis=2).astype(np.float32)  # [y][x][x']
        g[z] = (g1[None, :, :] + cy[:, :, None]).astype(np.float32).min(axis=1)  # [y][y'][x]
    for z in range(n):
        out[z] = (g + cz[z][:, None, None]).astype(np.float32).min(axis=0)
    return out


def surface(m: np.ndarray) -> np.ndarray:
    """Voxels of m with a 6-neighbour outside m or outside the volume."""
    p = np.pad(m, 1)
    inner = p[1:-1, 1:-1, 1:-1]
    full = p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return inner & ~full


def ranks(count: int, q: float):
    pos = (q / 100.0) * float(count - 1)
    return min(int(math.floor(pos)), count - 1), min(int(math.ceil(pos)), count - 1)


def oracle_agreement(a: np.ndarray, b: np.ndarray, n_labels: int, spacing=None, percentiles=(95,)) -> dict:
    nq = len(percentiles)
    out = {f: np.zeros(n_labels, np.int64) for f in ("voxels_a", "voxels_b", "intersection", "surface_a", "surface_b")}
    out["bbox"] = np.full((n_labels, 6), -1, np.int32)
    out["max_d2_ab"] = np.full(n_labels, -1, np.float32)
    out["max_d2_ba"] = np.full(n_labels, -1, np.float32)
    out["sum_d_ab"] = np.zeros(n_labels)
    out["sum_d_ba"] = np.zeros(n_labels)
    for f in ("order_ab", "order_ba", "order_pooled"):
        out[f] = np.full((n_labels, nq, 2), -1, np.float32)
    out["other_a"], out["other_b"] = int((a >= n_labels).sum()), int((b >= n_labels).sum())
    for k in range(n_labels):
        A, B = (a >= 1, b >= 1) if k == 0 else (a == k, b == k)
        out["voxels_a"][k], out["voxels_b"][k], out["intersection"][k] = A.sum(), B.sum(), (A & B).sum()
        sa, sb = surface(A), surface(B)
        out["surface_a"][k], out["surface_b"][k] = sa.sum(), sb.sum()
        if (A | B).any():
            z, y, x = np.nonzero(A | B)
            out["bbox"][k] = (z.min(), z.max() + 1, y.min(), y.max() + 1, x.min(), x.max() + 1)
        if not sa.any() or not sb.any():
            continue
        dab = np.sort(oracle_edt(sb, spacing)[sa])
        dba = np.sort(oracle_edt(sa, spacing)[sb])
        out["max_d2_ab"][k], out["max_d2_ba"][k] = dab[-1], dba[-1]
        out["sum_d_ab"][k] = np.sqrt(dab.astype(np.float64)).sum()
        out["sum_d_ba"][k] = np.sqrt(dba.astype(np.float64)).sum()
        pooled = np.sort(np.concatenate([dab, dba]))
        for f, lst in (("order_ab", dab), ("order_ba", dba), ("order_pooled", pooled)):
            for i, q in enumerate(percentiles):
                lo, hi = ranks(lst.size, q)
                out[f][k, i] = (lst[lo], lst[hi])
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def assert_agreement_equal(got: dict, want: dict, what=""):
    for f in ("voxels_a", "voxels_b", "intersection", "surface_a", "surface_b", "bbox"):
        assert np.array_equal(np.asarray(got[f]), want[f]), (what, f, got[f], want[f])
    for f in ("max_d2_ab", "max_d2_ba", "order_ab", "order_ba", "order_pooled"):
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f, got[f], want[f])
    for f in ("sum_d_ab", "sum_d_ba"):
        assert np.allclose(got[f], want[f], rtol=1e-9, atol=0), (what, f, got[f], want[f])
    assert (got["other_a"], got["other_b"]) == (want["other_a"], want["other_b"]), what


def blobs(rng, shape, n_labels, extra=0, fill=0.5):
    """Blocky random labels: cells of 3 x 4 x 5 voxels, so that labels have interiors as well as surfaces."""
    n, h, w = shape
    coarse = rng.integers(1, n_labels + extra, ((n + 2) // 3, (h + 3) // 4, (w + 4) // 5)) if n_labels + extra > 1 else \
        np.ones(((n + 2) // 3, (h + 3) // 4, (w + 4) // 5), np.int64)
    coarse = np.where(rng.random(coarse.shape) < fill, coarse, 0)
    return np.repeat(np.repeat(np.repeat(coarse, 3, 0), 4, 1), 5, 2)[:n, :h, :w].astype(np.uint8)


def word_boundary_rows(values=(1, 1, 1, 1)):
    """2 x 3 x 130, rows of three ballot words (the last one partial) for the x pass' search of the nearest set bit: features at
    x = 0 (every other word finds it in a word to its LEFT), x = 129 (in a word to the RIGHT), x = 63 (bit 63 of a word), x = 64
    (the voxel at bit 63 finds it in the next word), an empty row, and all four.  `values`: what is written at x = 0, 63, 64, 129."""
    v0, v63, v64, v129 = values
    vol = np.zeros((2, 3, 130), np.uint8)
    vol[0, 0, 0] = v0
    vol[0, 1, 129] = v129
    vol[0, 2, 63] = v63
    vol[1, 0, 64] = v64
    vol[1, 2, [0, 63, 64, 129]] = values
    return vol


# spacings for word_boundary_rows: unit, and one whose y and z steps cost more than any x distance (129^2 < 10^6), so that what the
# x pass found in a row with a feature is the result
WORD_SPACINGS = [None, (1000.0, 1000.0, 1.0)]


# ---------------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("spacing", SPACINGS)
def test_oracle_matches_scipy(spacing):
    """Five float32 roundings of positive terms: <= 5 * 2^-24 = 3e-7 relative on d2, half of it after the root."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    feat = rng.random((7, 19, 23)) < 0.02
    feat[3, 4, 5] = True
    ref = ndi.distance_transform_edt(~feat, sampling=spacing)
    got = np.sqrt(oracle_edt(feat, spacing).astype(np.float64))
    assert np.allclose(got, ref, rtol=1e-6, atol=0)
    m = rng.random((6, 9, 11)) < 0.6
    assert np.array_equal(surface(m), m ^ ndi.binary_erosion(m, ndi.generate_binary_structure(3, 1)))


# ---------------------------------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", [(1, 9, 13), (5, 1, 17), (4, 7, 1), (3, 11, 70), (6, 13, 31), (2, 5, 600)])
def test_edt_shapes(emu_engine, shape, spacing):
    """n == 1, a single row, a single column, odd sizes, rows of more than one ballot word and longer than a workgroup."""
    rng = np.random.default_rng(sum(shape))
    feat = (rng.random(shape) < 0.03).astype(np.uint8)
    feat.flat[rng.integers(feat.size)] = 200
    got = emu_engine.edt(feat, spacing)
    assert got.dtype == np.float32 and got.shape == shape
    assert np.array_equal(bits(got), bits(oracle_edt(feat, spacing))), (shape, spacing)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_edt_feature_sets(emu_engine, spacing):
    shape = (5, 12, 67)
    one = np.zeros(shape, np.uint8)
    one[4, 0, 66] = 1
    border = np.ones(shape, np.uint8)
    border[1:-1, 1:-1, 1:-1] = 0
    for what, feat in (("one", one), ("all", np.ones(shape, np.uint8)), ("border", border)):
        assert np.array_equal(bits(emu_engine.edt(feat, spacing)), bits(oracle_edt(feat, spacing))), what
    none = emu_engine.edt(np.zeros(shape, np.uint8), spacing)
    assert np.all(np.isposinf(none))
    assert np.all(emu_engine.edt(np.ones(shape, np.uint8), spacing) == 0)


@pytest.mark.parametrize("spacing", WORD_SPACINGS)
def test_edt_word_boundaries(emu_engine, spacing):
    feat = word_boundary_rows()
    got = emu_engine.edt(feat, spacing)
    assert np.array_equal(bits(got), bits(oracle_edt(feat, spacing))), spacing
    if spacing is not None:  # the x pass alone
        x = np.arange(130)
        assert np.array_equal(got[0, 0], (x ** 2).astype(np.float32)) and np.array_equal(got[0, 1], ((129 - x) ** 2).astype(np.float32))
        assert np.array_equal(got[0, 2], ((x - 63) ** 2).astype(np.float32)) and np.array_equal(got[1, 0], ((x - 64) ** 2).astype(np.float32))


def test_edt_long_lines(emu_engine):
    """Lines along y and z longer than one workgroup's threads (tiles a few columns wide)."""
    rng = np.random.default_rng(9)
    for shape in ((1, 530, 3), (530, 2, 5)):
        feat = (rng.random(shape) < 0.004).astype(np.uint8)
        feat[0, 0, 0] = 1
        assert np.array_equal(bits(emu_engine.edt(feat, (0.625, 0.71, 0.83))), bits(oracle_edt(feat, (0.625, 0.71, 0.83)))), shape


def test_edt_dev_in_place_buffer(emu_engine):
    rng = np.random.default_rng(10)
    feat = (rng.random((3, 8, 20)) < 0.05).astype(np.uint8)
    fd = emu_engine.to_device(feat)
    out = emu_engine.empty(feat.shape, np.float32)
    assert emu_engine.edt_dev(fd, (2.0, 1.0, 1.5), out=out) is out
    emu_engine.sync()
    assert np.array_equal(bits(out.download()), bits(oracle_edt(feat, (2.0, 1.0, 1.5))))
    fd.free()
    out.free()


def test_edt_invalid_arguments(emu_engine):
    feat = np.zeros((2, 4, 4), np.uint8)
    for sp in ((1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (np.nan, 1.0, 1.0), (np.inf, 1.0, 1.0)):
        with pytest.raises(nat.LMError, match="lm_edt_dev"):
            emu_engine.edt(feat, sp)
    with pytest.raises(nat.LMError):
        emu_engine.edt(feat, (1.0, 1.0))
    with pytest.raises(nat.LMError):
        emu_engine.edt(np.zeros((4, 4), np.uint8))
    for shape in ((2048, 1024, 1024), (2, 4097, 4)):  # refused before anything is read (the pointers are not valid)
        fd = nat.DeviceView.__new__(nat.DeviceView)
        fd.eng, fd.shape, fd.dtype, fd.ptr, fd.nbytes = emu_engine, shape, np.dtype(np.uint8), 16, 0
        od = nat.DeviceView.__new__(nat.DeviceView)
        od.eng, od.shape, od.dtype, od.ptr, od.nbytes = emu_engine, shape, np.dtype(np.float32), 16, 0
        with pytest.raises(nat.LMError, match="too large"):
            emu_engine.edt_dev(fd, None, out=od)
        with pytest.raises(nat.LMError, match="too large"):
            emu_engine.edt_dev(fd, None)


# ---------------------------------------------------------------------------------------------------------- agreement
@pytest.mark.parametrize("n_labels", [1, 3, 6, 16])
def test_agreement_random_blobs(emu_engine, n_labels):
    rng = np.random.default_rng(20 + n_labels)
    shape = (7, 18, 37) if n_labels < 16 else (9, 22, 48)
    a = blobs(rng, shape, n_labels)
    b = np.roll(a, (1, 2, 3), (0, 1, 2))
    b[rng.random(shape) < 0.05] = 0
    sp = SPACINGS[1]
    qs = (0, 50, 95, 100)
    assert_agreement_equal(emu_engine.label_agreement(a, b, n_labels, sp, qs), oracle_agreement(a, b, n_labels, sp, qs), n_labels)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_agreement_spacings_and_wide_rows(emu_engine, spacing):
    """w a multiple of 16 (the 16-byte path) and not (the scalar tail)."""
    rng = np.random.default_rng(31)
    for shape in ((4, 10, 48), (3, 9, 21)):
        a, b = blobs(rng, shape, 3, extra=1), blobs(rng, shape, 3, extra=1)
        assert_agreement_equal(emu_engine.label_agreement(a, b, 3, spacing, (95,)), oracle_agreement(a, b, 3, spacing, (95,)), (shape, spacing))


def test_agreement_identical_and_disjoint(emu_engine):
    rng = np.random.default_rng(32)
    shape = (6, 14, 32)
    a = blobs(rng, shape, 3)
    got = emu_engine.label_agreement(a, a, 3, None, (0, 50, 95, 100))
    assert_agreement_equal(got, oracle_agreement(a, a, 3, None, (0, 50, 95, 100)), "a == b")
    assert np.array_equal(got["intersection"], got["voxels_a"]) and np.all(got["max_d2_ab"] == 0) and np.all(got["sum_d_ba"] == 0)
    assert np.all(got["order_pooled"] == 0)
    left, right = a.copy(), a.copy()
    left[:, :, 16:] = 0
    right[:, :, :16] = 0
    got = emu_engine.label_agreement(left, right, 3, (1.0, 2.0, 0.5), (95,))
    assert_agreement_equal(got, oracle_agreement(left, right, 3, (1.0, 2.0, 0.5), (95,)), "disjoint")
    assert np.all(got["intersection"] == 0)


def test_agreement_empty_labels_and_other(emu_engine):
    """Label 2 only in a, label 3 in neither, labels >= n_labels in both; percentiles () leaves the order statistics out."""
    rng = np.random.default_rng(33)
    shape = (5, 12, 30)
    a = blobs(rng, shape, 3)  # labels 1, 2
    b = np.where(a == 2, 0, a).astype(np.uint8)
    a[0, 0, :4] = 7
    b[4, 11, 20:] = 9
    for qs in ((95,), ()):
        got = emu_engine.label_agreement(a, b, 4, None, qs)
        assert_agreement_equal(got, oracle_agreement(a, b, 4, None, qs), qs)
    assert got["other_a"] == 4 and got["other_b"] == 10
    assert got["voxels_b"][2] == 0 and got["max_d2_ab"][2] == -1 and got["voxels_a"][3] == 0 and got["bbox"][3].tolist() == [-1] * 6
    empty = np.zeros(shape, np.uint8)
    assert_agreement_equal(emu_engine.label_agreement(empty, empty, 3, None, (95,)), oracle_agreement(empty, empty, 3, None, (95,)), "empty")
    assert_agreement_equal(emu_engine.label_agreement(a, empty, 3, None, (95,)), oracle_agreement(a, empty, 3, None, (95,)), "b empty")


def test_agreement_label_touching_every_face(emu_engine):
    shape = (4, 9, 32)
    a = np.ones(shape, np.uint8)
    b = np.ones(shape, np.uint8)
    b[1:3, 3:6, 10:20] = 2
    got = emu_engine.label_agreement(a, b, 3, SPACINGS[2], (50,))
    assert_agreement_equal(got, oracle_agreement(a, b, 3, SPACINGS[2], (50,)), "full")
    n, h, w = shape
    assert got["surface_a"][1] == n * h * w - (n - 2) * (h - 2) * (w - 2)  # the volume's own border is surface


def test_agreement_closed_forms(emu_engine):
    """Two single voxels: Hausdorff = their distance.  Two boxes [0, s) and [0, s) + t: Hausdorff = |t| (corner to corner)."""
    shape = (8, 16, 32)
    sp = (2.5, 0.75, 0.5)
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[1, 2, 3] = 1
    b[6, 10, 30] = 1
    got = emu_engine.label_agreement(a, b, 2, sp, (0, 100))
    want = np.float32(np.float32(np.float32(0.25) * np.float32(27 ** 2)) + np.float32(np.float32(0.5625) * np.float32(64))) + \
        np.float32(np.float32(6.25) * np.float32(25))
    assert got["max_d2_ab"][1] == want == got["max_d2_ba"][1] == got["order_pooled"][1, 1, 1]
    assert math.isclose(math.sqrt(want), math.sqrt((5 * 2.5) ** 2 + (8 * 0.75) ** 2 + (27 * 0.5) ** 2), rel_tol=1e-6)
    assert got["voxels_a"][1] == 1 and got["surface_a"][1] == 1 and got["bbox"][1].tolist() == [1, 7, 2, 11, 3, 31]
    a[:], b[:] = 0, 0
    a[1:5, 2:8, 3:13] = 1
    b[2:6, 4:10, 6:16] = 1
    got = emu_engine.label_agreement(a, b, 2, None, (100,))
    assert got["max_d2_ab"][1] == 1 + 4 + 9 == got["max_d2_ba"][1] == got["order_ab"][1, 0, 0]
    assert got["intersection"][1] == 3 * 4 * 7
    assert_agreement_equal(got, oracle_agreement(a, b, 2, None, (100,)), "boxes")


def test_agreement_dev_form(emu_engine):
    rng = np.random.default_rng(35)
    a, b = blobs(rng, (4, 9, 32), 3), blobs(rng, (4, 9, 32), 3)
    ad, bd = emu_engine.to_device(a), emu_engine.to_device(b)
    got = emu_engine.label_agreement_dev(ad, bd, 3, (1.0, 1.0, 2.0), (95,))
    assert_agreement_equal(got, emu_engine.label_agreement(a, b, 3, (1.0, 1.0, 2.0), (95,)), "dev")
    ad.free()
    bd.free()


def test_agreement_invalid_arguments(emu_engine):
    a = np.zeros((2, 4, 4), np.uint8)
    for k in (0, 17, -1):
        with pytest.raises(nat.LMError, match="lm_label_agreement_dev"):
            emu_engine.label_agreement(a, a, k)
    for qs in ((-1,), (100.5,), (float("nan"),)):
        with pytest.raises(nat.LMError, match="lm_label_agreement_dev"):
            emu_engine.label_agreement(a, a, 2, None, qs)
    with pytest.raises(nat.LMError):
        emu_engine.label_agreement(a, a, 2, None, tuple(range(9)))
    with pytest.raises(nat.LMError, match="lm_label_agreement_dev"):
        emu_engine.label_agreement(a, a, 2, (1.0, 0.0, 1.0))
    with pytest.raises(nat.LMError):
        emu_engine.label_agreement(a, np.zeros((2, 4, 5), np.uint8), 2)
    ad = nat.DeviceView.__new__(nat.DeviceView)
    ad.eng, ad.shape, ad.dtype, ad.ptr, ad.nbytes = emu_engine, (2048, 1024, 1024), np.dtype(np.uint8), 16, 0
    with pytest.raises(nat.LMError, match="too large"):
        emu_engine.label_agreement_dev(ad, ad, 3)
