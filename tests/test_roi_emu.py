"""lm_roi_plan_dev / lm_roi_dev on the g++ emulation of the kernel sources, bit for bit against a numpy oracle that applies the
definitions of include/lungmask_hip.h directly (box, grid, trilinear float64 intensity, nearest-neighbour labels, inside test, mask,
window, output rounding), and -- independently of that oracle -- against scipy.ndimage.map_coordinates."""
import math
import warnings

import numpy as np
import pytest

from lungmask_amd import _native as nat

DTYPES = [np.int16, np.int32, np.int64, np.float32, np.float64]


# ---------------------------------------------------------------------------------------------------------------- the oracle
def keep_table(keep):
    t = np.zeros(256, bool)
    if keep is None:
        t[1:] = True
    else:
        t[list(keep)] = True
    return t


def oracle_box(lab, spacing, margin_mm, keep):
    """Step 1: bbox_3D (margin 0) of keep[lab], grown by ceil(margin_mm / s_i) (margin_mm voxels without a spacing), clipped."""
    kept = keep_table(keep)[lab]
    if not kept.any():
        return None
    box = []
    for ax in range(3):
        idx = np.nonzero(kept.any(axis=tuple(a for a in range(3) if a != ax)))[0]
        m = math.ceil(margin_mm / spacing[ax]) if spacing is not None else math.ceil(margin_mm)
        box += [max(int(idx[0]) - m, 0), min(int(idx[-1]) + 1 + m, lab.shape[ax])]
    return box


def oracle_taps(n_out, step, e):
    c = np.minimum(np.arange(n_out, dtype=np.float64) * step, float(e - 1))
    i0 = np.floor(c).astype(np.int64)
    f = c - i0
    i1 = np.minimum(i0 + 1, e - 1)
    j = np.minimum(np.floor(c + 0.5).astype(np.int64), e - 1)
    return c, i0, i1, f, j


def lerp(a, b, f):
    return a * (1.0 - f) + b * f


def oracle_roi(vol, lab, spacing=None, spacing_out=None, margin_mm=5.0, keep=None, dilate_mm=0.0, mask_outside=True, fill=-1024,
               window=None, dtype=np.float32, d2_of=None):
    """-> (image, labels, bbox, out_dims, step).  d2_of(features u8 box, spacing) -> lm_edt_dev's float32 squared distances."""
    box = oracle_box(lab, spacing, margin_mm, keep)
    if box is None:
        raise ValueError("no kept voxel")
    ext = [box[1] - box[0], box[3] - box[2], box[5] - box[4]]
    if spacing_out is None:
        step = [1.0, 1.0, 1.0]
    else:
        t = [float(spacing_out)] * 3 if np.ndim(spacing_out) == 0 else [float(v) for v in spacing_out]
        step = [t[i] / float(spacing[i]) for i in range(3)]
    dims = [int(math.floor((ext[i] - 1) / step[i])) + 1 for i in range(3)]
    (_, z0, z1, fz, zj), (_, y0, y1, fy, yj), (_, x0, x1, fx, xj) = (oracle_taps(dims[i], step[i], ext[i]) for i in range(3))
    sl = (slice(box[0], box[1]), slice(box[2], box[3]), slice(box[4], box[5]))
    src = vol[sl].astype(np.float64)
    lbox = lab[sl]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        v = lerp(src[:, :, x0], src[:, :, x1], fx[None, None, :])  # x
        v = lerp(v[:, y0, :], v[:, y1, :], fy[None, :, None])      # then y
        v = lerp(v[z0], v[z1], fz[:, None, None])                  # then z
        labels = lbox[np.ix_(zj, yj, xj)]
        if mask_outside:
            if dilate_mm > 0:
                d2 = d2_of(keep_table(keep)[lbox].astype(np.uint8), spacing)
                inside = d2[np.ix_(zj, yj, xj)] <= np.float32(dilate_mm * dilate_mm)
            else:
                inside = keep_table(keep)[labels]
            v = np.where(inside, v, float(fill))
        if window is not None:
            lo, hi = float(window[0]), float(window[1])
            v = np.where(v < lo, lo, np.where(v > hi, hi, v))
            v = (v - lo) / (hi - lo)
        dt = np.dtype(dtype)
        if dt == np.float32:
            img = v.astype(np.float32)
        elif dt == np.float16:
            img = v.astype(np.float32).astype(np.float16)
        else:
            img = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return img, labels, box, dims, step


def same_bits(a, b):
    """Equal dtype, shape and bit patterns; a NaN equals a NaN (IEEE 754 leaves the sign and payload of a generated NaN open, and
    the formulas do not define them)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint8 if a.itemsize == 1 else f"u{a.itemsize}"
    if a.dtype.kind != "f":
        return np.array_equal(a.view(u), b.view(u))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


def check(eng, vol, lab, what="", **kw):
    want = oracle_roi(vol, lab, d2_of=lambda f, sp: eng.edt(f, sp), **kw)
    img, out_lab, info = eng.roi(vol, lab, **kw)
    assert info["bbox"] == want[2] and info["out_dims"] == want[3] and info["step"] == want[4], (what, info, want[2:])
    assert tuple(img.shape) == tuple(want[3])
    assert np.array_equal(out_lab, want[1]), what
    assert same_bits(img, want[0]), (what, int(((img != want[0]) & ~(np.isnan(img) & np.isnan(want[0]))).sum()), "of", img.size, "differ")
    return img, out_lab, info


def blobs(shape, seed, n_labels=2):
    """A label volume with a few ellipsoids (labels 1 .. n_labels) away from some of the borders, touching others."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    lab = np.zeros(shape, np.uint8)
    for k in range(1, n_labels + 1):
        c = [rng.uniform(0.25, 0.75) * s for s in shape]
        r = [max(1.5, rng.uniform(0.15, 0.3) * s) for s in shape]
        lab[((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0] = k
    return lab


def volume(shape, dtype, seed, special=False):
    rng = np.random.default_rng(seed)
    vol = rng.integers(-1500, 3500, shape).astype(dtype)
    if np.dtype(dtype).kind == "f":
        vol = (vol + rng.uniform(-0.5, 0.5, shape)).astype(dtype)
        if special:
            vol.flat[::37] = np.nan
            vol.flat[5::41] = np.inf
            vol.flat[7::43] = -np.inf
    return vol


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("dtype", DTYPES)
def test_roi_every_input_dtype(emu_engine, dtype):
    shape = (11, 37, 45)  # odd shapes: scalar stores, partial tiles
    vol, lab = volume(shape, dtype, 1), blobs(shape, 2)
    check(emu_engine, vol, lab, "crop", spacing=(2.5, 0.7, 0.8), margin_mm=2.0)  # step 1: the crop path
    check(emu_engine, vol, lab, "iso", spacing=(2.5, 0.7, 0.8), spacing_out=1.0, margin_mm=3.0)  # z up-, y and x down-sampled
    check(emu_engine, vol, lab, "aniso", spacing=(2.5, 0.7, 0.8), spacing_out=(1.3, 1.9, 0.5), margin_mm=1.0)
    check(emu_engine, vol, lab, "f16", spacing=(2.5, 0.7, 0.8), spacing_out=1.0, dtype=np.float16)


def test_crop_returns_the_source_values(emu_engine):
    vol, lab = volume((9, 30, 33), np.int16, 3), blobs((9, 30, 33), 4)
    img, out_lab, info = check(emu_engine, vol, lab, "crop", margin_mm=2, mask_outside=False)  # no spacing: the margin in voxels
    b = info["bbox"]
    assert np.array_equal(img, vol[b[0]:b[1], b[2]:b[3], b[4]:b[5]].astype(np.float32))
    assert np.array_equal(out_lab, lab[b[0]:b[1], b[2]:b[3], b[4]:b[5]])
    assert info["step"] == [1.0, 1.0, 1.0] and info["spacing_mm"] is None


@pytest.mark.parametrize("out_dtype", [np.float32, np.float16, np.int16])
def test_roi_output_dtypes_vector_and_scalar_stores(emu_engine, out_dtype):
    for shape, spo in (((8, 40, 64), None), ((7, 33, 50), 1.1), ((6, 36, 44), (2.0, 0.9, 1.0))):
        vol, lab = volume(shape, np.int32, 5), blobs(shape, 6)
        check(emu_engine, vol, lab, (shape, spo), spacing=(2.0, 0.9, 1.0), spacing_out=spo, margin_mm=100.0, dtype=out_dtype, fill=-2000)
    # int16 saturates
    vol = volume((5, 20, 24), np.int64, 7) * 40
    check(emu_engine, vol, blobs((5, 20, 24), 8), "sat", spacing=(1, 1, 1), spacing_out=0.7, dtype=np.int16, fill=-10 ** 6)


def test_float16_equals_float32_cast(emu_engine):
    vol, lab = volume((7, 31, 42), np.float32, 9), blobs((7, 31, 42), 10)
    kw = dict(spacing=(2.0, 0.8, 0.8), spacing_out=1.0, window=(-1000.0, 400.0))
    f32 = emu_engine.roi(vol, lab, dtype=np.float32, **kw)[0]
    f16 = emu_engine.roi(vol, lab, dtype=np.float16, **kw)[0]
    assert same_bits(f16, f32.astype(np.float16))


def test_int16_output_refused_for_float_volumes_and_windows(emu_engine):
    lab = blobs((5, 20, 24), 8)
    for vol, kw in ((volume((5, 20, 24), np.float32, 1), {}), (volume((5, 20, 24), np.float64, 1), {}),
                    (volume((5, 20, 24), np.int16, 1), {"window": (-1000, 400)})):
        with pytest.raises(ValueError, match="int16"):
            emu_engine.roi(vol, lab, dtype=np.int16, **kw)
    # the C entry point refuses them as well
    import ctypes as C
    p = nat.RoiParams()
    p.bbox[:] = [0, 5, 0, 20, 0, 24]
    p.out_dims[:] = [5, 20, 24]
    p.step[:] = [1.0, 1.0, 1.0]
    p.spacing[:] = [1.0, 1.0, 1.0]
    p.out_dtype = 0  # LM_I16
    vd, ld = emu_engine.to_device(volume((5, 20, 24), np.float32, 1)), emu_engine.to_device(lab)
    img, ol = emu_engine.empty((5, 20, 24), np.int16), emu_engine.empty((5, 20, 24), np.uint8)
    lib = emu_engine.L.lib
    assert lib.lm_roi_dev(emu_engine.h, vd.ptr, 2, ld.ptr, 5, 20, 24, C.byref(p), img.ptr, ol.ptr) < 0
    assert b"LM_I16" in lib.lm_last_error()
    p.out_dtype = 2
    p.out_dims[:] = [5, 20, 25]  # not the header's N_i
    assert lib.lm_roi_dev(emu_engine.h, vd.ptr, 2, ld.ptr, 5, 20, 24, C.byref(p), img.ptr, ol.ptr) < 0
    assert b"out_dims" in lib.lm_last_error()
    p.out_dims[:] = [5, 20, 24]
    p.bbox[:] = [0, 6, 0, 20, 0, 24]  # beyond the volume
    assert lib.lm_roi_dev(emu_engine.h, vd.ptr, 2, ld.ptr, 5, 20, 24, C.byref(p), img.ptr, ol.ptr) < 0
    for d in (vd, ld, img, ol):
        d.free()


def test_margins_clipped_at_the_volume_edge(emu_engine):
    shape = (6, 25, 30)
    lab = np.zeros(shape, np.uint8)
    lab[0:3, 2:20, 25:30] = 1  # touches z = 0 and the last column
    vol = volume(shape, np.int16, 11)
    _, _, info = check(emu_engine, vol, lab, "edge", spacing=(3.0, 1.0, 1.0), spacing_out=(1.5, 1.0, 2.0), margin_mm=4.0)
    assert info["bbox"] == [0, 5, 0, 24, 21, 30]
    _, _, info = check(emu_engine, vol, lab, "all", spacing=(3.0, 1.0, 1.0), margin_mm=1000.0)
    assert info["bbox"] == [0, 6, 0, 25, 0, 30]


def test_keep_subsets(emu_engine):
    shape = (9, 33, 40)
    vol, lab = volume(shape, np.int16, 12), blobs(shape, 13, n_labels=4)
    lab[0, 0, 0] = 200  # a stray label far from the rest
    boxes = []
    for keep in (None, [1], [2, 4], [200], [3, 200]):
        _, out_lab, info = check(emu_engine, vol, lab, keep, spacing=(2.0, 1.0, 1.0), spacing_out=(1.0, 1.5, 0.75), margin_mm=2.0, keep=keep)
        boxes.append(info["bbox"])
    assert boxes[0][:1] == [0] and boxes[1] != boxes[2] and boxes[3] == [0, 2, 0, 3, 0, 3]
    with pytest.raises(ValueError, match="1..255"):
        emu_engine.roi(vol, lab, keep=[0])


@pytest.mark.parametrize("dilate_mm", [1.0, 2.5, 4.0])
def test_dilation_against_the_distance_transform(emu_engine, dilate_mm):
    from scipy import ndimage

    shape = (10, 34, 38)
    sp = (2.5, 0.7, 0.9)
    vol, lab = volume(shape, np.int16, 14), blobs(shape, 15, n_labels=3)
    for keep, spo in ((None, None), ([2], 1.0), ([1, 3], (1.25, 1.4, 0.45))):
        img, out_lab, info = check(emu_engine, vol, lab, (keep, spo), spacing=sp, spacing_out=spo, margin_mm=4.0, keep=keep,
                                   dilate_mm=dilate_mm, fill=-5000)
        # the float64 transform of scipy itself: the same inside set, except where a distance sits on the threshold
        b = info["bbox"]
        kept = keep_table(keep)[lab[b[0]:b[1], b[2]:b[3], b[4]:b[5]]]
        dist = ndimage.distance_transform_edt(~kept, sampling=sp)
        taps = [oracle_taps(info["out_dims"][i], info["step"][i], kept.shape[i])[4] for i in range(3)]
        d = dist[np.ix_(*taps)]
        clear = np.abs(d - dilate_mm) > 1e-5 * dilate_mm
        inside, outside = clear & (d <= dilate_mm), clear & (d > dilate_mm)
        assert inside.sum() > kept[np.ix_(*taps)].sum() > 0 and outside.sum() > 0  # the dilation adds voxels, and leaves some out
        assert np.all(img[outside] == -5000) and np.all(img[inside] >= -1500)  # (every source value is >= -1500: not the fill)
    with pytest.raises(ValueError, match="dilate_mm"):
        emu_engine.roi(vol, lab, spacing=sp, margin_mm=1.0, dilate_mm=2.0)


def test_mask_outside_off_and_window(emu_engine):
    shape = (8, 29, 35)
    vol, lab = volume(shape, np.float64, 16), blobs(shape, 17)
    for mask_outside in (True, False):
        for window in (None, (-1000.0, 400.0), (0.0, 1.0)):
            img, _, _ = check(emu_engine, vol, lab, (mask_outside, window), spacing=(2.0, 0.9, 0.8), spacing_out=1.0, margin_mm=3.0,
                              mask_outside=mask_outside, window=window, fill=-1024)
            if window is not None:
                assert img.min() >= 0.0 and img.max() <= 1.0
    with pytest.raises(ValueError, match="window"):
        emu_engine.roi(vol, lab, window=(5.0, 5.0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_and_inf_follow_the_formulas(emu_engine, dtype):
    shape = (7, 27, 31)
    vol, lab = volume(shape, dtype, 18, special=True), blobs(shape, 19)
    for kw in (dict(), dict(spacing_out=0.9), dict(spacing_out=(1.0, 1.7, 0.6), window=(-1000.0, 400.0)), dict(mask_outside=False, dtype=np.float16)):
        img, _, _ = check(emu_engine, vol, lab, kw, spacing=(2.0, 0.9, 0.8), margin_mm=2.0, **kw)
    assert np.isnan(img).any()


def test_empty_mask(emu_engine):
    import ctypes as C

    vol = volume((4, 10, 12), np.int16, 20)
    lab = np.zeros((4, 10, 12), np.uint8)
    with pytest.raises(ValueError, match="no voxel"):
        emu_engine.roi(vol, lab)
    lab[1, 2, 3] = 2
    with pytest.raises(ValueError, match="no voxel"):
        emu_engine.roi(vol, lab, keep=[1])
    ld = emu_engine.to_device(lab)
    bb = (C.c_int32 * 6)()
    lib = emu_engine.L.lib
    assert lib.lm_roi_plan_dev(emu_engine.h, ld.ptr, 4, 10, 12, nat.Engine._keep_table([1]), bb) < 0  # non-zero return code, message
    assert b"no kept voxel" in lib.lm_last_error() and list(bb) == [-1] * 6
    assert lib.lm_roi_plan_dev(emu_engine.h, ld.ptr, 4, 10, 12, nat.Engine._keep_table([2]), bb) == 0 and list(bb) == [1, 2, 2, 3, 3, 4]
    ld.free()


def test_limits_refused_before_anything_is_read(emu_engine):
    import ctypes as C

    lib = emu_engine.L.lib
    p = nat.RoiParams()
    bb = (C.c_int32 * 6)()
    for n, h, w in ((4097, 2, 2), (2, 4097, 2), (2, 2, 4097), (2048, 1024, 1024)):
        assert lib.lm_roi_plan_dev(emu_engine.h, 8, n, h, w, nat.Engine._keep_table(None), bb) < 0  # (the pointer is never used)
        assert b"too large" in lib.lm_last_error()
        assert lib.lm_roi_dev(emu_engine.h, 8, 0, 8, n, h, w, C.byref(p), 8, 8) < 0
        assert b"too large" in lib.lm_last_error()


def test_against_scipy_map_coordinates(emu_engine):
    """Independent of the oracle above: every voxel of a finite int16 volume, mask_outside=False, no window, float32 output, against
    scipy's own linear interpolation.  Both sides form a convex combination in float64 and differ by a few float64 ulps -- far below
    half a float32 ulp -- so the one final rounding can flip at most one float32 ulp: that is the bound.  The count of differing
    voxels is printed, not bounded."""
    from scipy import ndimage

    shape = (23, 40, 37)
    sp = (2.5, 0.7, 0.7)
    vol = np.random.default_rng(21).integers(-1500, 3500, shape).astype(np.int16)
    lab = np.zeros(shape, np.uint8)
    lab[3:20, 5:35, 4:33] = 1
    img, _, info = emu_engine.roi(vol, lab, spacing=sp, spacing_out=1.0, margin_mm=1000.0, mask_outside=False, dtype=np.float32)
    b = info["bbox"]
    box = vol[b[0]:b[1], b[2]:b[3], b[4]:b[5]].astype(np.float64)
    coords = np.meshgrid(*[oracle_taps(info["out_dims"][i], info["step"][i], box.shape[i])[0] for i in range(3)], indexing="ij")
    want = ndimage.map_coordinates(box, coords, order=1, mode="nearest").astype(np.float32)
    assert img.shape == want.shape and img.size > 10 ** 4
    differ = int((img != want).sum())
    print(f"scipy map_coordinates: {differ} of {img.size} float32 values differ")
    ulp = np.spacing(np.maximum(np.abs(img), np.abs(want)))
    assert np.all(np.abs(img.astype(np.float64) - want.astype(np.float64)) <= ulp)
