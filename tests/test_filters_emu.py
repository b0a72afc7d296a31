"""lm_filter_dev on the emulator engine against a numpy restatement of the header's definitions, bit for bit: the median (a sort with
the stated key) and the separable filter (padded shifts accumulated in float32 in tap order), unmasked and confined by labels.
The oracle and the case builders are shared with tests/test_gpu_filters.py."""
import ctypes as C

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import filters as flt

SHAPES = [(1, 1, 70), (1, 40, 130), (5, 33, 70), (3, 7, 600), (24, 90, 136)]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------
def keep_mask(labels, keep=None):
    table = np.zeros(256, bool)
    table[1:] = True
    if keep is not None:
        table[:] = False
        table[list(keep)] = True
    return table[labels]


def hu_of(vol):
    """(hu int64 saturated to int32, nonfinite): lm_label_stats_dev's HU value."""
    if vol.dtype.kind == "f":
        nan = np.isnan(vol)
        with np.errstate(invalid="ignore"):
            r = np.rint(np.where(nan, 0, vol).astype(np.float64))
        return np.clip(r, INT_MIN, INT_MAX).astype(np.int64), nan
    return np.clip(vol.astype(np.int64), INT_MIN, INT_MAX), np.zeros(vol.shape, bool)


def source_f32(vol, indicator=None):
    if indicator is None:
        return vol.astype(np.float32)
    hu, nan = hu_of(vol)
    lo = INT_MIN if indicator[0] is None else indicator[0]
    hi = INT_MAX if indicator[1] is None else indicator[1]
    return (~nan & (hu >= lo) & (hu <= hi)).astype(np.float32)


def oracle_pass(x, w, axis, clamp):
    w = np.asarray(w, np.float32)
    r = w.size // 2
    if r == 0 and w[0] == np.float32(1):
        return x
    pad = [(0, 0)] * 3
    pad[axis] = (r, r)
    xp = np.pad(x, pad, mode="edge" if clamp else "constant")
    acc = np.zeros(x.shape, np.float32)
    with np.errstate(all="ignore"):
        for k in range(2 * r + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(k, k + x.shape[axis])
            acc = acc + xp[tuple(sl)] * w[k]  # two float32 roundings, no fused multiply-add
    return acc


def oracle_separable(vol, labels, taps, keep=None, fill=None, indicator=None):
    taps = [np.ones(1, np.float32) if t is None else np.asarray(t, np.float32) for t in taps]
    v = source_f32(vol, indicator)
    if labels is None:
        for axis in (2, 1, 0):
            v = oracle_pass(v, taps[axis], axis, True)
        return v
    sel = keep_mask(labels, keep)
    num, den = np.where(sel, v, np.float32(0)), sel.astype(np.float32)
    for axis in (2, 1, 0):
        num, den = oracle_pass(num, taps[axis], axis, False), oracle_pass(den, taps[axis], axis, False)
    with np.errstate(all="ignore"):
        q = num / den
    return np.where(sel, q, v if fill is None else np.float32(fill)).astype(np.float32)


def sort_key(vol):
    """int64 keys: ascending key == ascending value, -0.0 before +0.0 (the bit patterns of float32 made monotone)."""
    if vol.dtype.kind == "f":
        b = vol.view(np.uint32).astype(np.int64)
        return np.where(b >> 31, 0xFFFFFFFF - b, b + 0x80000000)
    return vol.astype(np.int64)


def oracle_median(vol, labels, size, keep=None, fill=None):
    size = [size] * 3 if np.ndim(size) == 0 else list(size)
    half = [s // 2 for s in size]
    masked = labels is not None
    valid = ~np.isnan(vol) if vol.dtype.kind == "f" else np.ones(vol.shape, bool)
    sel = keep_mask(labels, keep) if masked else np.ones(vol.shape, bool)
    valid &= sel
    INVALID = np.int64(1) << 40
    key = np.where(valid, sort_key(vol), INVALID)
    pad = [(h, h) for h in half]
    kp = np.pad(key, pad, mode="constant", constant_values=INVALID) if masked else np.pad(key, pad, mode="edge")
    idx = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)  # which voxel a key came from: the result is one of the inputs
    ip = np.pad(idx, pad, mode="constant") if masked else np.pad(idx, pad, mode="edge")
    n, h, w = vol.shape
    ks, ids = [], []
    for dz in range(size[0]):
        for dy in range(size[1]):
            for dx in range(size[2]):
                ks.append(kp[dz:dz + n, dy:dy + h, dx:dx + w])
                ids.append(ip[dz:dz + n, dy:dy + h, dx:dx + w])
    ks, ids = np.stack(ks), np.stack(ids)
    order = np.argsort(ks, axis=0, kind="stable")
    cnt = (ks != INVALID).sum(axis=0)
    pick = np.take_along_axis(order, (np.maximum(cnt, 1) - 1)[None] // 2, axis=0)
    src = np.take_along_axis(ids, pick, axis=0)[0]
    out = vol.ravel()[src.ravel()].reshape(vol.shape)
    if vol.dtype.kind == "f":
        out = np.where(cnt == 0, np.float32(np.nan), out)
    if masked:
        out = np.where(sel, out, vol if fill is None else np.asarray(fill).astype(vol.dtype))
    return out.astype(vol.dtype)


def assert_same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), f"NaN positions differ at {np.argwhere(gn != wn)[:5].tolist()}"
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        g, w = np.where(gn, 0, got).astype(got.dtype).view(u), np.where(wn, 0, want).astype(want.dtype).view(u)
    else:
        g, w = got, want
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, f"{bad.shape[0]} voxels differ, first {bad[:5].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def volume(shape, dtype, seed):
    """Lung-like HU noise of `dtype`; the float types carry NaN, +-inf, +-0.0 and halves (rint's ties)."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    v = rng.integers(-1100, 400, shape)
    if dtype.kind == "f":
        a = (v / 2).astype(dtype)
        flat = a.ravel()
        m = flat.size
        for val, share in ((np.nan, 25), (np.inf, 60), (-np.inf, 60), (0.0, 30), (-0.0, 30)):
            flat[rng.choice(m, max(1, m // share), replace=False)] = val
        if dtype == np.float64:
            flat[rng.choice(m, max(1, m // 20), replace=False)] = 1.0 / 3.0 - 951.0  # not a float32
        return a
    if dtype == np.int64:
        v = v.astype(np.int64)
        flat = v.ravel()
        flat[rng.choice(flat.size, max(1, flat.size // 40), replace=False)] = (1 << 40) + 12345  # rounds in (float)v, saturates as hu
        flat[rng.choice(flat.size, max(1, flat.size // 40), replace=False)] = -(1 << 33) - 1
        return v
    if dtype == np.int32:
        v = v.astype(np.int32)
        flat = v.ravel()
        flat[rng.choice(flat.size, max(1, flat.size // 40), replace=False)] = INT_MAX
        flat[rng.choice(flat.size, max(1, flat.size // 40), replace=False)] = INT_MIN
        return v
    return v.astype(dtype)


def lung_labels(shape, seed, border=True):
    """Two label blobs (1 and 2, a few voxels of 3) with noise holes; with `border` the selection touches the volume's faces."""
    rng = np.random.default_rng(seed + 1000)
    n, h, w = shape
    lab = np.zeros(shape, np.uint8)
    z0, y0, x0 = (0, 0, 0) if border else (n // 3, h // 3, w // 3)
    z1, y1, x1 = (n, h, w) if border else (max(z0 + 1, 2 * n // 3), max(y0 + 1, 2 * h // 3), max(x0 + 1, 2 * w // 3))
    lab[z0:z1, y0:y1, x0:(x0 + x1) // 2] = 1
    lab[z0:z1, y0:y1, (x0 + x1) // 2:x1] = 2
    lab[rng.random(shape) < 0.25] = 0
    lab[(rng.random(shape) < 0.02) & (lab > 0)] = 3
    if not lab.any():
        lab[0, 0, 0] = 1
    return lab


def random_taps(r, seed, nonneg=False):
    rng = np.random.default_rng(seed + 77)
    t = rng.random(2 * r + 1) if nonneg else rng.normal(size=2 * r + 1)  # asymmetric: a reversed tap order would show
    if nonneg:
        t[r] += 0.5
        t /= t.sum()
    return t.astype(np.float32)


def run_filter(engine, vol, lab, **kw):
    return engine.filter(vol, lab, **kw)


def check_median(engine, vol, lab, size, keep=None, fill=None):
    got = run_filter(engine, vol, lab, kind="median", size=size, keep=keep, fill=fill)
    assert_same_bits(got, oracle_median(vol, lab, size, keep, fill))
    return got


def check_separable(engine, vol, lab, taps, keep=None, fill=None, indicator=None):
    got = run_filter(engine, vol, lab, kind="separable", taps=taps, keep=keep, fill=fill, indicator=indicator)
    assert_same_bits(got, oracle_separable(vol, lab, taps, keep, fill, indicator))
    return got


MEDIAN_SIZES = [3, 5, (1, 3, 3), (5, 1, 3)]
MEDIAN_DTYPES = [np.int16, np.int32, np.float32]
RADII = [(1, 7, 32), (32, 1, 0), (7, 0, 1), (0, 32, 7)]
ALL_DTYPES = [np.int16, np.int32, np.int64, np.float32, np.float64]


def median_cases(shape):
    """(dtype, size, masked): every size with every dtype, masked and unmasked, on the small shapes; on the largest one every size and
    every dtype once in each mode (its tiles differ from the smaller shapes' in number only)."""
    if shape == SHAPES[-1]:
        return [(MEDIAN_DTYPES[(i + m) % 3], s, bool(m)) for m in (0, 1) for i, s in enumerate(MEDIAN_SIZES)]
    return [(d, s, m) for d in MEDIAN_DTYPES for s in MEDIAN_SIZES for m in (False, True)]


def separable_cases(shape):
    """(dtype, radii, masked): mixed radii 0, 1, 7, 32 with the five dtypes rotating through them."""
    k = SHAPES.index(shape)
    return [(ALL_DTYPES[(i + k + m) % 5], r, bool(m)) for m in (0, 1) for i, r in enumerate(RADII)] + \
           [(ALL_DTYPES[(k + 4) % 5], (0, 0, 0), False), (ALL_DTYPES[(k + 2) % 5], (0, 0, 0), True)]


def run_median_cases(engine, shape):
    seed = sum(shape)
    lab = lung_labels(shape, seed)
    for dtype, size, masked in median_cases(shape):
        vol = volume(shape, dtype, seed)
        fill = None if not masked or size == 3 else (-1024 if np.dtype(dtype).kind == "i" else -0.5)
        check_median(engine, vol, lab if masked else None, size, keep=(1, 3) if masked and size == 5 else None, fill=fill)


def run_separable_cases(engine, shape):
    seed = sum(shape) + 5
    lab = lung_labels(shape, seed)
    for i, (dtype, radii, masked) in enumerate(separable_cases(shape)):
        vol = volume(shape, dtype, seed)
        taps = [random_taps(r, seed + 3 * i + a, nonneg=masked) for a, r in enumerate(radii)]
        if radii == (0, 0, 0):
            taps = [None, None, None]  # every pass skipped: the conversion alone
        elif 0 in radii and not masked:
            taps[radii.index(0)] = np.array([0.5], np.float32)  # radius 0 but not the identity: the pass runs
        check_separable(engine, vol, lab if masked else None, taps, keep=(1, 2) if masked and i % 2 else None,
                        fill=-1000.0 if masked and i % 3 == 0 else None)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_median(emu_engine, shape):
    run_median_cases(emu_engine, shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_separable(emu_engine, shape):
    run_separable_cases(emu_engine, shape)


def run_median_special(engine):
    shape = (5, 33, 70)
    vol = volume(shape, np.float32, 3)
    one = np.zeros(shape, np.uint8)
    one[2, 16, 64] = 2  # a one-voxel selection (on a tile border): its own value, or NaN when it is NaN
    for centre in (np.float32(-7.5), np.float32(np.nan)):
        vol[2, 16, 64] = centre
        got = check_median(engine, vol, one, 5, fill=1.0)
        assert (got[one == 0] == 1.0).all() and (np.isnan(got[2, 16, 64]) if np.isnan(centre) else got[2, 16, 64] == centre)
    two = np.zeros(shape, np.uint8)
    two[0, 0, 0:2] = 1  # an even count: the lower median
    iv = volume(shape, np.int16, 4)
    iv[0, 0, 0:2] = (30, -20)
    got = check_median(engine, iv, two, 3)
    assert got[0, 0, 0] == -20 and got[0, 0, 1] == -20 and np.array_equal(got[two == 0], iv[two == 0])
    zeros = np.zeros(shape, np.float32)  # -0.0 sorts before +0.0: windows of both give a definite bit pattern
    zeros[:, ::2] = -0.0
    got = check_median(engine, zeros, None, (1, 3, 3))
    assert np.signbit(got).any() and not np.signbit(got).all()
    allnan = np.full(shape, np.nan, np.float32)
    assert np.isnan(check_median(engine, allnan, None, 3)).all()


def test_median_special(emu_engine):
    run_median_special(emu_engine)


def run_separable_special(engine):
    shape = (5, 33, 70)
    lab = lung_labels(shape, 9)
    g = [flt.gaussian_taps(0.25), flt.gaussian_taps(1.75), flt.gaussian_taps(8.0)]
    assert [t.size // 2 for t in g] == [1, 7, 32]
    for dtype in (np.int16, np.float32, np.float64):
        vol = volume(shape, dtype, 11)
        # Gaussian-derivative taps (orders 1 and 2), unmasked
        check_separable(engine, vol, None, [flt.gaussian_taps(1.0, 2), flt.gaussian_taps(1.75, 1), flt.gaussian_taps(0.25)])
        # the low-attenuation form: indicator with an open bound, fill outside, keep a subset
        got = check_separable(engine, vol, lab, g, keep=(1, 3), fill=0.0, indicator=(None, -951))
        sel = keep_mask(lab, (1, 3))
        assert (got[~sel] == 0).all() and np.nanmin(got[sel]) >= 0
        check_separable(engine, vol, lab, g[::-1], indicator=(-950, -200))  # without fill: the indicator itself outside
        check_separable(engine, vol, None, [None, g[1], None], indicator=(-500, None))
    iv = volume(shape, np.int64, 12)
    check_separable(engine, iv, lab, [g[0], g[0], g[1]], indicator=(INT_MIN, -951))
    check_separable(engine, iv, lab, [None, None, None], fill=5.0, indicator=(0, INT_MAX))  # every pass skipped, masked


def test_separable_special(emu_engine):
    run_separable_special(emu_engine)


def run_box_property(engine):
    """Masked mode may work in the box of the selection: a selection far smaller than the volume equals the whole-volume oracle."""
    shape = SHAPES[-1]
    lab = np.zeros(shape, np.uint8)
    lab[9:13, 40:52, 70:90] = lung_labels((4, 12, 20), 1)
    lab[10, 45, 75] = 1
    vol = volume(shape, np.int16, 21)
    taps = [random_taps(7, 1, True), random_taps(7, 2, True), random_taps(7, 3, True)]
    check_separable(engine, vol, lab, taps)
    check_separable(engine, vol, lab, [random_taps(32, 4, True), None, random_taps(1, 5, True)], fill=0.0, indicator=(None, -700))
    corner = np.zeros(shape, np.uint8)
    corner[-2:, -3:, -5:] = 2  # the box is clipped by the volume
    check_separable(engine, vol.astype(np.float32), corner, taps)
    check_median(engine, vol, lab, 5, fill=7)


def test_masked_box_equals_whole_volume(emu_engine):
    run_box_property(emu_engine)


def test_argument_errors(emu_engine):
    vol = volume((3, 8, 9), np.int16, 2)
    lab = lung_labels((3, 8, 9), 2)
    with pytest.raises(ValueError, match="size"):
        emu_engine.filter(vol, None, kind="median", size=4)
    with pytest.raises(ValueError, match="size"):
        emu_engine.filter(vol, None, kind="median", size=(3, 3))
    with pytest.raises(ValueError, match="radius at most 32"):
        emu_engine.filter(vol, None, kind="separable", taps=[np.ones(67, np.float32), None, None])
    with pytest.raises(ValueError, match="taps >= 0"):
        emu_engine.filter(vol, lab, kind="separable", taps=[np.array([0.5, 1.0, -0.5], np.float32), None, None])
    with pytest.raises(ValueError, match="centre tap"):
        emu_engine.filter(vol, lab, kind="separable", taps=[np.array([0.5, 0.0, 0.5], np.float32), None, None])
    with pytest.raises(ValueError, match="cast"):
        emu_engine.filter(vol.astype(np.float64), None, kind="median")
    with pytest.raises(ValueError, match="fill needs labels"):
        emu_engine.filter(vol, None, kind="median", fill=0)
    with pytest.raises(nat.NoKeptVoxel):
        emu_engine.filter(vol, np.zeros_like(lab), kind="median")
    with pytest.raises(nat.NoKeptVoxel):
        emu_engine.filter(vol, lab, kind="separable", taps=[None, None, None], keep=(9,))
    # the C entry point refuses the same things itself, before anything is read
    lib, vd, ld = emu_engine.L.lib, emu_engine.to_device(vol), emu_engine.to_device(lab)
    out = emu_engine.empty(vol.shape, np.int16)
    outf = emu_engine.empty(vol.shape, np.float32)

    def call(p, dtype=0, lab_ptr=None, o=out, shape=vol.shape):
        rc = lib.lm_filter_dev(emu_engine.h, vd.ptr, dtype, lab_ptr, shape[0], shape[1], shape[2], C.byref(p), o.ptr)
        return rc, lib.lm_last_error().decode()

    p = nat.Engine._filter_params("median", size=3)
    p.size[1] = 2
    assert call(p)[0] == -1 and "size[1]" in call(p)[1]
    p = nat.Engine._filter_params("median", size=3)
    assert call(p, dtype=3)[0] == -1 and "LM_F32" in call(p, dtype=3)[1]  # a float64 median
    p.flags = nat.FILTER_MASKED
    assert call(p)[0] == -1 and "needs labels" in call(p)[1]  # masked without labels
    p = nat.Engine._filter_params("separable", taps=[None, None, None])
    p.radius[2] = 33
    assert call(p, o=outf)[0] == -1 and "radius[2]" in call(p, o=outf)[1]
    p = nat.Engine._filter_params("separable", taps=[np.ones(3, np.float32), None, None])
    p.taps[0][0] = -1.0
    p.flags = nat.FILTER_MASKED
    assert call(p, lab_ptr=ld.ptr, o=outf)[0] == -1 and "taps >= 0" in call(p, lab_ptr=ld.ptr, o=outf)[1]
    p = nat.Engine._filter_params("median", size=3)
    assert call(p, shape=(1, 1, 4097))[0] == -1 and "too large" in call(p, shape=(1, 1, 4097))[1]
    assert call(p, o=vd)[0] == -1  # in place
    p.kind = 7
    assert call(p)[0] == -1 and "unknown kind" in call(p)[1]
    for d in (vd, ld, out, outf):
        d.free()
