"""lm_spline_prefilter_dev / lm_resample_dev on the g++ emulation of the kernel sources, bit for bit against a numpy restatement of
the definition in include/lungmask_hip.h (coordinate, domain test, nearest, trilinear, cubic B-spline prefilter and sample, the
label-linear argmax, output rounding), and -- independently of that restatement -- against scipy.ndimage."""
import ctypes as C
import warnings

import numpy as np
import pytest

from lungmask_amd import _native as nat
from tests.test_roi_emu import DTYPES, blobs, same_bits, volume

# the smallest shapes at which each part can go wrong: one voxel; axes of extent 1 skipped and mirror periods 2 and 4; odd sizes;
# either side of the 37-term start sum; lines crossing and not filling the 64-wide x-pass tiles (64 + 2 and 2 * 64 + 2)
SHAPES = [(1, 1, 1), (1, 2, 3), (5, 7, 9), (3, 37, 38), (2, 66, 130)]
Z = np.sqrt(3.0) - 2.0


# ---------------------------------------------------------------------------------------------------------------- the restatement
def coordinates(A, b, dims):
    """Steps 1 and 2: (c [3] float64 arrays, inside, j [3] int arrays) without the extents applied to `inside` yet."""
    A, b = np.asarray(A, np.float64).reshape(3, 3), np.asarray(b, np.float64).reshape(3)
    o = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij")
    return [((A[i, 0] * o[0] + A[i, 1] * o[1]) + A[i, 2] * o[2]) + b[i] for i in range(3)]


def domain(c, ext):
    inside = np.ones(c[0].shape, bool)
    j = []
    for i in range(3):
        t = np.floor(c[i] + 0.5)
        ok = (t >= 0.0) & (t < float(ext[i]))
        inside &= ok
        j.append(np.where(ok, t, 0.0).astype(np.int64))
    return inside, j


def clamp(c, e):
    return np.minimum(np.maximum(c, 0.0), float(e - 1))


def taps2(c, e):
    c = clamp(c, e)
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, e - 1), c - i0


def mirror(k, e):
    k = np.asarray(k, np.int64)
    if e == 1:
        return np.zeros_like(k)
    P = 2 * e - 2
    m = np.mod(k, P)
    return np.where(m >= e, P - m, m)


def lerp(a, b, f):
    return a * (1.0 - f) + b * f


def prefilter_axis(v, axis):
    e = v.shape[axis]
    if e == 1:
        return v
    s = np.moveaxis(v, axis, 0)
    cp = np.empty_like(s)
    acc, zk = np.zeros(s.shape[1:]), 1.0
    for k in range(37):
        acc = acc + zk * s[int(mirror(k, e))]
        zk = zk * Z
    cp[0] = acc
    for i in range(1, e):
        cp[i] = s[i] + Z * cp[i - 1]
    c = np.empty_like(s)
    c[e - 1] = (Z / (Z * Z - 1.0)) * (cp[e - 1] + Z * cp[e - 2])
    for i in range(e - 2, -1, -1):
        c[i] = Z * (c[i + 1] - cp[i])
    return np.moveaxis(6.0 * c, 0, axis)


def prefilter(vol):
    """Step 5, prefilter: x, then y, then z, on the volume converted to double."""
    v = vol.astype(np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for axis in (2, 1, 0):
            v = prefilter_axis(v, axis)
    return v


def taps4(c, e):
    c = clamp(c, e)
    i0 = np.floor(c).astype(np.int64)
    f = c - i0
    g = 1.0 - f
    idx = [mirror(i0 - 1 + k, e) for k in range(4)]
    w = [((g * g) * g) / 6.0, 2.0 / 3.0 - ((f * f) * (2.0 - f)) / 2.0, 2.0 / 3.0 - ((g * g) * (1.0 + f)) / 2.0, ((f * f) * f) / 6.0]
    return idx, w


def cast_out(v, dtype):
    dt = np.dtype(dtype)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if dt == np.float32:
            return v.astype(np.float32)
        if dt == np.float16:
            return v.astype(np.float32).astype(np.float16)
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def nearest_fill(dtype, fill):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return dt.type(fill)
    if dt == np.uint8:
        return np.uint8(int(fill))
    info = np.iinfo(dt)
    return dt.type(min(max(int(np.rint(fill)), info.min), info.max))


def restate(src, A, b, dims, mode, fill=-1024, dtype=None, raw=False):
    """The definition applied directly -> the output array (`raw`: the float64 values of linear / cubic before the final cast)."""
    ext = src.shape
    c = coordinates(A, b, dims)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        inside, j = domain(c, ext)
        if mode == "nearest":
            return np.where(inside, src[j[0], j[1], j[2]], nearest_fill(src.dtype, fill)).astype(src.dtype)
        if mode == "linear":
            (z0, z1, fz), (y0, y1, fy), (x0, x1, fx) = (taps2(c[i], ext[i]) for i in range(3))
            s = src.astype(np.float64)
            v00 = lerp(s[z0, y0, x0], s[z0, y0, x1], fx)
            v01 = lerp(s[z0, y1, x0], s[z0, y1, x1], fx)
            v10 = lerp(s[z1, y0, x0], s[z1, y0, x1], fx)
            v11 = lerp(s[z1, y1, x0], s[z1, y1, x1], fx)
            v = lerp(lerp(v00, v01, fy), lerp(v10, v11, fy), fz)
        elif mode == "cubic":
            coef = prefilter(src)
            (iz, wz), (iy, wy), (ix, wx) = (taps4(c[i], ext[i]) for i in range(3))
            v = np.zeros(c[0].shape)
            for a in range(4):
                vy = np.zeros(c[0].shape)
                for bb in range(4):
                    vx = np.zeros(c[0].shape)
                    for k in range(4):
                        vx = vx + wx[k] * coef[iz[a], iy[bb], ix[k]]
                    vy = vy + wy[bb] * vx
                v = v + wz[a] * vy
        else:  # label_linear
            (z0, z1, fz), (y0, y1, fy), (x0, x1, fx) = (taps2(c[i], ext[i]) for i in range(3))
            lab, wgt = [], []
            for zi, wz in ((z0, 1.0 - fz), (z1, fz)):
                for yi, wy in ((y0, 1.0 - fy), (y1, fy)):
                    for xi, wx in ((x0, 1.0 - fx), (x1, fx)):
                        lab.append(src[zi, yi, xi].astype(np.int64))
                        wgt.append((wz * wy) * wx)
            best, best_sum = np.full(c[0].shape, 256, np.int64), np.full(c[0].shape, -1.0)
            for k in range(8):
                s = np.zeros(c[0].shape)
                for q in range(8):
                    s = np.where(lab[q] == lab[k], s + wgt[q], s)
                better = (s > best_sum) | ((s == best_sum) & (lab[k] < best))
                best, best_sum = np.where(better, lab[k], best), np.where(better, s, best_sum)
            return np.where(inside, best, int(fill)).astype(np.uint8)
        v = np.where(inside, v, float(fill))
    return v if raw else cast_out(v, np.float32 if dtype is None else dtype)


# ---------------------------------------------------------------------------------------------------------------- the maps
def maps_for(shape):
    """name -> (A, b, out_dims): every map with output dims that differ from the source's."""
    e = np.asarray(shape)
    I = np.eye(3)
    a = np.radians(17.0)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])  # about the z axis of the array
    p = np.array([0.3 * (e[0] - 1), 0.2 * (e[1] - 1), 0.7 * (e[2] - 1)])  # an off-centre point
    perm = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # z <- x, y <- flipped z, x <- y: determinant -1
    return {
        "identity": (I, np.zeros(3), tuple(e + (1, 2, 3))),
        "shift": (I, np.array([1.0, -2.0, 3.0]), tuple(e + (2, 1, 1))),
        "half": (I, np.array([0.5, -0.5, 0.5]), tuple(e + (1, 1, 2))),
        "scale": (np.diag([0.5, 1.7, 0.83]), np.array([0.1, -0.3, 0.2]), (2 * e[0] + 1, e[1] // 2 + 2, e[2] + 3)),
        "permute": (perm, np.array([0.0, e[1] - 1.0, 0.0]), (e[1] + 1, e[2] + 1, e[0] + 1)),
        "rotate": (R, p - R @ p, tuple(e + (1, 3, 2))),
        "outside": (I, np.array([e[0] + 5.0, 0.0, 0.0]), tuple(e + (1, 0, 2))),
    }


def labels_for(shape, seed):
    lab = blobs(shape, seed, n_labels=3) if min(shape) > 2 else np.zeros(shape, np.uint8)
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 5, shape).astype(np.uint8)  # neighbouring voxels with different labels everywhere
    return np.where(rng.random(shape) < 0.5, lab, noise).astype(np.uint8)


def check(eng, src, A, b, dims, mode, what="", **kw):
    want = restate(src, A, b, dims, mode, **kw)
    got = eng.resample(src, A, b, dims, mode, **kw)
    assert same_bits(got, want), (what, mode, src.dtype, src.shape, dims, int(((got != want) & ~((got != got) & (want != want))).sum()), "of", got.size, "differ")
    return got


def check_shape(eng, shape, seed=0):
    """Every mode, input dtype and map on one source shape."""
    for name, (A, b, dims) in maps_for(shape).items():
        for dtype in DTYPES:
            vol = volume(shape, dtype, seed + 1, special=True)
            check(eng, vol, A, b, dims, "linear", name, fill=-1000.5)
            check(eng, vol, A, b, dims, "nearest", name, fill=-1000.5)
        finite = volume(shape, np.int16, seed + 2)
        check(eng, finite, A, b, dims, "cubic", name)
        check(eng, finite.astype(np.float32) + 0.25, A, b, dims, "cubic", name, dtype=np.float16)
        lab = labels_for(shape, seed + 3)
        check(eng, lab, A, b, dims, "nearest", name, fill=7)
        check(eng, lab, A, b, dims, "label_linear", name, fill=7)


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("shape", SHAPES)
def test_every_mode_dtype_and_map(emu_engine, shape):
    check_shape(emu_engine, shape)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cubic_every_input_dtype(emu_engine, dtype):
    shape = (5, 7, 9)
    vol = volume(shape, dtype, 4)
    for name in ("scale", "rotate"):
        A, b, dims = maps_for(shape)[name]
        check(emu_engine, vol, A, b, dims, "cubic", name)
    if np.dtype(dtype).kind == "f":  # NaN and inf run through the recursion as the formulas say
        A, b, dims = maps_for(shape)["scale"]
        out = check(emu_engine, volume(shape, dtype, 5, special=True), A, b, dims, "cubic", "special")
        assert np.isnan(out).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_prefilter_alone_equals_the_restatement(emu_engine, shape):
    for dtype in (np.int16, np.float64):
        vol = volume(shape, dtype, 6)
        assert same_bits(emu_engine.spline_prefilter(vol), prefilter(vol)), (shape, dtype)


@pytest.mark.parametrize("shape", SHAPES[2:])
def test_identity_returns_the_source(emu_engine, shape):
    A, b, dims = maps_for(shape)["identity"]
    n, h, w = shape
    for dtype in DTYPES:
        vol = volume(shape, dtype, 7)
        near = emu_engine.resample(vol, A, b, dims, "nearest", fill=-7)
        assert same_bits(near[:n, :h, :w], vol) and np.all(near[n:] == -7) and np.all(near[:, h:] == -7) and np.all(near[:, :, w:] == -7)
        lin = emu_engine.resample(vol, A, b, dims, "linear", fill=-7)
        assert same_bits(lin[:n, :h, :w], vol.astype(np.float32)) and np.all(lin[n:] == -7) and np.all(lin[:, :, w:] == -7)


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_label_linear_equals_nearest_under_a_whole_voxel_shift(emu_engine, shape):
    A, b, dims = maps_for(shape)["shift"]
    lab = labels_for(shape, 8)
    near = emu_engine.resample(lab, A, b, dims, "nearest", fill=9)
    assert np.array_equal(emu_engine.resample(lab, A, b, dims, "label_linear", fill=9), near)
    assert (near != 9).any() or min(shape) < 3


def test_label_linear_ties_go_to_the_smaller_label(emu_engine):
    shape = (5, 7, 9)
    lab = labels_for(shape, 9)
    A, b, dims = np.eye(3), np.array([0.0, 0.0, 0.5]), (5, 7, 8)  # between two x neighbours: each of them weighs exactly 0.5
    out = check(emu_engine, lab, A, b, dims, "label_linear", "tie", fill=0)
    assert np.array_equal(out, np.minimum(lab[:, :, :-1], lab[:, :, 1:]))
    assert (lab[:, :, :-1] != lab[:, :, 1:]).sum() > 50  # (ties there are)
    near = emu_engine.resample(lab, A, b, dims, "nearest", fill=0)
    assert np.array_equal(near, lab[:, :, 1:])  # nearest rounds half up instead


@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_float16_and_int16_equal_the_float32_cast(emu_engine, mode):
    shape = (5, 7, 9)
    vol = volume(shape, np.int32, 10) * 12  # beyond the int16 range: saturation
    for name in ("scale", "rotate"):
        A, b, dims = maps_for(shape)[name]
        raw = restate(vol, A, b, dims, mode, fill=-40000, raw=True)
        f32 = check(emu_engine, vol, A, b, dims, mode, name, fill=-40000, dtype=np.float32)
        f16 = check(emu_engine, vol, A, b, dims, mode, name, fill=-40000, dtype=np.float16)
        i16 = check(emu_engine, vol, A, b, dims, mode, name, fill=-40000, dtype=np.int16)
        with np.errstate(over="ignore"):
            assert same_bits(f16, f32.astype(np.float16))
        assert same_bits(f32, raw.astype(np.float32))
        assert np.array_equal(i16, np.clip(np.rint(raw), -32768, 32767).astype(np.int16))
        assert (i16 == -32768).any() and (i16 == 32767).any()


def test_every_output_voxel_outside(emu_engine):
    shape = (5, 7, 9)
    A, b, dims = maps_for(shape)["outside"]
    vol = volume(shape, np.float32, 11)
    for mode, dt in (("linear", np.float32), ("cubic", np.float16), ("nearest", None)):
        out = emu_engine.resample(vol, A, b, dims, mode, fill=-3.5, dtype=dt)
        assert out.shape == tuple(dims) and np.all(out == -3.5)
    nan_map = emu_engine.resample(vol, np.full((3, 3), np.nan), np.zeros(3), dims, "linear", fill=5)  # a NaN coordinate is outside
    assert np.all(nan_map == 5)
    lab = labels_for(shape, 12)
    assert np.all(emu_engine.resample(lab, A, b, dims, "label_linear", fill=200) == 200)


# ---------------------------------------------------------------------------------------------------------------- against scipy
# max |restatement - scipy| / max |v| over the points inside the source, measured on these volumes (uniform noise in +-2060 HU, the
# hardest input for a spline: the coefficients swing beyond the data): 3.70e-15, i.e. 7.6e-12 HU, at (2, 66, 130) "scale"; the
# coefficients alone differ from scipy's by 1.93e-15 of their maximum.  The bar is 4 x the measured maximum, 1.48e-14, rounded up
# to a power of two.
SCIPY_CUBIC_BAR = 2.0 ** -45


def scipy_points(shape, name):
    A, b, dims = maps_for(shape)[name]
    c = coordinates(A, b, dims)
    ok = np.ones(c[0].shape, bool)
    for i in range(3):
        ok &= (c[i] >= 0.0) & (c[i] <= shape[i] - 1.0)
    return A, b, dims, np.stack([c[i][ok] for i in range(3)]), ok


@pytest.mark.parametrize("shape", [(5, 7, 9), (3, 37, 38), (2, 66, 130)])
def test_cubic_against_scipy(emu_engine, shape):
    from scipy import ndimage

    vol = np.random.default_rng(13).integers(-2060, 2061, shape).astype(np.int16)
    coef = ndimage.spline_filter(vol.astype(np.float64), 3, mode="mirror", output=np.float64)
    for name in ("half", "scale", "rotate"):
        A, b, dims, pts, ok = scipy_points(shape, name)
        assert ok.sum() > 20
        want = ndimage.map_coordinates(coef, pts, order=3, mode="mirror", prefilter=False)
        raw = restate(vol, A, b, dims, "cubic", raw=True)[ok]
        rel = float(np.abs(raw - want).max() / np.abs(vol).max())
        print(f"cubic vs scipy {shape} {name}: max |diff| / max |v| = {rel:.3e}")
        assert rel <= SCIPY_CUBIC_BAR
        got = emu_engine.resample(vol, A, b, dims, "cubic")[ok]
        w32 = want.astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(w32))))
    rel_coef = float(np.abs(prefilter(vol) - coef).max() / np.abs(coef).max())
    print(f"coefficients vs scipy {shape}: max relative difference {rel_coef:.3e}")
    assert rel_coef <= SCIPY_CUBIC_BAR


def test_linear_against_scipy(emu_engine):
    from scipy import ndimage

    shape = (5, 37, 38)
    vol = np.random.default_rng(14).integers(-1500, 3500, shape).astype(np.int16)
    for name in ("half", "scale", "rotate"):
        A, b, dims, pts, ok = scipy_points(shape, name)
        want = ndimage.map_coordinates(vol.astype(np.float64), pts, order=1, mode="nearest").astype(np.float32)
        got = emu_engine.resample(vol, A, b, dims, "linear")[ok]
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want))))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(emu_engine):
    eng, lib = emu_engine, emu_engine.L.lib
    p = nat.ResampleParams()
    p.out_dims[:] = [2, 2, 2]
    p.A[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    p.mode, p.out_dtype = 1, 2
    for n, h, w in ((4097, 2, 2), (2, 4097, 2), (2, 2, 4097), (2048, 1024, 1024)):  # (the pointers are never used)
        assert lib.lm_resample_dev(eng.h, 8, 0, n, h, w, C.byref(p), 16) < 0 and b"too large" in lib.lm_last_error()
        assert lib.lm_spline_prefilter_dev(eng.h, 8, 0, n, h, w, 16) < 0 and b"too large" in lib.lm_last_error()
    for dims in ([4097, 1, 1], [1, 1, 4097], [2048, 1024, 1024]):
        p.out_dims[:] = dims
        assert lib.lm_resample_dev(eng.h, 8, 0, 2, 2, 2, C.byref(p), 16) < 0 and b"too large" in lib.lm_last_error()
    assert lib.lm_last_error() == b"lm_resample_dev: output too large (N_0 * N_1 * N_2 must stay below 2^31)"  # the whole text, both kinds
    p.out_dims[:] = [2, 0, 4097]
    assert lib.lm_resample_dev(eng.h, 8, 0, 2, 2, 2, C.byref(p), 16) < 0
    assert lib.lm_last_error() == b"lm_resample_dev: output too large or empty (1 <= out_dims[1] <= 4096, got 0)"
    p.out_dims[:] = [2, 2, 2]
    p.out_dtype = 0  # LM_I16 out of a float source
    for code in (2, 3):
        for mode in (1, 2):
            p.mode = mode
            assert lib.lm_resample_dev(eng.h, 8, code, 2, 2, 2, C.byref(p), 16) < 0 and b"LM_I16 output needs an integer source" in lib.lm_last_error()
    p.mode, p.out_dtype = 0, 2  # nearest with another dtype
    assert lib.lm_resample_dev(eng.h, 8, 0, 2, 2, 2, C.byref(p), 16) < 0 and b"out_dtype must equal dtype" in lib.lm_last_error()
    p.mode, p.out_dtype = 3, 4  # label-linear of an image
    assert lib.lm_resample_dev(eng.h, 8, 0, 2, 2, 2, C.byref(p), 16) < 0 and b"LM_U8" in lib.lm_last_error()
    p.mode = 7
    assert lib.lm_resample_dev(eng.h, 8, 4, 2, 2, 2, C.byref(p), 16) < 0 and b"unknown mode" in lib.lm_last_error()
    # the Python layer refuses them before anything is allocated
    vol = volume((3, 4, 5), np.float32, 15)
    with pytest.raises(ValueError, match="int16"):
        eng.resample(vol, np.eye(3), np.zeros(3), (3, 4, 5), "cubic", dtype=np.int16)
    with pytest.raises(ValueError, match="raw values"):
        eng.resample(vol, np.eye(3), np.zeros(3), (3, 4, 5), "nearest", dtype=np.float16)
    with pytest.raises(nat.LMError, match="too large"):
        eng.resample(vol, np.eye(3), np.zeros(3), (4097, 1, 1), "linear")
    with pytest.raises(ValueError, match="0..255"):
        eng.resample(vol.astype(np.uint8), np.eye(3), np.zeros(3), (3, 4, 5), "label_linear", fill=-1)
