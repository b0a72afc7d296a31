"""lm_warp_dev, lm_demons_step_dev and lm_jacobian_dev on the emulation library, bit for bit against numpy restatements of the
definitions in include/lungmask_hip.h (`warp_oracle`, `demons_step_oracle`, `jacobian_oracle`; test_gpu_deform.py runs the same
cases on the device), their properties and refusals, a five-iteration loop against the same loop written with the oracles, and the
recovery of a known smooth field at a coarse size.

Shapes: the smallest at which each part can go wrong -- (1, 1, 1), where every difference degenerates; (2, 3, 5) against a moving
volume of (4, 2, 7), where the extents differ on every axis; (3, 37, 130), where lines cross the workgroups' shares and the last
workgroup is partial; and a constant 41 x 41 x 41 pair whose squared differences pass 2^32."""
import warnings

import numpy as np
import pytest

from lungmask_amd import _native as nat
from lungmask_amd import deformable as dfm
from lungmask_amd import resample as rs
from tests.test_filters_emu import oracle_separable
from tests.test_register_emu import volume


# ------------------------------------------------------------------------------------------------ the oracles
def same_bits(a, b):
    """Equal dtype, shape and bits; a NaN equals a NaN (which NaN comes out is not defined)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = f"u{a.itemsize}"
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def scales(spacing):
    fs = [1.0, 1.0, 1.0] if spacing is None else [1.0 / float(v) for v in spacing]
    return fs, [v / 2.0 for v in fs]


def coordinate(A, b, shape, field, fs):
    """The coordinate rule -> three float64 arrays of `shape`."""
    A, b = np.asarray(A, np.float64).reshape(3, 3), np.asarray(b, np.float64).reshape(3)
    o = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    p = o if field is None else [o[i] + field[i].astype(np.float64) * fs[i] for i in range(3)]
    return [((A[i, 0] * p[0] + A[i, 1] * p[1]) + A[i, 2] * p[2]) + b[i] for i in range(3)]


def domain(c, ext):
    inside, j = np.ones(c[0].shape, bool), []
    for i in range(3):
        t = np.floor(c[i] + 0.5)
        ok = (t >= 0.0) & (t < float(ext[i]))
        inside &= ok
        j.append(np.where(ok, t, 0.0).astype(np.int64))
    return inside, j


def taps2(c, e):
    c = np.minimum(np.maximum(c, 0.0), float(e - 1))
    c = np.where(np.isnan(c), 0.0, c)  # (an outside voxel: its value is not used)
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, e - 1), c - i0


def lerp(a, b, f):
    return a * (1.0 - f) + b * f


def trilinear(src, c):
    e = src.shape
    (z0, z1, fz), (y0, y1, fy), (x0, x1, fx) = (taps2(c[i], e[i]) for i in range(3))
    s = src.astype(np.float64)
    v00, v01 = lerp(s[z0, y0, x0], s[z0, y0, x1], fx), lerp(s[z0, y1, x0], s[z0, y1, x1], fx)
    v10, v11 = lerp(s[z1, y0, x0], s[z1, y0, x1], fx), lerp(s[z1, y1, x0], s[z1, y1, x1], fx)
    return lerp(lerp(v00, v01, fy), lerp(v10, v11, fy), fz)


def mirror(k, e):
    if e == 1:
        return np.zeros_like(k)
    P = 2 * e - 2
    m = np.mod(k, P)
    return np.where(m >= e, P - m, m)


def taps4(c, e):
    c = np.minimum(np.maximum(c, 0.0), float(e - 1))
    c = np.where(np.isnan(c), 0.0, c)
    i0 = np.floor(c).astype(np.int64)
    f = c - i0
    g = 1.0 - f
    idx = [mirror(i0 - 1 + k, e) for k in range(4)]
    return idx, [((g * g) * g) / 6.0, 2.0 / 3.0 - ((f * f) * (2.0 - f)) / 2.0, 2.0 / 3.0 - ((g * g) * (1.0 + f)) / 2.0, ((f * f) * f) / 6.0]


def cast_out(v, dtype):
    dt = np.dtype(dtype)
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


def warp_oracle(src, field, A, b, out_shape, mode="linear", fill=-1024, dtype=None, spacing=None):
    """lm_warp_dev's definition; for "cubic" `src` is the float64 coefficient volume."""
    fs, _ = scales(spacing)
    ext = src.shape
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        c = coordinate(A, b, out_shape, field, fs)
        inside, j = domain(c, ext)
        if mode == "nearest":
            return np.where(inside, src[j[0], j[1], j[2]], nearest_fill(src.dtype, fill)).astype(src.dtype)
        if mode == "linear":
            v = trilinear(src, c)
        elif mode == "cubic":
            (iz, wz), (iy, wy), (ix, wx) = (taps4(c[i], ext[i]) for i in range(3))
            v = np.zeros(c[0].shape)
            for a in range(4):
                vy = np.zeros(c[0].shape)
                for bb in range(4):
                    vx = np.zeros(c[0].shape)
                    for k in range(4):
                        vx = vx + wx[k] * src[iz[a], iy[bb], ix[k]]
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
        return cast_out(np.where(inside, v, float(fill)), np.float32 if dtype is None else dtype)


def demons_step_oracle(fixed, moving, u, A, b, spacing=None, inv_k2=1.0, den_min=1e-9, labels=None, keep=None):
    """lm_demons_step_dev's definition -> (out float32 [3][n][h][w], counts: five Python integers)."""
    fs, gs = scales(spacing)
    shape = fixed.shape
    F = fixed.astype(np.float64)
    sel = np.ones(shape, bool)
    if labels is not None:
        table = np.zeros(256, bool)
        table[list(range(1, 256)) if keep is None else list(keep)] = True
        sel = table[labels]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        fnan = np.isnan(F)
        c = coordinate(A, b, shape, u, fs)
        inside, _ = domain(c, moving.shape)
        m = trilinear(moving, c)
        g = []
        for j in range(3):
            if shape[j] == 1:
                g.append(np.zeros(shape))
                continue
            idx = np.arange(shape[j])
            hi, lo = np.take(F, np.minimum(idx + 1, shape[j] - 1), axis=j), np.take(F, np.maximum(idx - 1, 0), axis=j)
            g.append((hi - lo) * gs[j])
        nan = np.isnan(m) | np.isnan(g[0]) | np.isnan(g[1]) | np.isnan(g[2])
        d = F - m
        dd = d * d
        den = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + dd * inv_k2
        still = den < den_min
        c_nan = sel & (fnan | (inside & nan))
        c_out = sel & ~fnan & ~inside
        c_in = sel & ~fnan & inside & ~nan
        out = np.empty((3,) + shape, np.float32)
        for j in range(3):
            step = np.where(still, 0.0, (d * g[j]) / den)
            out[j] = np.where(c_in, (u[j].astype(np.float64) + step).astype(np.float32), u[j])
        capped = np.where(dd < 16777216.0, dd, 16777216.0)
        terms = np.floor(capped * 16.0 + 0.5)[c_in]
    ssd = sum(int(t) for t in terms.astype(np.int64).reshape(-1)) if terms.size < 4096 else int(terms.astype(np.int64).sum())
    return out, [int(sel.sum()), int(c_in.sum()), int(c_out.sum()), int(c_nan.sum()), ssd]


def jacobian_oracle(field, spacing=None):
    """lm_jacobian_dev's definition -> (det float32 [n][h][w], folded, nan)."""
    fs, _ = scales(spacing)
    shape = field.shape[1:]
    a = [[None] * 3 for _ in range(3)]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i in range(3):
            ui = field[i].astype(np.float64)
            for j in range(3):
                e = shape[j]
                G = np.zeros(shape)
                if e > 1:
                    G = np.moveaxis(G, j, 0)
                    s = np.moveaxis(ui, j, 0)
                    G[1:-1] = ((s[2:] - s[:-2]) * fs[i]) * 0.5
                    G[0] = (s[1] - s[0]) * fs[i]
                    G[-1] = (s[-1] - s[-2]) * fs[i]
                    G = np.moveaxis(G, 0, j)
                a[i][j] = (1.0 if i == j else 0.0) + G
        det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) + \
            a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])
        return det.astype(np.float32), int((det <= 0.0).sum()), int(np.isnan(det).sum())


# ------------------------------------------------------------------------------------------------ cases
SHAPES = [((1, 1, 1), (1, 1, 1)), ((2, 3, 5), (4, 2, 7)), ((3, 37, 130), (3, 37, 130))]
SHAPE_IDS = ["x".join(map(str, s[0])) for s in SHAPES]
FIELDS = ["null", "zeros", "shift", "random", "special"]
SPACING = (2.5, 0.7, 0.8)


def rot_scale():
    a = np.radians(4.0)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    return R @ np.diag([0.8, 1.05, 0.93]), np.array([0.3, -0.7, 1.2])


def make_field(kind, shape, seed=0, spacing=None):
    """The five fields of the issue, in the units of `spacing`: None (NULL), zeros, a shift by whole voxels, a random field of a few
    voxels' amplitude that throws some samples outside, and one with NaN and inf entries."""
    if kind == "null":
        return None
    sp = np.ones(3) if spacing is None else np.asarray(spacing, np.float64)
    f = np.zeros((3,) + tuple(shape), np.float32)
    if kind == "shift":
        for i, s in enumerate((1.0, -2.0, 3.0)):
            f[i] = np.float32(s * sp[i])
    elif kind in ("random", "special"):
        rng = np.random.default_rng(seed)
        f = (rng.normal(0.0, 2.0, f.shape) * sp.reshape(3, 1, 1, 1)).astype(np.float32)
        if kind == "special":
            flat = f.reshape(-1)
            pos = rng.choice(flat.size, min(6, flat.size), replace=False)
            flat[pos] = [np.nan, np.inf, -np.inf, np.nan, 1e30, -1e30][:pos.size]
    return f


def check_warp(eng, src, field, A, b, out_shape, mode, fill=-1024, dtype=None, spacing=None):
    coef = eng.spline_prefilter(src) if mode == "cubic" else src
    got = eng.warp(src, field, A, b, out_shape, mode, fill, dtype, spacing)
    want = warp_oracle(coef, field, A, b, out_shape, mode, fill, dtype, spacing)
    assert same_bits(got, want), (mode, np.argwhere(got != want)[:5])
    return got


def run_warp_cases(eng, shapes, kind):
    out_shape, src_shape = shapes
    A, b = (np.eye(3), np.zeros(3)) if kind in ("null", "zeros", "shift") and out_shape == (1, 1, 1) else rot_scale()
    field = make_field(kind, out_shape, 3, SPACING)
    img = volume(src_shape, np.int16, 1)
    lab = volume(src_shape, np.uint8, 2)
    for mode, src, fill, dt in (("nearest", img, -1000, None), ("linear", img, -1024, None), ("cubic", img, -1024, None),
                                ("label_linear", lab, 0, None), ("nearest", lab, 9, None)):
        got = check_warp(eng, src, field, A, b, out_shape, mode, fill, dt, SPACING)
        if kind in ("null", "zeros"):  # the coordinate rule gives p = o exactly: lm_resample_dev bit for bit
            assert same_bits(got, eng.resample(src, A, b, out_shape, mode, fill, dt))


def run_warp_dtypes(eng):
    A, b = rot_scale()
    field = make_field("random", (2, 3, 5), 4)
    for dt in (np.int16, np.int32, np.int64, np.float32, np.float64):
        src = volume((4, 2, 7), dt, 5)
        check_warp(eng, src, field, A, b, (2, 3, 5), "nearest", -3)
        for out in (np.float32, np.float16) + ((np.int16,) if np.dtype(dt).kind == "i" else ()):
            check_warp(eng, src, field, A, b, (2, 3, 5), "linear", -1024, out)
    src = volume((4, 2, 7), np.int16, 6)
    for out in (np.float32, np.float16, np.int16):
        check_warp(eng, src, field, A, b, (2, 3, 5), "cubic", -1024, out)


def run_whole_voxel_shift(eng):
    """A field of whole voxels equals a translation by b, in every mode (a power-of-two spacing, so that u / spacing is exact)."""
    src, lab = volume((5, 9, 11), np.int16, 7), volume((5, 9, 11), np.uint8, 8)
    sp = (2.0, 0.5, 4.0)
    field = make_field("shift", (4, 8, 12), spacing=sp)
    A = np.eye(3)
    for mode, s, fill in (("nearest", src, -7), ("linear", src, -1024), ("cubic", src, -1024), ("label_linear", lab, 0)):
        got = eng.warp(s, field, A, np.zeros(3), (4, 8, 12), mode, fill, spacing=sp)
        assert same_bits(got, eng.resample(s, A, np.array([1.0, -2.0, 3.0]), (4, 8, 12), mode, fill))
    assert same_bits(eng.warp(lab, field, A, np.zeros(3), (4, 8, 12), "label_linear", 0, spacing=sp),
                     eng.warp(lab, field, A, np.zeros(3), (4, 8, 12), "nearest", 0, spacing=sp))


def demons_host(eng, fixed, moving, u, A, b, spacing=None, inv_k2=1.0, den_min=1e-9, labels=None, keep=None):
    with eng.scope() as dev:
        out, counts = dev.empty(u.shape, np.float32), dev.empty((5,), np.int64)
        out.upload(np.full(u.shape, -77.0, np.float32))  # a dirty output: fully written
        counts.upload(np.full(5, -1, np.int64))
        eng.demons_step_dev(dev.upload(fixed), dev.upload(moving), dev.upload(u), out, counts, A, b, spacing, inv_k2, den_min,
                            dev.upload(labels) if labels is not None else None, keep)
        eng.sync()
        return out.download(), [int(v) for v in counts.download()]


def check_demons(eng, fixed, moving, u, A, b, **kw):
    got, counts = demons_host(eng, fixed, moving, u, A, b, **kw)
    want, wc = demons_step_oracle(fixed, moving, u, A, b, **kw)
    assert counts == wc, (counts, wc)
    assert counts[0] == counts[1] + counts[2] + counts[3]
    assert same_bits(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    return got, counts


def run_demons_cases(eng, shapes, kind):
    fshape, mshape = shapes
    A, b = rot_scale()
    u = make_field("zeros" if kind == "null" else kind, fshape, 9, SPACING)
    fixed, moving = volume(fshape, np.int16, 10), volume(mshape, np.float32, 11)
    labels = np.random.default_rng(12).integers(0, 4, fshape).astype(np.uint8)
    check_demons(eng, fixed, moving, u, A, b, spacing=SPACING, inv_k2=0.25, den_min=1e-9)
    got, counts = check_demons(eng, fixed, moving, u, A, b, spacing=SPACING, inv_k2=0.25, den_min=1e-9, labels=labels, keep=(1, 3))
    keep = np.isin(labels, (1, 3))
    assert counts[0] == int(keep.sum()) and same_bits(got[:, ~keep], u[:, ~keep])  # an unselected voxel keeps u


DEMONS_DTYPES = [np.int16, np.int32, np.int64, np.float32, np.float64]


def run_demons_dtypes(eng, fdtype, mdtype):
    A, b = rot_scale()
    fixed, moving = volume((5, 7, 9), fdtype, 13), volume((4, 6, 11), mdtype, 14)
    u = make_field("random", (5, 7, 9), 15)
    _, counts = check_demons(eng, fixed, moving, u, A, b, inv_k2=0.01, den_min=1e-3)
    if np.dtype(fdtype).kind == "f":
        assert counts[3] >= 1  # the NaN of the fixed volume
    labels = np.random.default_rng(16).integers(0, 3, fixed.shape).astype(np.uint8)
    check_demons(eng, fixed, moving, u, A, b, inv_k2=0.0, den_min=0.0, labels=labels)


def run_demons_properties(eng):
    # a constant difference of 4096 over 41^3 voxels: every term is the cap 2^24 * 16 = 2^28, the sum passes 2^32
    fixed, moving = np.full((41, 41, 41), 3000, np.int16), np.full((41, 41, 41), -1096, np.int16)
    zero = np.zeros((3, 41, 41, 41), np.float32)
    got, counts = check_demons(eng, fixed, moving, zero, np.eye(3), np.zeros(3))
    assert counts == [68921, 68921, 0, 0, 68921 * 2 ** 28] and counts[4] > 2 ** 32
    assert not got.any()  # no gradient: no step
    # fixed == moving, a zero field and the identity: nothing moves and nothing differs
    vol = volume((3, 37, 130), np.int16, 17)
    u = np.zeros((3,) + vol.shape, np.float32)
    got, counts = check_demons(eng, vol, vol, u, np.eye(3), np.zeros(3))
    assert same_bits(got, u) and counts[4] == 0 and counts[1] == vol.size
    # a step is never longer than k / 2
    moving = volume((3, 37, 130), np.int16, 18)
    got, _ = check_demons(eng, vol, moving, u, np.eye(3), np.zeros(3), inv_k2=1.0 / (4.0 * 0.25))
    assert np.sqrt((got.astype(np.float64) ** 2).sum(axis=0)).max() <= 0.5 * (1 + 1e-6)


def linear_field(shape, G, spacing):
    """u_i = sum_j G_ij o_j / field_scale_i: exact in float32 for entries of G that are multiples of 1/8 and power-of-two spacings."""
    o = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.stack([(G[i, 0] * o[0] + G[i, 1] * o[1] + G[i, 2] * o[2]) * spacing[i] for i in range(3)]).astype(np.float32)


def run_jacobian_cases(eng):
    for shape in ((1, 1, 1), (2, 3, 5), (3, 37, 130), (1, 4, 1)):
        for kind in ("zeros", "shift", "random", "special"):
            field = make_field(kind, shape, 19, SPACING)
            det, folded, nan = eng.jacobian(field, SPACING)
            want, wf, wn = jacobian_oracle(field, SPACING)
            assert same_bits(det, want) and (folded, nan) == (wf, wn), (shape, kind)
            if kind in ("zeros", "shift"):
                assert np.all(det == 1.0) and folded == 0
            if kind == "special" and min(shape) > 1:
                assert nan >= 1
    # a linear field has an exact Jacobian at every voxel, the border included
    G = np.array([[0.125, -0.25, 0.5], [0.375, -0.125, 0.25], [-0.5, 0.125, 0.625]])
    spacing = (2.0, 0.5, 4.0)
    field = linear_field((5, 6, 7), G, spacing)
    det, folded, nan = eng.jacobian(field, spacing)
    assert np.all(det.view(np.uint32) == np.float32(np.linalg.det(np.eye(3) + G)).view(np.uint32)) and (folded, nan) == (0, 0)
    assert same_bits(det, jacobian_oracle(field, spacing)[0])
    # a field built to fold: the x component runs back faster than the index advances on a slab of four voxels per line; one NaN
    # in the interior reaches its six neighbours' central differences (not its own)
    fold = np.zeros((3, 4, 9, 20), np.float32)
    fold[2, :, :, 8:14] = -1.5 * np.arange(6, dtype=np.float32)
    fold[0, 2, 4, 3] = np.nan
    det, folded, nan = eng.jacobian(fold)
    want, wf, wn = jacobian_oracle(fold)
    assert same_bits(det, want) and (folded, nan) == (wf, wn) and folded == 4 * 9 * 4 and nan == 6
    # without the counts, and into a dirty output
    with eng.scope() as dev:
        out = dev.empty(fold.shape[1:], np.float32)
        out.upload(np.full(fold.shape[1:], 7.0, np.float32))
        assert same_bits(eng.jacobian_dev(dev.upload(fold), out=out).download(), want)


# ------------------------------------------------------------------------------------------------ a loop of five iterations
def oracle_level(fixed_l, moving_l, labels_l, keep, u, A, b, spacing, iterations, taps, inv_k2, den_min, patience):
    """`deformable.run_level` written with the oracles -> (field, metrics, reason)."""
    rule, metrics, why = dfm.StopRule(patience), [], "iterations"
    for _ in range(iterations):
        v, c = demons_step_oracle(fixed_l, moving_l, u, A, b, spacing, inv_k2, den_min, labels_l, keep)
        u = np.stack([oracle_separable(v[i], None, taps) for i in range(3)])
        metrics.append([c[4], c[1]])
        stop = rule.update((c[4], c[1]))
        if stop is not None:
            why = stop
            break
    return u, metrics, why


def device_level(eng, fixed_l, moving_l, labels_l, keep, u, A, b, grid, iterations, taps, inv_k2, den_min, patience):
    with eng.scope() as dev:
        ud, vd, counts = dev.upload(u), dev.empty(u.shape, np.float32), dev.empty((5,), np.int64)
        ran, metrics, why = dfm.run_level(eng, dev.upload(fixed_l), dev.upload(moving_l), dev.upload(labels_l) if labels_l is not None else None,
                                          keep, ud, vd, counts, A, b, grid, iterations, taps, inv_k2, den_min, patience)
        eng.sync()
        return ud.download(), metrics, why


def run_five_iterations(eng):
    fixed, moving, _ = recovery_pair()
    fixed, moving = fixed[4:20, 8:32, 8:36].astype(np.float32), moving[4:20, 8:32, 8:36].astype(np.float32)
    grid = rs.Grid(fixed.shape, (0.8, 0.7, 2.5))
    labels = np.zeros(fixed.shape, np.uint8)
    labels[2:-2, 3:-3, 3:-3] = 1
    taps, inv_k2 = dfm.field_taps(grid, None), dfm.level_inv_k2(grid, None)
    u0 = np.zeros((3,) + fixed.shape, np.float32)
    for lab in (None, labels):
        got = device_level(eng, fixed, moving, lab, None, u0, np.eye(3), np.zeros(3), grid, 5, taps, inv_k2, 1e-9, 5)
        want = oracle_level(fixed, moving, lab, None, u0, np.eye(3), np.zeros(3), (2.5, 0.7, 0.8), 5, taps, inv_k2, 1e-9, 5)
        assert same_bits(got[0], want[0]) and got[1] == want[1] and got[2] == want[2] == "iterations"
        assert len(got[1]) == 5 and got[1][-1][0] * got[1][0][1] < got[1][0][0] * got[1][-1][1]  # the metric fell


# ------------------------------------------------------------------------------------------------ recovery of a known field
RECOVERY_SHAPE = (28, 44, 44)
RECOVERY_KW = dict(levels_mm=(2.0, 1.0), iterations=(40, 20))
_PAIR = {}


def content(z, y, x):
    """A smooth synthetic image that can be evaluated anywhere: a few Gaussian blobs on a ramp (HU-like values)."""
    v = -800.0 + 6.0 * z + 4.0 * y - 3.0 * x
    for cz, cy, cx, s, amp in ((9.0, 14.0, 13.0, 5.0, 700.0), (17.0, 28.0, 30.0, 6.0, -350.0), (12.0, 30.0, 12.0, 4.0, 500.0),
                               (20.0, 12.0, 31.0, 5.0, 600.0), (6.0, 24.0, 24.0, 4.5, -300.0), (22.0, 34.0, 20.0, 5.0, 450.0),
                               (14.0, 20.0, 22.0, 4.0, 550.0), (7.0, 36.0, 34.0, 4.5, 500.0), (21.0, 22.0, 9.0, 4.0, -400.0),
                               (5.0, 9.0, 33.0, 4.0, -350.0)):
        v = v + amp * np.exp(-((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2) / (2.0 * s * s))
    return v


def recovery_pair():
    """(fixed int16, moving int16, the true field float64 [3][n][h][w] in voxels on the fixed grid): fixed(o) = content(o + u(o)),
    moving(o) = content(o), each with its own N(0, 20) noise.  u: one sinusoid period per axis, peak 2 voxels, zero at the border."""
    if not _PAIR:
        n, h, w = RECOVERY_SHAPE
        z, y, x = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        sz, sy, sx = np.sin(2 * np.pi * z / (n - 1)), np.sin(2 * np.pi * y / (h - 1)), np.sin(2 * np.pi * x / (w - 1))
        env = np.sin(np.pi * z / (n - 1)) * np.sin(np.pi * y / (h - 1)) * np.sin(np.pi * x / (w - 1))  # zero at the border
        u = np.stack([2.0 * env * sy, 2.0 * env * sx, 2.0 * env * sz])
        u *= 2.0 / np.abs(u).max()
        rng = np.random.default_rng(7)
        fixed = np.rint(content(z + u[0], y + u[1], x + u[2]) + rng.normal(0.0, 20.0, z.shape)).astype(np.int16)
        moving = np.rint(content(z, y, x) + rng.normal(0.0, 20.0, z.shape)).astype(np.int16)
        for a in (fixed, moving, u):
            a.setflags(write=False)
        _PAIR["pair"] = (fixed, moving, u)
    return _PAIR["pair"]


def recovery_figures(reg, truth):
    """(mean end-point error, mean length of the true field) in voxels over the voxels at least 4 from the border, the metric ratio
    final / initial, and the Jacobian's range."""
    inner = (slice(None),) + (slice(4, -4),) * 3
    err = np.sqrt(((reg.field.array.astype(np.float64) - truth)[inner] ** 2).sum(axis=0)).mean()
    length = np.sqrt((truth[inner] ** 2).sum(axis=0)).mean()
    return float(err), float(length)


def check_recovery(eng, reg=None):
    fixed, moving, truth = recovery_pair()
    reg = reg or dfm.register_deformable(fixed, moving, engine=eng, **RECOVERY_KW)
    err, length = recovery_figures(reg, truth)
    det, info = reg.jacobian(engine=eng)
    (i_ssd, i_n), (f_ssd, f_n) = reg.initial_metric, reg.final_metric
    print(f"recovery: end-point error {err:.3f} of {length:.3f} voxels; mean squared difference {i_ssd / 16 / i_n:.1f} -> {f_ssd / 16 / f_n:.1f}; "
          f"Jacobian {info['min']:.3f} .. {info['max']:.3f}; iterations {[lv['iterations'] for lv in reg.levels]} ({[lv['stopped'] for lv in reg.levels]})")
    assert err <= 0.5 * length
    assert 2 * f_ssd * i_n <= i_ssd * f_n  # the final mean squared difference is at most half of the initial one, in integers
    assert info["folded"] == 0 and info["nonfinite"] == 0 and reg.folding == {"folded": 0, "nonfinite": 0}
    for lv in reg.levels:  # never more than `patience` iterations in a row that are not below the lowest value so far
        assert dfm.run_stop_rule(lv["metric"], dfm.PATIENCE) == (lv["iterations"], lv["stopped"])
        assert lv["iterations"] <= dict(zip(RECOVERY_KW["levels_mm"], RECOVERY_KW["iterations"]))[lv["level_mm"]]
    return reg


def oracle_first_level(eng):
    """The first level of `register_deformable` on the recovery pair with the loop written with the oracles; the level's volumes come
    from the engine's filter and resampler (covered bit for bit by their own tests)."""
    fixed, moving, _ = recovery_pair()
    grid = rs.Grid.of(fixed)
    level = dfm.level_grid(grid, RECOVERY_KW["levels_mm"][0])
    A0, b0 = rs.index_map(grid, level, None)
    vols = [eng.resample(eng.filter(v, kind="separable", taps=dfm.antialias_taps(grid, level)), A0, b0, level.shape, "linear", 0.0, np.float32)
            for v in (fixed, moving)]
    A, b = rs.index_map(level, level, None)
    u0 = np.zeros((3,) + level.shape, np.float32)
    return oracle_level(vols[0], vols[1], None, None, u0, A, b, dfm.spacing_zyx(level), RECOVERY_KW["iterations"][0], dfm.field_taps(level, None),
                        dfm.level_inv_k2(level, None), dfm.DEN_MIN, dfm.PATIENCE), level


def run_recovery(eng):
    reg = check_recovery(eng)
    # bit-identity with the oracle loop for the first level: the same registration stopped after that level returns its field
    (want, metrics, why), level = oracle_first_level(eng)
    first = dfm.register_deformable(recovery_pair()[0], recovery_pair()[1], engine=eng, levels_mm=RECOVERY_KW["levels_mm"][:1],
                                    iterations=RECOVERY_KW["iterations"][:1])
    assert first.levels[0]["metric"] == metrics == reg.levels[0]["metric"] and first.levels[0]["stopped"] == why
    grid = rs.Grid.of(recovery_pair()[0])
    A, b = rs.index_map(level, grid, None)
    up = np.stack([eng.resample(want[i], A, b, grid.shape, "linear", 0.0, np.float32) for i in range(3)])
    assert same_bits(first.field.array, up)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shapes", SHAPES, ids=SHAPE_IDS)
def test_warp(emu_engine, shapes, kind):
    run_warp_cases(emu_engine, shapes, kind)


def test_warp_dtypes(emu_engine):
    run_warp_dtypes(emu_engine)


def test_whole_voxel_field_is_a_translation(emu_engine):
    run_whole_voxel_shift(emu_engine)


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shapes", SHAPES, ids=SHAPE_IDS)
def test_demons_step(emu_engine, shapes, kind):
    run_demons_cases(emu_engine, shapes, kind)


@pytest.mark.parametrize("mdtype", DEMONS_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fdtype", DEMONS_DTYPES, ids=lambda d: np.dtype(d).name)
def test_demons_dtypes(emu_engine, fdtype, mdtype):
    run_demons_dtypes(emu_engine, fdtype, mdtype)


def test_demons_properties(emu_engine):
    run_demons_properties(emu_engine)


def test_jacobian(emu_engine):
    run_jacobian_cases(emu_engine)


def test_five_iterations_equal_the_oracle_loop(emu_engine):
    run_five_iterations(emu_engine)


def test_recovery_of_a_known_field(emu_engine):
    run_recovery(emu_engine)


def test_refusals(emu_engine):
    eng = emu_engine
    vol = np.zeros((2, 3, 4), np.int16)
    I, z = np.eye(3), np.zeros(3)
    with eng.scope() as dev:
        vd, u = dev.upload(vol), dev.upload(np.zeros((3, 2, 3, 4), np.float32))
        v, counts = dev.empty((3, 2, 3, 4), np.float32), dev.empty((5,), np.int64)
        with pytest.raises(nat.LMError, match="in-place"):
            eng.demons_step_dev(vd, vd, u, u, counts, I, z)
        p = nat.DemonsParams()
        rc = eng.L.lib.lm_demons_step_dev(eng.h, vd.ptr, 0, 2, 3, 4, None, vd.ptr, 0, 2, 3, 4, u.ptr, p, u.ptr, counts.ptr)
        assert rc < 0 and b"in-place" in eng.L.lib.lm_last_error()
        rc = eng.L.lib.lm_demons_step_dev(eng.h, vd.ptr, 0, 2, 3, 4, None, vd.ptr, 0, 2, 3, 4, u.ptr, p, None, counts.ptr)
        assert rc < 0 and b"not NULL" in eng.L.lib.lm_last_error()
        for bad in (dev.upload(np.zeros((2, 3, 4), np.uint8)), dev.upload(np.zeros((2, 3, 4), np.uint16))):
            with pytest.raises(nat.LMError, match="dtype"):
                eng.demons_step_dev(bad, vd, u, v, counts, I, z)
            with pytest.raises(nat.LMError, match="dtype"):
                eng.demons_step_dev(vd, bad, u, v, counts, I, z)
        rc = eng.L.lib.lm_demons_step_dev(eng.h, vd.ptr, 4, 2, 3, 4, None, vd.ptr, 0, 2, 3, 4, u.ptr, p, v.ptr, counts.ptr)
        assert rc < 0 and b"dtype must be" in eng.L.lib.lm_last_error()
        with pytest.raises(nat.LMError, match="field must be"):
            eng.demons_step_dev(vd, vd, dev.upload(np.zeros((3, 2, 3, 5), np.float32)), v, counts, I, z)
        # an unprefiltered cubic source, a NULL output, a field that is the output
        with pytest.raises(ValueError, match="coefficients"):
            eng.warp_dev(vd, None, I, z, (2, 3, 4), "cubic")
        rp = nat.ResampleParams()
        rp.out_dims[:] = [2, 3, 4]
        rp.mode, rp.out_dtype = nat.RESAMPLE_MODES["cubic"], 2
        fs = eng.field_scale(None)
        out = dev.empty((2, 3, 4), np.float32)
        assert eng.L.lib.lm_warp_dev(eng.h, vd.ptr, 0, 2, 3, 4, None, rp, fs, out.ptr) < 0 and b"coefficients" in eng.L.lib.lm_last_error()
        rp.mode = nat.RESAMPLE_MODES["linear"]
        assert eng.L.lib.lm_warp_dev(eng.h, vd.ptr, 0, 2, 3, 4, None, rp, fs, None) < 0 and b"bad arguments" in eng.L.lib.lm_last_error()
        assert eng.L.lib.lm_warp_dev(eng.h, vd.ptr, 0, 2, 3, 4, out.ptr, rp, fs, out.ptr) < 0
        assert eng.L.lib.lm_warp_dev(eng.h, vd.ptr, 0, 2, 3, 4, None, rp, fs, out.ptr) == 0
        for dims, text in (([2, 3, 4097], b"lm_warp_dev: output too large or empty (1 <= out_dims[2] <= 4096, got 4097)"),
                           ([2048, 1024, 1024], b"lm_warp_dev: output too large (N_0 * N_1 * N_2 must stay below 2^31)")):
            rp.out_dims[:] = dims  # (refused before anything is read or written)
            assert eng.L.lib.lm_warp_dev(eng.h, vd.ptr, 0, 2, 3, 4, None, rp, fs, out.ptr) < 0 and eng.L.lib.lm_last_error() == text
        rp.out_dims[:] = [2, 3, 4]
        assert eng.L.lib.lm_jacobian_dev(eng.h, u.ptr, 2, 3, 4, fs, None, None) < 0 and b"bad arguments" in eng.L.lib.lm_last_error()
        assert eng.L.lib.lm_jacobian_dev(eng.h, u.ptr, 2, 3, 4, fs, u.ptr + 96, None) < 0 and b"inside the field" in eng.L.lib.lm_last_error()
        with pytest.raises(nat.LMError, match="float32"):
            eng.jacobian_dev(dev.upload(np.zeros((3, 2, 3, 4), np.float64)))
    # dimensions over the limits, refused before anything is read
    wide = np.zeros((1, 1, 4097), np.int16)
    with pytest.raises(nat.LMError, match="too large"):
        eng.warp(wide, None, I, z, (1, 1, 2))
    with pytest.raises(nat.LMError, match="too large"):
        eng.warp(vol, None, I, z, (1, 1, 4097))
    with pytest.raises(nat.LMError, match="too large"):
        eng.jacobian(np.zeros((3, 1, 1, 4097), np.float32))
    p = nat.DemonsParams()
    rc = eng.L.lib.lm_demons_step_dev(eng.h, 8, 0, 1, 1, 4097, None, 8, 0, 1, 1, 1, 8, p, 16, 24)  # (no pointer is followed)
    assert rc < 0 and b"4096" in eng.L.lib.lm_last_error()
    with pytest.raises(ValueError, match="spacing"):
        eng.jacobian(np.zeros((3, 1, 1, 2), np.float32), (1.0, 0.0, 1.0))


def test_host_functions_on_the_emulator(emu_engine):
    """warp_image / warp_labels / jacobian_determinant against the oracles through the geometry of two different grids."""
    from lungmask_amd import volume_io

    eng = emu_engine
    moving = volume_io.Volume(volume((4, 6, 11), np.int16, 21), (0.9, 0.6, 2.0), (-10.0, 31.0, 5.5))
    grid = rs.Grid((5, 7, 9), (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), [[0, 1, 0], [1, 0, 0], [0, 0, -1]])
    T = rs.Affine.rotation((0, 0, 1), 5.0).compose(rs.Affine.translation((1.0, -2.0, 0.5)))
    field = dfm.DisplacementField(make_field("random", grid.shape, 22, dfm.spacing_zyx(grid)), grid, T)
    A, b = rs.index_map(rs.Grid.of(moving), grid, T)
    sp = dfm.spacing_zyx(grid)
    for order, mode in ((0, "nearest"), (1, "linear"), (3, "cubic")):
        got = dfm.warp_image(moving, field, order, engine=eng)
        src = eng.spline_prefilter(moving.array) if order == 3 else moving.array
        assert same_bits(got.array, warp_oracle(src, field.array, A, b, grid.shape, mode, -1024, None, sp)) and got.spacing == grid.spacing
    zero = dfm.DisplacementField.zeros(grid, T)
    assert same_bits(dfm.warp_image(moving, zero, 3, engine=eng).array, rs.resample_image(moving, grid, T, 3, engine=eng).array)
    lab = moving.like(volume((4, 6, 11), np.uint8, 23))
    for mode, m in (("nearest", "nearest"), ("linear", "label_linear")):
        assert same_bits(dfm.warp_labels(lab, field, mode, engine=eng).array, warp_oracle(lab.array, field.array, A, b, grid.shape, m, 0, None, sp))
    det, info = dfm.jacobian_determinant(field, engine=eng)
    want, wf, wn = jacobian_oracle(field.array, sp)
    assert same_bits(det, want) and (info["folded"], info["nonfinite"]) == (wf, wn) and info["min"] == float(want.min())
    with pytest.raises(TypeError, match="DisplacementField"):
        dfm.warp_image(moving, field.array, engine=eng)


def test_apply_deformable_on_the_emulator(emu_engine, monkeypatch):
    """The two stages on the device-resident input and labels equal the stand-alone functions the docstring names, in the one-GPU
    branch and in the detour of the multi-GPU forms."""
    from lungmask_amd import morphology, registration as reg
    from tests.test_mask_wrappers_emu import Harness
    from tests.test_register_emu import REG_SPACING, RIGID_CASES, lung_classes, registration_case

    fixed, moving, _ = registration_case("rigid", RIGID_CASES["a"])
    labels = (lung_classes(fixed.array) == 1).astype(np.uint8)
    labels[:, :, 44:] *= 2  # two labels
    h = Harness(emu_engine, labels)
    try:
        rkw = dict(levels_mm=(8.0,), max_evaluations=20)
        dkw = dict(levels_mm=(8.0, 6.0), iterations=(4, 3))
        rim = morphology.dilate(fixed.like(labels), 6.0, engine=emu_engine)
        first = reg.register(fixed, moving, "rigid", labels=rim, moving_spacing=REG_SPACING, engine=emu_engine, **rkw)
        want = dfm.register_deformable(fixed, moving, initial=first, labels=rim, moving_spacing=REG_SPACING, engine=emu_engine, **dkw)
        image = want.resample(moving, moving_spacing=REG_SPACING, engine=emu_engine).array
        for host in (False, True):
            if host:
                monkeypatch.setattr(h.inf, "_shard", object())
            out, r = h.inf.apply_deformable(fixed, moving, margin_mm=6.0, moving_spacing=REG_SPACING, register_kw=rkw, **dkw)
            assert np.array_equal(out, labels) and h.applied == (1 if host else 0)
            assert r.affine_registration.parameters == first.parameters and r.levels == want.levels
            assert same_bits(r.field.array, want.field.array) and same_bits(r.image, image) and r.image.shape == labels.shape
            assert (r.initial_metric, r.final_metric, r.folding) == (want.initial_metric, want.final_metric, want.folding)
            assert r.field_dev is None and r.meta()["affine"]["parameters"] == first.parameters
        selected = int(np.asarray(rim.array if hasattr(rim, "array") else rim).astype(bool).sum())
        assert 0 < r.levels[-1]["metric"][0][1] < labels.size and selected < labels.size
        with pytest.raises(TypeError, match="unexpected"):
            h.inf.apply_deformable(fixed, moving, moving_spacing=REG_SPACING, labels=labels)
        with pytest.raises(ValueError, match="same length"):
            h.inf.apply_deformable(fixed, moving, moving_spacing=REG_SPACING, levels_mm=(8.0,), iterations=(1, 2))
    finally:
        monkeypatch.undo()
        h.inf.close()
    e = Harness(emu_engine, np.zeros_like(labels))
    try:
        with pytest.raises(ValueError, match="no voxel is labelled"):
            e.inf.apply_deformable(fixed, moving, moving_spacing=REG_SPACING)
    finally:
        e.inf.close()
