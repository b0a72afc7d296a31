"""Label morphology (lm_nearest_label_dev, lm_morph_dev) on the g++ emulation of the kernel sources, bit for bit against a numpy
oracle that applies the definitions of include/lungmask_hip.h literally: the three min-plus passes on (distance, label) pairs in
lexicographic order, and the set definitions of the four operators on the WHOLE volume (the device confines itself to a box)."""
import numpy as np
import pytest

from lungmask_amd import _native as nat
from tests.test_metrics_emu import SPACINGS, WORD_SPACINGS, bits, oracle_edt, word_boundary_rows

SHAPES = [(5, 9, 70), (1, 40, 33), (33, 1, 20), (12, 1, 1)]
OPS = ("dilate", "erode", "open", "close")


def table(values, lo=1):
    """bool[256]: None = every label >= 1."""
    t = np.zeros(256, bool)
    if values is None:
        t[lo:] = True
    else:
        t[list(values)] = True
    return t


def lexmin(d, k, axis):
    """The lexicographic minimum of the pairs (d, k) along `axis`: the smallest d, then the smallest k among those."""
    dm = d.min(axis=axis)
    km = np.where(d == np.expand_dims(dm, axis), k, 256).min(axis=axis)
    return dm.astype(np.float32), km.astype(np.int64)


def oracle_nearest(lab: np.ndarray, keep=None, spacing=None):
    """(d2, near) of lm_nearest_label_dev: oracle_edt's broadcast, on pairs."""
    sp = (1.0, 1.0, 1.0) if spacing is None else spacing
    wz, wy, wx = (np.float32(float(s) * float(s)) for s in sp)
    n, h, w = lab.shape
    feat = table(keep)[lab]
    ix, iy, iz = np.arange(w), np.arange(h), np.arange(n)
    cx = wx * ((ix[:, None] - ix[None, :]) ** 2).astype(np.float32)  # [x][x']
    cy = wy * ((iy[:, None] - iy[None, :]) ** 2).astype(np.float32)  # [y][y']
    cz = wz * ((iz[:, None] - iz[None, :]) ** 2).astype(np.float32)  # [z][z']
    gd, gk = np.empty((n, h, w), np.float32), np.empty((n, h, w), np.int64)
    for z in range(n):
        f = feat[z][:, None, :]  # [y][1][x']
        d = np.where(f, cx[None], np.float32(np.inf))  # [y][x][x']
        k = np.broadcast_to(np.where(f, lab[z][:, None, :].astype(np.int64), 0), d.shape)
        d1, k1 = lexmin(d, k, 2)  # [y][x]
        c = (d1[None, :, :] + cy[:, :, None]).astype(np.float32)  # [y][y'][x]
        gd[z], gk[z] = lexmin(c, np.broadcast_to(k1[None], c.shape), 1)
    od, ok = np.empty((n, h, w), np.float32), np.empty((n, h, w), np.int64)
    for z in range(n):
        c = (gd + cz[z][:, None, None]).astype(np.float32)  # [z'][y][x]
        od[z], ok[z] = lexmin(c, gk, 0)
    return od, ok.astype(np.uint8)


def r2_of(radius):
    return np.float32(float(radius) * float(radius))


def dilated(X, r2, spacing):
    return oracle_edt(X, spacing) <= r2


def eroded(X, r2, spacing):
    return X & ~(oracle_edt(~X, spacing) <= r2)  # (no background inside the volume: +inf, nothing erodes)


def oracle_morph(lab, op, radius, spacing=None, keep=None, into=(0,)):
    """-> (labels, (added, removed)) of lm_morph_dev, on the whole volume."""
    S, can, r2 = table(keep)[lab], table(into, 0)[lab], r2_of(radius)
    out = lab.copy()
    if op in ("dilate", "close"):
        d2, near = oracle_nearest(lab, keep, spacing)
        grown = (d2 <= r2) if op == "dilate" else eroded(dilated(S, r2, spacing), r2, spacing)
        m = grown & ~S & can
        out[m] = near[m]
        return out, (int(m.sum()), 0)
    m = S & ~(eroded(S, r2, spacing) if op == "erode" else dilated(eroded(S, r2, spacing), r2, spacing))
    out[m] = 0
    return out, (0, int(m.sum()))


def tie_volume(shape):
    """Mostly empty labels with exact ties, the LARGER label met first in search order (left / lower index first): two labels
    equidistant from a voxel along x, along y and along z, and a tie ACROSS passes -- label 7 at distance 2 in the voxel's own row,
    label 3 at distance 2 along the next axis, which an outward search that stops at `c >= best` never looks at.  -> (labels,
    [(voxel, expected label)])."""
    n, h, w = shape
    lab = np.zeros(shape, np.uint8)
    want = []
    if w >= 9:  # along x: 5 . . (v) . . 2
        lab[0, 0, 1], lab[0, 0, 7] = 5, 2
        want.append(((0, 0, 4), 2))
    if h >= 9:  # along y, in the last column
        lab[n - 1, 2, w - 1], lab[n - 1, 6, w - 1] = 6, 4
        want.append(((n - 1, 4, w - 1), 4))
    if n >= 9:  # along z, in the last row
        lab[2, h - 1, w // 2], lab[6, h - 1, w // 2] = 9, 8
        want.append(((4, h - 1, w // 2), 8))
    if h >= 9 and w >= 16:  # across x and y (w_y == w_x in two of the spacings): own row 7 at dx = 2, column 3 at dy = 2
        lab[0, 4, 14], lab[0, 6, 12] = 7, 3
        want.append(((0, 4, 12), 3))
    if n >= 9 and w >= 16:  # across x and z (unit spacing only)
        lab[n - 3, 0, 12], lab[n - 1, 0, 10] = 7, 3
        want.append(((n - 3, 0, 10), 3))
    return lab, want


def random_labels(rng, shape, n_labels=6, fill=0.3):
    """Blocky random labels 1 .. n_labels-1 (cells of 2 x 3 x 4 voxels), with holes and single voxels."""
    n, h, w = shape
    cs = ((n + 1) // 2, (h + 2) // 3, (w + 3) // 4)
    coarse = np.where(rng.random(cs) < fill, rng.integers(1, n_labels, cs), 0)
    lab = np.repeat(np.repeat(np.repeat(coarse, 2, 0), 3, 1), 4, 2)[:n, :h, :w].astype(np.uint8)
    lab[rng.random(shape) < 0.02] = 0
    spots = rng.random(shape) < 0.01
    lab[spots] = rng.integers(1, n_labels, int(spots.sum()))
    lab.flat[rng.choice(lab.size, 3, replace=False)] = (1, 2, 5)  # (never without the labels the keep subsets of the tests name)
    return lab


def radii(spacing):
    return (1.0, 2.0, np.sqrt(5.0)) if spacing is None else (0.8, 1.9, 3.2)


# ---------------------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_ties_and_distances():
    lab, want = tie_volume((9, 9, 20))
    d2, near = oracle_nearest(lab)
    assert len(want) == 5
    for v, k in want:
        assert near[v] == k, (v, near[v], k)
    assert np.array_equal(bits(d2), bits(oracle_edt(lab != 0)))
    rng = np.random.default_rng(1)
    lab = random_labels(rng, (4, 7, 9))
    d2, near = oracle_nearest(lab, keep=[2, 3], spacing=SPACINGS[2])
    assert np.array_equal(bits(d2), bits(oracle_edt(np.isin(lab, [2, 3]), SPACINGS[2])))
    assert np.all(np.isin(near, [2, 3])) and np.array_equal(near[np.isin(lab, [2, 3])], lab[np.isin(lab, [2, 3])])


def test_oracle_matches_scipy():
    """spacing None: d2 is an exact integer and the structuring element the ball {dz^2 + dy^2 + dx^2 <= r^2}."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    S = random_labels(rng, (6, 11, 13), fill=0.4) != 0
    S[0, :3, :3] = True  # (touches the border)
    for r in (1.0, 2.0, np.sqrt(5.0)):
        g = np.arange(-3, 4)
        ball = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= np.float32(r * r)
        lab = S.astype(np.uint8)
        dil = ndi.binary_dilation(S, ball)
        ero = ndi.binary_erosion(S, ball, border_value=1)
        assert np.array_equal(oracle_morph(lab, "dilate", r)[0] != 0, dil), r
        assert np.array_equal(oracle_morph(lab, "erode", r)[0] != 0, ero), r
        assert np.array_equal(oracle_morph(lab, "close", r)[0] != 0, ndi.binary_erosion(dil, ball, border_value=1)), r
        assert np.array_equal(oracle_morph(lab, "open", r)[0] != 0, ndi.binary_dilation(ero, ball)), r


# ---------------------------------------------------------------------------------------------------------- nearest-label transform
def check_nearest(eng, lab, keep, spacing, what):
    near, d2 = eng.nearest_label(lab, spacing, keep, return_distance=True)
    wd, wn = oracle_nearest(lab, keep, spacing)
    assert near.dtype == np.uint8 and d2.dtype == np.float32 and near.shape == d2.shape == lab.shape
    assert np.array_equal(bits(d2), bits(wd)), what
    assert np.array_equal(bits(d2), bits(eng.edt(table(keep)[lab].astype(np.uint8), spacing))), what
    assert np.array_equal(near, wn), (what, np.argwhere(near != wn)[:5])
    assert np.array_equal(eng.nearest_label(lab, spacing, keep), wn), what  # (d2_out_dev NULL: the distances in the workspace)
    return near


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_nearest_label(emu_engine, shape, spacing):
    lab, want = tie_volume(shape)
    near = check_nearest(emu_engine, lab, None, spacing, "ties")
    ties = 0
    for v, k in want:
        if oracle_nearest(lab, None, spacing)[1][v] == k:
            assert near[v] == k
            ties += 1
    assert ties >= (1 if max(shape) >= 9 else 0)
    rng = np.random.default_rng(sum(shape))
    lab = random_labels(rng, shape)
    check_nearest(emu_engine, lab, None, spacing, "random")
    check_nearest(emu_engine, lab, [2, 5], spacing, "labels outside keep")


def test_nearest_label_tie_voxels_unit_spacing(emu_engine):
    """Every tie of tie_volume, the cross-pass ones included, is exact with unit spacing and resolves to the smaller label."""
    lab, want = tie_volume((9, 9, 70))
    near = emu_engine.nearest_label(lab)
    assert len(want) == 5
    for v, k in want:
        assert near[v] == k, (v, near[v], k)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_nearest_label_feature_sets(emu_engine, spacing):
    shape = (5, 9, 70)
    near, d2 = emu_engine.nearest_label(np.zeros(shape, np.uint8), spacing, return_distance=True)
    assert np.all(np.isposinf(d2)) and not near.any()
    lab = np.full(shape, 4, np.uint8)  # labels, but none of them kept
    near, d2 = emu_engine.nearest_label(lab, spacing, keep=[1], return_distance=True)
    assert np.all(np.isposinf(d2)) and not near.any()
    one = np.zeros(shape, np.uint8)
    one[4, 0, 66] = 9
    check_nearest(emu_engine, one, None, spacing, "one")
    assert np.all(emu_engine.nearest_label(one, spacing) == 9)
    check_nearest(emu_engine, np.full(shape, 3, np.uint8), None, spacing, "all")


@pytest.mark.parametrize("spacing", WORD_SPACINGS)
def test_nearest_label_word_boundaries(emu_engine, spacing):
    lab = word_boundary_rows((5, 2, 7, 3))
    near = check_nearest(emu_engine, lab, None, spacing, "word boundaries")
    if spacing is not None:  # the x pass alone
        assert np.all(near[0, 0] == 5) and np.all(near[0, 1] == 3) and np.all(near[0, 2] == 2) and np.all(near[1, 0] == 7)


def test_nearest_label_invalid_arguments(emu_engine):
    lab = np.zeros((2, 4, 4), np.uint8)
    for sp in ((1.0, 0.0, 1.0), (np.nan, 1.0, 1.0), (np.inf, 1.0, 1.0)):
        with pytest.raises(nat.LMError, match="lm_nearest_label_dev"):
            emu_engine.nearest_label(lab, sp)
    with pytest.raises(nat.LMError):
        emu_engine.nearest_label(lab, (1.0, 1.0))
    with pytest.raises(ValueError):
        emu_engine.nearest_label(lab, keep=[0])
    lib = emu_engine.L.lib
    keep = nat.Engine._keep_table(None)
    for n, h, w in ((2048, 1024, 1024), (2, 4097, 4)):  # refused before anything is read (the pointers are not valid)
        assert lib.lm_nearest_label_dev(emu_engine.h, 8, n, h, w, keep, None, None, 16) < 0
    ld = emu_engine.to_device(lab)
    assert lib.lm_nearest_label_dev(emu_engine.h, ld.ptr, 2, 4, 4, keep, None, None, ld.ptr) < 0  # near_out_dev == lab_dev
    ld.free()


# ---------------------------------------------------------------------------------------------------------- the operators
def check_op(eng, lab, op, radius, spacing, keep, into, what):
    got, changed = eng.morph(lab, op, radius, spacing=spacing, keep=keep, into=into)
    want, wchanged = oracle_morph(lab, op, radius, spacing, keep, into)
    assert np.array_equal(got, want), (what, op, radius, np.argwhere(got != want)[:5])
    assert changed == wchanged, (what, op, radius, changed, wchanged)
    return got


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_operators(emu_engine, shape, spacing):
    rng = np.random.default_rng(100 + sum(shape))
    ties, _ = tie_volume(shape)
    lab = random_labels(rng, shape)
    for op in OPS:
        for r in radii(spacing):
            if ties.any():
                check_op(emu_engine, ties, op, r, spacing, None, (0,), "ties")
            check_op(emu_engine, lab, op, r, spacing, None, (0,), "random")
        check_op(emu_engine, lab, op, radii(spacing)[1], spacing, [2, 5], (0,), "labels outside keep")
        check_op(emu_engine, lab, op, radii(spacing)[1], spacing, [2, 5], (0, 1, 3), "into may overwrite 1 and 3")
        check_op(emu_engine, lab, op, radii(spacing)[2], spacing, [1, 2, 3], (4,), "into protects 0")


@pytest.mark.parametrize("spacing", SPACINGS)
def test_operator_properties(emu_engine, spacing):
    """Closing is extensive and idempotent, opening anti-extensive and idempotent; radius 0 is the identity."""
    rng = np.random.default_rng(7)
    lab = random_labels(rng, (5, 9, 70), fill=0.4)
    lab[:, :, 10:40] = np.where(rng.random((5, 9, 30)) < 0.03, 0, 3)  # (a slab with pinholes that survives every opening here)
    everything = tuple(range(256))
    for r in radii(spacing):
        closed, (added, removed) = emu_engine.morph(lab, "close", r, spacing=spacing)
        assert removed == 0 and np.array_equal(closed[lab != 0], lab[lab != 0]) and added == int(((closed != 0) & (lab == 0)).sum())
        again, changed = emu_engine.morph(closed, "close", r, spacing=spacing)
        assert changed == (0, 0) and np.array_equal(again, closed)
        opened, (added, removed) = emu_engine.morph(lab, "open", r, spacing=spacing)
        assert added == 0 and np.all((opened == lab) | (opened == 0)) and removed == int((opened != lab).sum())
        assert opened.any() and removed > 0
        again, changed = emu_engine.morph(opened, "open", r, spacing=spacing)
        assert changed == (0, 0) and np.array_equal(again, opened)
    for op in OPS:
        same, changed = emu_engine.morph(lab, op, 0.0, spacing=spacing, into=everything)
        assert changed == (0, 0) and np.array_equal(same, lab), op


@pytest.mark.parametrize("spacing", SPACINGS)
def test_propagation(emu_engine, spacing):
    """radius +inf: every `into` voxel takes the nearest kept label."""
    rng = np.random.default_rng(8)
    lab = random_labels(rng, (5, 9, 70))
    for keep, into in ((None, (0,)), ([2, 5], (0, 1)), ([1, 2], (3,))):
        got, (added, removed) = emu_engine.morph(lab, "dilate", np.inf, spacing=spacing, keep=keep, into=into)
        near = oracle_nearest(lab, keep, spacing)[1]
        m = np.isin(lab, into) & ~table(keep)[lab]
        want = np.where(m, near, lab)
        assert np.array_equal(got, want) and (added, removed) == (int(m.sum()), 0)
    for op in ("erode", "open", "close"):
        with pytest.raises(ValueError):
            emu_engine.morph(lab, op, np.inf)


def test_in_place_equals_out_of_place(emu_engine):
    rng = np.random.default_rng(9)
    lab = random_labels(rng, (5, 9, 70))
    for op in OPS:
        ld = emu_engine.to_device(lab)
        out, changed = emu_engine.morph_dev(ld, op, 2.0, spacing=SPACINGS[2])
        emu_engine.sync()
        assert out is not ld and np.array_equal(ld.download(), lab)  # (the input is left alone)
        res = out.download()
        out2, changed2 = emu_engine.morph_dev(ld, op, 2.0, spacing=SPACINGS[2], out=ld)
        emu_engine.sync()
        assert out2 is ld and changed2 == changed and np.array_equal(ld.download(), res), op
        assert np.array_equal(res, oracle_morph(lab, op, 2.0, SPACINGS[2])[0]), op
        ld.free()
        out.free()


@pytest.mark.parametrize("spacing", SPACINGS)
def test_box_confinement(emu_engine, spacing):
    """The device works inside the grown box of the selection, the oracle on the whole volume: a selection far from every border (a
    box much smaller than the volume), one in a corner (the box clipped on three sides) and one touching opposite borders."""
    shape = (12, 30, 40)
    rng = np.random.default_rng(10)
    inner = np.zeros(shape, np.uint8)
    inner[5:8, 12:18, 15:24] = random_labels(rng, (3, 6, 9), fill=0.7)
    inner[0, 0, 0] = 7  # (another label far away: it is not selected, and `into` protects it)
    corner = np.zeros(shape, np.uint8)
    corner[:3, :6, :9] = random_labels(rng, (3, 6, 9), fill=0.7)
    across = np.zeros(shape, np.uint8)
    across[4:7, :, 18:22] = random_labels(rng, (3, 30, 4), fill=0.8)
    for what, lab in (("inner", inner), ("corner", corner), ("across", across)):
        for op in OPS:
            for r in radii(spacing)[1:]:
                check_op(emu_engine, lab, op, r, spacing, [1, 2, 3, 4, 5], (0,), what)


def test_operators_match_scipy(emu_engine):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    S = random_labels(rng, (5, 9, 70), fill=0.4) != 0
    lab = S.astype(np.uint8)
    g = np.arange(-3, 4)
    for r in (1.0, 2.0, np.sqrt(5.0)):
        ball = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= np.float32(r * r)
        dil = ndi.binary_dilation(S, ball)
        ero = ndi.binary_erosion(S, ball, border_value=1)
        assert np.array_equal(emu_engine.morph(lab, "dilate", r)[0] != 0, dil), r
        assert np.array_equal(emu_engine.morph(lab, "erode", r)[0] != 0, ero), r
        assert np.array_equal(emu_engine.morph(lab, "close", r)[0] != 0, ndi.binary_erosion(dil, ball, border_value=1)), r
        assert np.array_equal(emu_engine.morph(lab, "open", r)[0] != 0, ndi.binary_dilation(ero, ball)), r


def test_morph_invalid_arguments(emu_engine):
    import ctypes as C

    lab = np.zeros((2, 4, 5), np.uint8)
    lab[1, 2, 3] = 4
    with pytest.raises(ValueError, match="no voxel"):
        emu_engine.morph(np.zeros((2, 4, 5), np.uint8), "close", 1.0)
    with pytest.raises(ValueError, match="no voxel"):
        emu_engine.morph(lab, "close", 1.0, keep=[1])
    with pytest.raises(ValueError):
        emu_engine.morph(lab, "shrink", 1.0)
    for r in (-1.0, np.nan):
        with pytest.raises(ValueError):
            emu_engine.morph(lab, "dilate", r)
    with pytest.raises(ValueError):
        emu_engine.morph(lab, "dilate", 1.0, into=[256])
    with pytest.raises(nat.LMError, match="lm_morph_dev"):
        emu_engine.morph(lab, "dilate", 1.0, spacing=(1.0, 0.0, 1.0))
    lib = emu_engine.L.lib
    ld = emu_engine.to_device(lab)
    p = nat.MorphParams()
    p.op, p.radius_mm = 3, 1.0
    p.spacing[:] = [1.0, 1.0, 1.0]
    C.memmove(p.keep, nat.Engine._keep_table(None), 256)
    changed = (C.c_int64 * 2)()
    assert lib.lm_morph_dev(emu_engine.h, ld.ptr, 2, 4, 5, C.byref(p), ld.ptr, changed) == 0
    p.op = 4
    assert lib.lm_morph_dev(emu_engine.h, ld.ptr, 2, 4, 5, C.byref(p), ld.ptr, changed) < 0
    p.op, p.radius_mm = 3, float("inf")
    assert lib.lm_morph_dev(emu_engine.h, ld.ptr, 2, 4, 5, C.byref(p), ld.ptr, changed) < 0
    p.radius_mm = 1.0
    for n, h, w in ((2048, 1024, 1024), (2, 4097, 4)):  # refused before anything is read (the pointers are not valid)
        assert lib.lm_morph_dev(emu_engine.h, 8, n, h, w, C.byref(p), 8, changed) < 0
    ld.free()
