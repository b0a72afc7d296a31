"""Connected components and their table (lm_components_dev, lm_component_table_dev, lm_relabel_dev) on the g++ emulation of the kernel
sources, bit for bit against a numpy oracle that applies the definitions of include/lungmask_hip.h literally: a union-find by minimum
propagation over the edges between selected voxels of equal key, numbered by the first raster voxel, and table rows grouped by id.
`check_components` is shared with the GPU suite (tests/test_gpu_components.py)."""
import ctypes as C

import numpy as np
import pytest

from lungmask_amd import _native as nat

try:
    from scipy import ndimage
except ImportError:  # the oracle below stands alone
    ndimage = None

SHAPES = [(1, 1, 70), (1, 40, 130), (5, 33, 70), (3, 7, 600), (24, 90, 136)]
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def oracle_hu(image):
    """(hu int64, nonfinite bool) of a volume: lm_label_stats_dev's HU value."""
    image = np.asarray(image)
    if image.dtype.kind == "f":
        nan = np.isnan(image)
        r = np.rint(np.where(nan, 0, image))  # half to even, in the volume's own precision
        hu = np.where(r >= 2147483648.0, INT_MAX, np.where(r < -2147483648.0, INT_MIN, r)).astype(np.int64)
        hu = np.where(r >= 2147483648.0, INT_MAX, hu)  # (the float -> int of the saturated values above is the clipped one)
        return np.where(nan, 0, hu), nan
    return np.clip(image.astype(np.int64), INT_MIN, INT_MAX), np.zeros(image.shape, bool)


def keep_table(keep):
    t = np.zeros(256, bool)
    if keep is None:
        t[1:] = True
    else:
        t[list(keep)] = True
    return t


def oracle_select(labels, image=None, hu_range=None, keep=None, per_label=True):
    """(key uint8 volume, counts int64 [3][256])."""
    labels = np.asarray(labels, np.uint8)
    sel = keep_table(keep)[labels]
    nan = np.zeros(labels.shape, bool)
    if image is not None:
        hu, nan = oracle_hu(image)
        lo, hi = (None, None) if hu_range is None else hu_range
        sel = sel & ~nan
        if lo is not None:
            sel = sel & (hu >= lo)
        if hi is not None:
            sel = sel & (hu <= hi)
    counts = np.zeros((3, 256), np.int64)
    counts[0] = np.bincount(labels.ravel(), minlength=256)
    counts[1] = np.bincount(labels[nan], minlength=256)
    counts[2] = np.bincount(labels[sel], minlength=256)
    return np.where(sel, labels if per_label else 1, 0).astype(np.uint8), counts


def offsets(connectivity):
    """The raster-later half of the neighbourhood."""
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]
    return [o for o in offs if connectivity == 26 or sum(abs(c) for c in o) == 1]


def oracle_label(key, connectivity=6):
    """(ids int32, T): union-find over the edges between adjacent voxels of equal non-zero key.  L[v] is always a voxel of v's component
    with an index <= v, so pointer jumping (L = L[L]) is valid; at the fixed point it is the component's first voxel."""
    n, h, w = key.shape
    flat = np.arange(key.size, dtype=np.int64).reshape(key.shape)
    ea, eb = [], []
    for dz, dy, dx in offsets(connectivity):
        za, zb = slice(max(0, -dz), n - max(0, dz)), slice(max(0, dz), n - max(0, -dz))
        ya, yb = slice(max(0, -dy), h - max(0, dy)), slice(max(0, dy), h - max(0, -dy))
        xa, xb = slice(max(0, -dx), w - max(0, dx)), slice(max(0, dx), w - max(0, -dx))
        m = (key[za, ya, xa] != 0) & (key[za, ya, xa] == key[zb, yb, xb])
        ea.append(flat[za, ya, xa][m])
        eb.append(flat[zb, yb, xb][m])
    a, b = np.concatenate(ea), np.concatenate(eb)
    L = np.arange(key.size, dtype=np.int64)
    while True:
        m = np.minimum(L[a], L[b])
        new = L.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, L):
            break
        L = new
    sel = key.ravel() != 0
    roots = np.unique(L[sel])  # ascending: the raster order of the first voxels
    ids = np.zeros(key.size, np.int32)
    ids[sel] = np.searchsorted(roots, L[sel]) + 1
    return ids.reshape(key.shape), int(roots.size)


def oracle_table(ids, labels, image=None):
    """The rows 1 .. max(ids) as a record array of nat.COMPONENT_DTYPE."""
    ids = np.asarray(ids)
    T = int(ids.max()) if ids.size else 0
    rows = np.zeros(T, nat.COMPONENT_DTYPE)
    rows["bbox"] = -1
    rows["first"] = -1
    if T == 0:
        return rows
    n, h, w = ids.shape
    sel = ids > 0
    g = ids[sel].astype(np.int64) - 1
    z, y, x = (c[sel] for c in np.indices(ids.shape))
    flat = np.arange(ids.size).reshape(ids.shape)[sel]
    rows["voxels"] = np.bincount(g, minlength=T)
    for k, c in enumerate((z, y, x)):
        s = np.zeros(T, np.int64)
        np.add.at(s, g, c)
        rows["index_sum"][:, k] = s
        lo, hi = np.full(T, INT_MAX, np.int64), np.full(T, -1, np.int64)
        np.minimum.at(lo, g, c)
        np.maximum.at(hi, g, c)
        rows["bbox"][:, 2 * k] = lo
        rows["bbox"][:, 2 * k + 1] = hi + 1
    first = np.full(T, INT_MAX, np.int64)
    np.minimum.at(first, g, flat)
    rows["first"] = first
    rows["label"] = np.asarray(labels, np.uint8).ravel()[first]
    pad = np.pad(ids, 1)  # outside the volume: no component
    core = (slice(1, -1),) * 3
    for k in range(3):
        lo_side = tuple(slice(0, -2) if a == k else slice(1, -1) for a in range(3))
        hi_side = tuple(slice(2, None) if a == k else slice(1, -1) for a in range(3))
        f = (pad[lo_side] != pad[core]).astype(np.int64) + (pad[hi_side] != pad[core])
        s = np.zeros(T, np.int64)
        np.add.at(s, g, f[sel])
        rows["faces"][:, k] = s
    if image is not None:
        hu, nan = oracle_hu(image)
        ok = ~nan[sel]
        s = np.zeros(T, np.int64)
        np.add.at(s, g[ok], hu[sel][ok])
        rows["hu_sum"] = s
        lo, hi = np.full(T, INT_MAX, np.int64), np.full(T, INT_MIN, np.int64)
        np.minimum.at(lo, g[ok], hu[sel][ok])
        np.maximum.at(hi, g[ok], hu[sel][ok])
        none = lo > hi
        rows["hu_min"] = np.where(none, 0, lo)
        rows["hu_max"] = np.where(none, 0, hi)
    return rows


def oracle_components(labels, image=None, hu_range=None, keep=None, per_label=True, connectivity=6):
    key, counts = oracle_select(labels, image, hu_range, keep, per_label)
    ids, T = oracle_label(key, connectivity)
    return ids, T, counts, oracle_table(ids, labels, image), key


def assert_rows_equal(got, want):
    assert got.shape == want.shape
    for f in nat.COMPONENT_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (f, got[f][:8], want[f][:8])


def check_components(engine, image, labels, **kw):
    """Engine.components against the oracle: ids, total, counts and every table field, for equality.  -> (ids, T, rows)."""
    labels = np.asarray(labels, np.uint8)
    ids, T, counts, rows = engine.components(labels, image, **kw)
    oids, oT, ocounts, orows, key = oracle_components(labels, image, **kw)
    assert T == oT
    assert ids.dtype == np.int32 and np.array_equal(ids, oids)
    assert np.array_equal(counts, ocounts)
    assert_rows_equal(rows, orows)
    if ndimage is not None and len(np.unique(key)) <= 2:  # a binary selection: scipy's numbering
        full = kw.get("connectivity", 6) == 26
        assert np.array_equal(ids, ndimage.label(key != 0, structure=np.ones((3, 3, 3)) if full else None)[0])
    return ids, T, rows


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def random_case(shape, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 7, shape).astype(np.uint8)
    image = rng.integers(-1100, 200, shape).astype(np.int16)
    return labels, image


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return (((z + y + x) & 1) == 0).astype(np.uint8)


def serpentine(shape):
    """A one-voxel-wide path through the volume: the even rows of the even slices, joined at alternating ends."""
    n, h, w = shape
    lab = np.zeros(shape, np.uint8)
    end = w - 1
    for z in range(0, n, 2):
        ys = range(h) if (z // 2) % 2 == 0 else range(h - 1, -1, -1)
        last = None
        for y in ys:
            if y % 2 == 0:
                lab[z, y, :] = 1
                end = 0 if end == w - 1 else w - 1  # the path leaves this row at the other end
                last = y
            else:
                lab[z, y, end] = 1
        if z + 1 < n:
            lab[z + 1, last, end] = 1
    return lab


# ---- the oracle itself --------------------------------------------------------------------------------------------------------------
def test_oracle_against_direct_masking():
    labels, image = random_case((4, 9, 11), 5)
    ids, T, _, rows, _ = oracle_components(labels, image, hu_range=(-900, 0))
    assert T > 3
    seen = 0
    for i in range(1, T + 1):
        m = ids == i
        zz, yy, xx = np.nonzero(m)
        r = rows[i - 1]
        assert r["voxels"] == m.sum() and np.flatnonzero(m)[0] == r["first"] > seen - 1
        seen = r["first"] + 1  # numbered by the first raster voxel
        assert list(r["bbox"]) == [zz.min(), zz.max() + 1, yy.min(), yy.max() + 1, xx.min(), xx.max() + 1]
        assert list(r["index_sum"]) == [zz.sum(), yy.sum(), xx.sum()]
        assert r["hu_sum"] == image[m].astype(np.int64).sum() and r["hu_min"] == image[m].min() and r["hu_max"] == image[m].max()
        assert r["label"] == labels[m][0] and (labels[m] == r["label"]).all()
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 1, 1] = 1
    assert list(oracle_table(one.astype(np.int32), one)["faces"][0]) == [2, 2, 2]
    box = np.ones((2, 3, 4), np.uint8)
    assert list(oracle_table(box.astype(np.int32), box)["faces"][0]) == [2 * 12, 2 * 8, 2 * 6]  # border faces count


def test_serpentine_is_one_wide_path():
    lab = serpentine((5, 33, 70))
    assert oracle_label(lab, 6)[1] == 1 and lab.sum() > 3 * 17 * 70


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("hu_range", [(-950, -200), (None, -951), (-300, None), None])
def test_random_labels(emu_engine, shape, hu_range):
    labels, image = random_case(shape, sum(shape))
    _, T, _ = check_components(emu_engine, image, labels, hu_range=hu_range)
    assert T > 0


@pytest.mark.parametrize("shape", SHAPES[:4])
def test_random_labels_without_image_and_26(emu_engine, shape):
    labels, image = random_case(shape, 3)
    ids, _, rows = check_components(emu_engine, None, labels)
    assert not rows["hu_sum"].any() and not rows["hu_min"].any() and not rows["hu_max"].any()
    check_components(emu_engine, None, labels, connectivity=26)
    check_components(emu_engine, image, labels, hu_range=(-700, None), connectivity=26, per_label=False)
    check_components(emu_engine, image, labels, hu_range=(-700, None), per_label=False)


def raw_table(engine, ids, labels, image, cap, extra=5):
    """lm_component_table_dev into a sentinel-filled buffer of cap + extra rows -> (buffer, total)."""
    buf = np.full((cap + extra) * nat.COMPONENT_DTYPE.itemsize, 0x5A, np.uint8)
    total = C.c_int64()
    d_ids, d_lab = engine.to_device(ids), engine.to_device(labels)
    d_img = engine.to_device(image) if image is not None else None
    try:
        n, h, w = ids.shape
        engine.L.check(engine.L.lib.lm_component_table_dev(engine.h, d_ids.ptr, d_lab.ptr, d_img.ptr if d_img is not None else None,
                                                           nat.LM_DTYPES[image.dtype] if image is not None else 0, n, h, w, buf.ctypes.data, cap,
                                                           C.byref(total)), "lm_component_table_dev")
    finally:
        for d in (d_ids, d_lab, d_img):
            if d is not None:
                d.free()
    return buf.view(nat.COMPONENT_DTYPE), int(total.value)


def test_checkerboard_6_every_voxel_alone_and_cap(emu_engine):
    shape = (5, 33, 70)
    labels = checkerboard(shape)
    image = random_case(shape, 1)[1]
    ids, T, rows = check_components(emu_engine, image, labels)
    assert T == labels.sum() == (labels.size + 1) // 2 and (rows["voxels"] == 1).all()
    assert emu_engine.component_table_launch(labels.size)[1] // 2 > 256  # more components per workgroup than hash slots: the bypass runs
    want = oracle_table(ids, labels, image)
    for cap in (100, T - 1, T, 100000):
        got, total = raw_table(emu_engine, ids, labels, image, cap)
        k = min(cap, T)
        assert total == T
        assert_rows_equal(got[:k], want[:k])
        assert (got[k:].view(np.uint8) == 0x5A).all()  # nothing beyond min(T, cap) is written
    got, total = raw_table(emu_engine, ids, labels, image, 0)
    assert total == T and (got.view(np.uint8) == 0x5A).all()


def test_checkerboard_26_is_one_component(emu_engine):
    _, T, rows = check_components(emu_engine, None, checkerboard((5, 33, 70)), connectivity=26)
    assert T == 1 and rows["voxels"][0] == (5 * 33 * 70 + 1) // 2


def test_full_volume_one_component_over_several_workgroups(emu_engine):
    shape = SHAPES[4]
    labels = np.full(shape, 3, np.uint8)
    image = random_case(shape, 2)[1]
    _, T, rows = check_components(emu_engine, image, labels)
    groups, per = emu_engine.component_table_launch(labels.size)
    assert T == 1 and rows["voxels"][0] == labels.size
    assert groups >= 2 and per < labels.size and (groups - 1) * per < labels.size <= groups * per  # the launch splits it
    assert list(rows["faces"][0]) == [2 * 90 * 136, 2 * 24 * 136, 2 * 24 * 90]


def test_serpentine(emu_engine):
    lab = serpentine((5, 33, 70))
    _, T, _ = check_components(emu_engine, None, lab)
    assert T == 1
    two = lab.copy()
    two[2, 16, :] = 0  # cut in the middle
    assert check_components(emu_engine, None, two)[1] >= 2


def test_labels_touching_face_to_face(emu_engine):
    labels = np.zeros((3, 7, 600), np.uint8)
    labels[1, 2:5, 10:300] = 1
    labels[1, 2:5, 300:590] = 2
    assert check_components(emu_engine, None, labels, per_label=True)[1] == 2
    ids, T, rows = check_components(emu_engine, None, labels, per_label=False)
    assert T == 1 and rows["label"][0] == 1  # the label of the first voxel


def test_corner_contact(emu_engine):
    labels = np.zeros((5, 33, 70), np.uint8)
    labels[1, 4, 63] = labels[2, 5, 64] = 1  # across a 64-voxel segment border as well
    assert check_components(emu_engine, None, labels, connectivity=6)[1] == 2
    assert check_components(emu_engine, None, labels, connectivity=26)[1] == 1


def test_float_image_nan_inf_half(emu_engine):
    shape = (5, 33, 70)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 3, shape).astype(np.uint8)
    image = (rng.integers(-2000, 400, shape) / 2).astype(np.float32)  # exact .5 values
    flat = image.ravel()
    flat[rng.choice(flat.size, 300, replace=False)] = np.nan
    flat[rng.choice(flat.size, 100, replace=False)] = np.inf
    flat[rng.choice(flat.size, 100, replace=False)] = -np.inf
    assert oracle_hu(np.float32([0.5, 1.5, 2.5, -0.5, np.inf, -np.inf, 3e9]))[0].tolist() == [0, 2, 2, 0, INT_MAX, INT_MIN, INT_MAX]
    for hu_range in ((-950, -200), (None, -500), (-500, None), None):
        _, _, rows = check_components(emu_engine, image, labels, hu_range=hu_range)
    assert rows["hu_max"].max() == INT_MAX and rows["hu_min"].min() == INT_MIN  # the open range selects +-inf, saturated
    check_components(emu_engine, image.astype(np.float64), labels, hu_range=(-950, -200))


def test_int32_extremes_over_a_large_component(emu_engine):
    shape = (5, 33, 70)
    labels = np.ones(shape, np.uint8)
    image = np.full(shape, INT_MAX, np.int32)
    image[3:] = INT_MIN
    image[2, 5, 7] = 0
    _, T, rows = check_components(emu_engine, image, labels)
    assert T == 1 and rows["hu_min"][0] == INT_MIN and rows["hu_max"][0] == INT_MAX
    assert rows["hu_sum"][0] == (3 * 33 * 70 - 1) * INT_MAX + 2 * 33 * 70 * INT_MIN
    big = np.full(shape, INT_MAX, np.int32)
    assert check_components(emu_engine, big, labels)[2]["hu_sum"][0] == labels.size * INT_MAX  # far beyond 32 bits
    check_components(emu_engine, big.astype(np.int64) * 8, labels, hu_range=(0, None))  # int64: saturated to int32


def test_keep(emu_engine):
    labels, image = random_case((5, 33, 70), 4)
    ids, _, rows = check_components(emu_engine, image, labels, keep=(2, 5), hu_range=(None, -300))
    assert set(np.unique(labels[ids > 0])) <= {2, 5} and set(rows["label"]) <= {2, 5}
    check_components(emu_engine, None, labels, keep=(6,), per_label=False)


def test_empty_selection(emu_engine):
    labels, image = random_case((5, 33, 70), 6)
    for kw in (dict(hu_range=(5000, None)), dict(keep=(9,))):
        ids, T, rows = check_components(emu_engine, image, labels, **kw)
        assert T == 0 and not ids.any() and rows.shape == (0,)
    ids, T, counts, rows = emu_engine.components(np.zeros((0, 4, 4), np.uint8))
    assert T == 0 and ids.shape == (0, 4, 4) and not counts.any()


def test_argument_errors(emu_engine):
    labels, image = random_case((2, 5, 9), 1)
    with pytest.raises(ValueError):
        emu_engine.components(labels, image, connectivity=18)
    with pytest.raises(ValueError):
        emu_engine.components(labels, image, hu_range=(10, -10))
    with pytest.raises(ValueError):
        emu_engine.components(labels, None, hu_range=(None, -950))
    with pytest.raises(nat.LMError):
        emu_engine.components(labels, image[:, :, :5])
    p = nat.ComponentsParams()
    p.connectivity = 18
    total, counts = C.c_int64(), np.zeros((3, 256), np.int64)
    assert emu_engine.L.lib.lm_components_dev(emu_engine.h, None, None, 0, 0, 5, 9, C.byref(p), None, C.byref(total), counts.ctypes.data) == -1
    assert b"connectivity" in emu_engine.L.lib.lm_last_error()


# ---- lm_relabel_dev -----------------------------------------------------------------------------------------------------------------
def test_relabel(emu_engine):
    labels, image = random_case((5, 33, 70), 8)
    ids, T, rows = check_components(emu_engine, image, labels, hu_range=(None, -600))
    rng = np.random.default_rng(0)
    lut = np.concatenate([[0], rng.permutation(T) + 1]).astype(np.int32)
    d = emu_engine.to_device(ids)
    try:
        out = emu_engine.relabel_dev(d, lut)
        assert np.array_equal(out.download(), lut[ids]) and np.array_equal(d.download(), ids)
        out.free()
        assert emu_engine.relabel_dev(d, lut, out=d) is d  # in place
        assert np.array_equal(d.download(), lut[ids])
        d.upload(ids)
        keep = rows["voxels"] >= 3  # min_voxels compaction
        lut2 = np.zeros(T + 1, np.int32)
        lut2[1:][keep] = np.arange(1, keep.sum() + 1)
        emu_engine.relabel_dev(d, lut2, out=d)
        got = d.download()
        assert np.array_equal(got, lut2[ids]) and got.max() == keep.sum()
        d.upload(ids)
        with pytest.raises(nat.LMError, match="outside the table"):  # a clean error, no out-of-bounds read
            emu_engine.relabel_dev(d, lut[:T], out=d)
        short = d.download()
        assert np.array_equal(short, np.where(ids < T, lut[np.minimum(ids, T - 1)], 0))
        d.upload(np.where(ids == 1, -7, ids).astype(np.int32))
        with pytest.raises(nat.LMError, match="outside the table"):
            emu_engine.relabel_dev(d, lut, out=d)
    finally:
        d.free()
