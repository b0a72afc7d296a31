"""Texture matrices (lm_texture_dev, Engine.texture) on the g++ emulation of the kernel sources, against a numpy restatement of the
Semantics of include/lungmask_hip.h: every matrix and every count compared with np.array_equal on int64, no tolerances.  Every
matrix test also asserts that the labels it means to test have non-zero totals, so that an empty result cannot pass."""
import numpy as np
import pytest

from lungmask_amd import _native as nat
from tests.test_stats_emu import oracle_hu

DIRS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]
COUNTS = ("voxels", "valid", "nonfinite", "below", "above", "longest_run")


def oracle_codes(lab, vol, n_labels, lo, hi, bin_width):
    """(code int64 [n][h][w]: 0 = takes no part, else 1 + label * 64 + level; the per-label counts without longest_run)."""
    hu, nan = oracle_hu(vol)
    lab = np.where(lab < n_labels, lab, 0).astype(np.int64)
    valid = (lab > 0) & ~nan & (hu >= lo) & (hu <= hi)
    level = np.where(valid, (hu - lo) // bin_width, 0)  # (hu - lo >= 0 where it counts: floor == truncation)
    counts = {f: np.zeros(n_labels, np.int64) for f in COUNTS}
    for k in range(1, n_labels):
        m = lab == k
        counts["voxels"][k] = m.sum()
        counts["valid"][k] = (m & valid).sum()
        counts["nonfinite"][k] = (m & nan).sum()
        counts["below"][k] = (m & ~nan & (hu < lo)).sum()
        counts["above"][k] = (m & ~nan & (hu > hi)).sum()
    return np.where(valid, 1 + lab * 64 + level, 0), counts


def _shifted(n, o):
    """Slices (p, q) along an axis of length n such that q = p + o, both inside."""
    return slice(max(0, -o), max(0, n - max(0, o))), slice(max(0, o), max(0, n - max(0, -o)))


def oracle_glcm(code, n_labels, ng, distance):
    out = np.zeros((n_labels, 13, ng, ng), np.int64)
    for d, off in enumerate(DIRS):
        sl = [_shifted(n, distance * o) for n, o in zip(code.shape, off)]
        p, q = code[tuple(s[0] for s in sl)], code[tuple(s[1] for s in sl)]
        m = (p > 0) & (q > 0) & ((p - 1) // 64 == (q - 1) // 64)
        np.add.at(out, ((p[m] - 1) // 64, d, (p[m] - 1) % 64, (q[m] - 1) % 64), 1)
    return out


def run_lengths(code, off):
    """(code of the first voxel, length) of every run along `off`: the starts walk forward together until none continues."""
    shape = np.array(code.shape)
    pos = np.argwhere(code > 0)
    prev = pos - off
    inside = ((prev >= 0) & (prev < shape)).all(axis=1)
    cont = np.zeros(len(pos), bool)
    cont[inside] = code[tuple(prev[inside].T)] == code[tuple(pos[inside].T)]
    pos = pos[~cont]
    c0 = code[tuple(pos.T)]
    length = np.ones(len(pos), np.int64)
    alive = np.arange(len(pos))
    while alive.size:
        pos[alive] += off
        cur = pos[alive]
        ok = ((cur >= 0) & (cur < shape)).all(axis=1)
        ok[ok] = code[tuple(cur[ok].T)] == c0[alive[ok]]
        alive = alive[ok]
        length[alive] += 1
    return c0, length


def run_lengths_python(code, off):
    """The same by a plain walk, voxel by voxel (small volumes only)."""
    n, h, w = code.shape
    inside = lambda z, y, x: 0 <= z < n and 0 <= y < h and 0 <= x < w
    c0, length = [], []
    for z in range(n):
        for y in range(h):
            for x in range(w):
                c = code[z, y, x]
                if c == 0:
                    continue
                pz, py, px = z - off[0], y - off[1], x - off[2]
                if inside(pz, py, px) and code[pz, py, px] == c:
                    continue
                r, (qz, qy, qx) = 1, (z + off[0], y + off[1], x + off[2])
                while inside(qz, qy, qx) and code[qz, qy, qx] == c:
                    r, (qz, qy, qx) = r + 1, (qz + off[0], qy + off[1], qx + off[2])
                c0.append(c)
                length.append(r)
    return np.array(c0, np.int64), np.array(length, np.int64)


def oracle_glrlm(code, n_labels, ng, walk=run_lengths):
    """(unclamped glrlm [n_labels][13][ng][longest run, at least 1], longest_run [n_labels])."""
    runs = [walk(code, np.array(off)) for off in DIRS]
    cols = max([1] + [int(r.max()) for _, r in runs if r.size])
    out = np.zeros((n_labels, 13, ng, cols), np.int64)
    longest = np.zeros(n_labels, np.int64)
    for d, (c0, r) in enumerate(runs):
        np.add.at(out, ((c0 - 1) // 64, d, (c0 - 1) % 64, r - 1), 1)
        np.maximum.at(longest, (c0 - 1) // 64, r)
    return out, longest


def oracle_texture(lab, vol, n_labels, lo=-1000, hi=199, bin_width=25, distance=1, nr=None, walk=run_lengths) -> dict:
    """What Engine.texture returns; nr None: the unclamped GLRLM with as many columns as the longest run (what texture_matrices
    returns), else nr columns with the last one absorbing the longer runs."""
    ng = (hi - lo) // bin_width + 1
    code, out = oracle_codes(np.asarray(lab), np.asarray(vol), n_labels, lo, hi, bin_width)
    out["glcm"] = oracle_glcm(code, n_labels, ng, distance)
    full, out["longest_run"] = oracle_glrlm(code, n_labels, ng, walk)
    if nr is not None:
        clamped = np.zeros(full.shape[:3] + (nr,), np.int64)
        for c in range(full.shape[3]):
            clamped[..., min(c, nr - 1)] += full[..., c]
        full = clamped
    out["glrlm"], out["levels"] = full, ng
    out.update(lo=lo, hi=hi, bin_width=bin_width, distance=distance)
    return out


def assert_texture_equal(got: dict, want: dict, pairs=(), runs=(), what=""):
    """Bit for bit; `pairs` / `runs`: the labels that must have a non-zero GLCM / GLRLM total."""
    for f in COUNTS + ("glcm",):
        assert np.array_equal(np.asarray(got[f], np.int64), want[f]), (what, f, got[f], want[f])
    if got["glrlm"] is not None:
        assert got["glrlm"].dtype == np.int64 and np.array_equal(got["glrlm"], want["glrlm"]), (what, "glrlm")
    assert got["levels"] == want["levels"]
    for k in pairs:
        assert want["glcm"][k].sum() > 0, (what, "no pair of label", k)
    for k in runs:
        assert want["glrlm"][k].sum() > 0, (what, "no run of label", k)


def random_case(rng, shape, n_labels, dtype=np.int16, extra=1, lo=-1000, bin_width=25, levels=6, first_level=0):
    """Labels in blocks of 3 along x (0 .. n_labels + extra - 1); intensities from `levels` values one bin apart plus a few values
    outside the range, so that runs longer than 1 and repeated pairs occur."""
    n, h, w = shape
    lab = np.repeat(rng.integers(0, n_labels + extra, (n, h, (w + 2) // 3)), 3, axis=2)[:, :, :w].astype(np.uint8)
    inside = lo + bin_width * (first_level + rng.integers(0, levels, shape)) + rng.integers(0, bin_width, shape) // 2
    outside = rng.choice([lo - 1, lo - 300, lo + bin_width * 64 + 700], shape)
    vol = np.where(rng.random(shape) < 0.08, outside, inside).astype(dtype)
    return lab, vol


def check(eng, lab, vol, n_labels, pairs=None, runs=None, what="", **kw):
    every = [k for k in range(1, n_labels)]
    got = eng.texture(lab, vol, n_labels, **kw)
    want = oracle_texture(lab, vol, n_labels, nr=kw.pop("nr", 64), **kw)
    assert_texture_equal(got, want, every if pairs is None else pairs, every if runs is None else runs, what)
    return got


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64, np.float32, np.float64])
def test_texture_dtypes(emu_engine, dtype):
    rng = np.random.default_rng(1)
    lab, vol = random_case(rng, (3, 21, 48), 3, dtype)
    if np.dtype(dtype).kind == "f":
        vol = vol + rng.choice([0.0, 0.25, 0.5, -0.5, 1.5], vol.shape).astype(dtype)
    check(emu_engine, lab, vol, 3, what=dtype)


def test_texture_vectorised_walk_is_the_plain_walk():
    """The oracle's run walk against the plain voxel-by-voxel one."""
    rng = np.random.default_rng(2)
    lab, vol = random_case(rng, (3, 9, 14), 3)
    a = oracle_texture(lab, vol, 3)
    b = oracle_texture(lab, vol, 3, walk=run_lengths_python)
    assert np.array_equal(a["glrlm"], b["glrlm"]) and np.array_equal(a["longest_run"], b["longest_run"])
    assert a["glrlm"][1:].sum() > 0 and a["glrlm"].shape[3] > 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_texture_float_specials(emu_engine, dtype):
    """.5 ties at a bin edge and at the range's ends (half to even), NaN, +-inf, values just outside lo and hi."""
    rng = np.random.default_rng(3)
    shape = (2, 9, 37)
    lab = np.repeat(rng.integers(0, 4, (2, 9, 13)), 3, axis=2)[:, :, :37].astype(np.uint8)
    specials = np.array([-975.5, -974.5, -976.5, -975.0, -1000.5, -1001.5, -1000.4, -1000.6, 199.5, 198.5, 199.4, 199.6, 200.0, -1001.0,
                         -950.0, -925.5, np.nan, np.inf, -np.inf, 3e9, -3e9], dtype=np.float64)
    vol = rng.choice(specials, shape).astype(dtype)
    vol[0, 0, :5] = np.nan
    got = check(emu_engine, lab, vol, 4, what=dtype)
    assert got["nonfinite"][1:].sum() > 0 and got["below"][1:].sum() > 0 and got["above"][1:].sum() > 0


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 7), (2, 3, 33), (4, 13, 50), (3, 11, 64), (5, 1, 16)])
def test_texture_shapes(emu_engine, shape):
    """One voxel, no z directions, no y directions, w not a multiple of 16 and a multiple of it."""
    rng = np.random.default_rng(4)
    lab, vol = random_case(rng, shape, 3, extra=2)
    if shape == (1, 1, 1):
        lab[...], vol[...] = 1, -900
    got = check(emu_engine, lab, vol, 3, pairs=() if shape == (1, 1, 1) else None, runs=(1,) if shape == (1, 1, 1) else None, what=shape)
    if shape[0] == 1:
        assert got["glcm"][:, 4:].sum() == 0 and got["glrlm"][:, 4:, :, 1:].sum() == 0  # no pair and no run > 1 along z


@pytest.mark.parametrize("n_labels", [1, 3, 6, 16])
def test_texture_label_groups(emu_engine, n_labels):
    """n_labels 1, 3, 6 and 16 with labels >= n_labels present: one workgroup's labels, and several label groups."""
    rng = np.random.default_rng(5 + n_labels)
    lab, vol = random_case(rng, (3, 17, 48), n_labels, extra=2)
    assert (lab >= n_labels).any()
    got = check(emu_engine, lab, vol, n_labels, what=n_labels)
    assert got["glcm"][0].sum() == 0 and got["glrlm"][0].sum() == 0 and got["voxels"][0] == 0
    if n_labels == 16:  # 64 levels: three labels per workgroup, five groups
        lab, vol = random_case(rng, (3, 17, 48), 16, extra=1, levels=64)
        check(emu_engine, lab, vol, 16, what="16 x 64", hi=599)


def test_texture_label_extents(emu_engine):
    """A label that fills the volume (runs and pairs end at every border), a single-voxel label, an empty label."""
    rng = np.random.default_rng(6)
    shape = (3, 10, 20)
    _, vol = random_case(rng, shape, 2)
    full = np.ones(shape, np.uint8)
    check(emu_engine, full, vol, 2, what="full")
    lab = np.where(rng.random(shape) < 0.5, 1, 4).astype(np.uint8)
    lab[2, 9, 19], vol[2, 9, 19] = 3, -900  # a single voxel in the last position; label 2 empty
    got = check(emu_engine, lab, vol, 5, pairs=(1, 4), runs=(1, 3, 4), what="mixed")
    assert got["glcm"][3].sum() == 0 and got["glrlm"][3].sum() == 13 and got["longest_run"][3] == 1
    assert got["voxels"][2] == 0 and got["glrlm"][2].sum() == 0 and got["longest_run"][2] == 0


@pytest.mark.parametrize("distance", [2, 8])
def test_texture_distance(emu_engine, distance):
    """Distances 2 and 8; n = 3 and h = 7 are smaller than 8: only the x direction has such pairs."""
    rng = np.random.default_rng(7)
    lab, vol = random_case(rng, (3, 7, 40), 2, extra=0)
    got = check(emu_engine, lab, vol, 2, what=distance, distance=distance)
    assert (got["glcm"][1, 1:].sum() == 0) == (distance == 8) and got["glcm"][1, 0].sum() > 0


@pytest.mark.parametrize("levels, kw", [(1, dict(bin_width=1200)), (48, {}), (64, dict(hi=599))])
def test_texture_levels(emu_engine, levels, kw):
    rng = np.random.default_rng(8)
    lab, vol = random_case(rng, (2, 12, 32), 3, levels=levels)
    got = check(emu_engine, lab, vol, 3, what=levels, **kw)
    assert got["levels"] == levels and got["glcm"].shape == (3, 13, levels, levels)
    if levels == 64:
        assert got["glcm"][:, :, 60:, :].sum() > 0  # the top levels are in use


def test_texture_invalid_arguments(emu_engine):
    lab = np.ones((2, 4, 4), np.uint8)
    vol = np.full((2, 4, 4), -900, np.int16)
    for kw in (dict(hi=600), dict(bin_width=0), dict(lo=200), dict(nr=0), dict(nr=8193), dict(distance=9), dict(distance=0)):
        with pytest.raises(nat.LMError, match="lm_texture_dev"):
            emu_engine.texture(lab, vol, 2, **kw)
    for k in (0, 17):
        with pytest.raises(nat.LMError, match="lm_texture_dev"):
            emu_engine.texture(lab, vol, k)
    with pytest.raises(nat.LMError):
        emu_engine.texture(lab, vol.astype(np.uint16), 2)
    with pytest.raises(nat.LMError):
        emu_engine.texture(lab, np.zeros((2, 4, 5), np.int16), 2)
    ld = nat.DeviceView.__new__(nat.DeviceView)
    ld.eng, ld.shape, ld.dtype, ld.ptr, ld.nbytes = emu_engine, (2, 2, 4097), np.dtype(np.uint8), 16, 0
    vd = nat.DeviceView.__new__(nat.DeviceView)
    vd.eng, vd.shape, vd.dtype, vd.ptr, vd.nbytes = emu_engine, (2, 2, 4097), np.dtype(np.int16), 16, 0
    with pytest.raises(nat.LMError, match="too large"):
        emu_engine.texture_dev(ld, vd, 2)  # refused before anything is read


def test_texture_long_runs(emu_engine):
    """A constant 2 x 3 x 40 block with nr = 8: the last column absorbs the long runs, longest_run says so, and texture_matrices
    returns the unclamped 40-column matrix."""
    from lungmask_amd import texture as tx

    lab = np.zeros((4, 5, 44), np.uint8)
    lab[1:3, 1:4, 2:42] = 1
    vol = np.full(lab.shape, -800, np.int16)
    got = check(emu_engine, lab, vol, 2, what="nr 8", nr=8)
    level = (-800 + 1000) // 25
    assert got["longest_run"][1] == 40 and got["glrlm"].shape[3] == 8
    assert got["glrlm"][1, 0, level, 7] == 6 and got["glrlm"][1, 0].sum() == 6  # the six rows along x, all in the last column
    raw = tx.texture_matrices(vol, lab, engine=emu_engine)
    want = oracle_texture(lab, vol, 2)
    assert raw["glrlm"].shape == (2, 13, 48, 40) and want["glrlm"].shape == (2, 13, 48, 40)
    assert_texture_equal(raw, want, (1,), (1,), "unclamped")
    assert raw["glrlm"][1, 0, level, 39] == 6


def test_texture_second_call_for_runs_beyond_64_columns(emu_engine):
    from lungmask_amd import texture as tx

    lab = np.ones((1, 2, 100), np.uint8)
    vol = np.full(lab.shape, 0, np.int32)
    raw = tx.texture_matrices(vol, lab, engine=emu_engine)
    assert_texture_equal(raw, oracle_texture(lab, vol, 2), (1,), (1,), "100 columns")
    assert raw["glrlm"].shape[3] == 100 and raw["longest_run"][1] == 100


def test_texture_without_glrlm(emu_engine):
    """glrlm_out = NULL: the GLCM, the counts and longest_run (short and long runs) all the same."""
    rng = np.random.default_rng(9)
    lab, vol = random_case(rng, (2, 8, 40), 3)
    vol[1, 3, 5:35], lab[1, 3, 5:35] = -700, 2  # a run of 30: beyond the columns the device keeps without the matrix
    got = emu_engine.texture(lab, vol, 3, glrlm=False)
    assert got["glrlm"] is None
    want = oracle_texture(lab, vol, 3)
    assert want["longest_run"][2] >= 30 > 16 > want["longest_run"][1] > 1
    assert_texture_equal(got, want, (1, 2), (1, 2), "no glrlm")
