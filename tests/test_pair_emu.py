"""lm_pair_map_dev on the emulation library, bit for bit against `pair_map_oracle`, a numpy restatement of the definition in
include/lungmask_hip.h (test_gpu_pair.py runs the same `run_*` cases on the device): the three maps and the integer table at the
shapes of test_deform_emu.py, every field kind, every dtype pair, label patterns, NULL outputs, the folded field, the sum that
passes 2^32 and values exactly on the bounds; the properties that tie the call to lm_warp_dev and lm_jacobian_dev; every refusal;
and the mass pair -- a synthetic pair whose fixed image is the moving one deformed AND diluted by the Jacobian, on which the
mass-corrected change stays within the noise while the plain difference does not."""
import warnings

import numpy as np
import pytest

from lungmask_amd import _native as nat
from tests.test_deform_emu import (DEMONS_DTYPES, FIELDS, RECOVERY_SHAPE, SHAPES, SHAPE_IDS, SPACING, content, coordinate, domain, jacobian_oracle,
                                   make_field, rot_scale, same_bits, scales, trilinear, warp_oracle)
from tests.test_register_emu import volume

COLS = nat.LM_PAIR_COLS
MAPS = ("classes", "change", "jacobian")
DEFAULTS = dict(spacing=None, jac_scale=1.0, air=-1000.0, fixed_thr=-950.0, moving_thr=-856.0, lo=-1000.0, hi=-500.0, keep=None)


# ------------------------------------------------------------------------------------------------ the oracle
def det64(field, spacing=None):
    """lm_jacobian_dev's determinant before its rounding to float32 (jacobian_oracle's expressions; test_det64 holds them together)."""
    fs, _ = scales(spacing)
    shape = field.shape[1:]
    a = [[None] * 3 for _ in range(3)]
    for i in range(3):
        ui = field[i].astype(np.float64)
        for j in range(3):
            G = np.zeros(shape)
            if shape[j] > 1:
                G = np.moveaxis(G, j, 0)
                s = np.moveaxis(ui, j, 0)
                G[1:-1] = ((s[2:] - s[:-2]) * fs[i]) * 0.5
                G[0] = (s[1] - s[0]) * fs[i]
                G[-1] = (s[-1] - s[-2]) * fs[i]
                G = np.moveaxis(G, 0, j)
            a[i][j] = (1.0 if i == j else 0.0) + G
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) + \
        a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])


def exact_sum(terms):
    return sum(int(t) for t in terms.astype(np.int64).reshape(-1)) if terms.size < 4096 else int(terms.astype(np.int64).sum())


def pair_map_oracle(fixed, labels, moving, field, A, b, n_labels, spacing=None, jac_scale=1.0, air=-1000.0, fixed_thr=-950.0,
                    moving_thr=-856.0, lo=-1000.0, hi=-500.0, keep=None):
    """lm_pair_map_dev's definition -> (table: n_labels rows of LM_PAIR_COLS Python integers, {"classes", "change", "jacobian"})."""
    fs, _ = scales(spacing)
    shape = fixed.shape
    kept = np.zeros(256, bool)
    kept[list(range(1, 256)) if keep is None else list(keep)] = True
    kept[n_labels:] = False
    sel = kept[labels]
    F = fixed.astype(np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        c = coordinate(A, b, shape, field, fs)
        inside, _ = domain(c, moving.shape)
        m = trilinear(moving, c)
        J = jac_scale * (np.ones(shape) if field is None else det64(field, spacing))
        nan_f = np.isnan(F)
        rest = sel & ~nan_f & inside
        nan_mj = rest & (np.isnan(m) | np.isnan(J))
        folded = rest & ~nan_mj & (J <= 0.0)
        live = rest & ~nan_mj & ~folded
        mc = J * (m - air) + air
        change = mc - F
        nan_c = live & np.isnan(change)
        valid = live & ~nan_c
        nonfinite = (sel & nan_f) | nan_mj | nan_c
        outside = sel & ~nan_f & ~inside
        window = (lo <= F) & (F <= hi) & (lo <= m) & (m <= hi)
        code = 1 + (F < fixed_thr).astype(np.int64) + 2 * (m < moving_thr).astype(np.int64)
        classes = np.where(valid & window, code, 0).astype(np.uint8)
        out = {"classes": classes, "change": np.where(valid, change, 0.0).astype(np.float32),
               "jacobian": np.where(valid | folded, J, 0.0).astype(np.float32)}
        t5 = np.floor(np.where(J < 64.0, J, 64.0) * 1048576.0 + 0.5)
        cc = np.where(change < 65536.0, change, 65536.0)
        t6 = np.floor(np.where(cc > -65536.0, cc, -65536.0) * 16.0 + 0.5)
        c2 = change * change
        t7 = np.floor(np.where(c2 < 16777216.0, c2, 16777216.0) * 16.0 + 0.5)
    table = []
    for L in range(n_labels):
        at = labels == L
        v = valid & at
        row = [int((sel & at).sum()), int(v.sum()), int((outside & at).sum()), int((nonfinite & at).sum()), int((folded & at).sum()),
               exact_sum(t5[v]), exact_sum(t6[v]), exact_sum(t7[v]), int((v & ~window).sum())]
        table.append(row + [int((classes[at] == k).sum()) for k in (1, 2, 3, 4)])
    return table, out


def pair_host(eng, fixed, labels, moving, field, A, b, n_labels, maps=MAPS, **kw):
    """The call into dirty outputs -> (table as nested lists, {name: array})."""
    with eng.scope() as dev:
        table = dev.empty((n_labels, COLS), np.int64)
        table.upload(np.full((n_labels, COLS), -1, np.int64))
        out = {}
        for name in maps:
            dt = np.uint8 if name == "classes" else np.float32
            out[name] = dev.empty(fixed.shape, dt)
            out[name].upload(np.full(fixed.shape, 77, dt))
        eng.pair_map_dev(dev.upload(fixed), dev.upload(labels), dev.upload(moving), dev.upload(field) if field is not None else None, A, b, table,
                         n_labels, classes=out.get("classes"), change=out.get("change"), jacobian=out.get("jacobian"), **kw)
        eng.sync()
        return [[int(v) for v in row] for row in table.download()], {k: v.download() for k, v in out.items()}


def invariants(table):
    for row in table:
        assert row[0] == row[1] + row[2] + row[3] + row[4], row
        assert row[1] == sum(row[8:13]), row
        assert min(row[:6]) >= 0 and min(row[7:]) >= 0, row


def check_pair(eng, fixed, labels, moving, field, A, b, n_labels, maps=MAPS, **kw):
    table, out = pair_host(eng, fixed, labels, moving, field, A, b, n_labels, maps, **kw)
    want_table, want = pair_map_oracle(fixed, labels, moving, field, A, b, n_labels, **kw)
    assert table == want_table, (table, want_table)
    invariants(table)
    assert sorted(out) == sorted(maps)
    for name in maps:
        assert same_bits(out[name], want[name]), (name, np.argwhere(out[name] != want[name])[:5])
    return table, out


def lung_row(table):
    return [sum(row[c] for row in table[1:]) for c in range(COLS)]


def labels_of(shape, seed, top=4):
    return np.random.default_rng(seed).integers(0, top, shape).astype(np.uint8)


def lungish(shape, dtype, seed):
    """A volume whose values spread over the class window and both thresholds (and, for floats, `volume`'s special values)."""
    v = volume(shape, dtype, seed)
    base = np.random.default_rng(seed + 100).normal(-850.0, 120.0, shape)
    if np.dtype(dtype).kind == "f":
        return np.where(np.isfinite(v) & (np.abs(v) < 2e3), base, v).astype(dtype)
    return np.where(np.abs(v) < 2 ** 31, np.rint(base), v).astype(dtype)


# ------------------------------------------------------------------------------------------------ cases
def run_pair_cases(eng, shapes, kind):
    fshape, mshape = shapes
    A, b = (np.eye(3), np.zeros(3)) if fshape == (1, 1, 1) else rot_scale()
    field = make_field(kind, fshape, 31, SPACING)
    fixed, moving = lungish(fshape, np.int16, 32), lungish(mshape, np.float32, 33)
    labels = labels_of(fshape, 34)
    scale = 1.0 if fshape == (1, 1, 1) else abs(float(np.linalg.det(A)))
    table, _ = check_pair(eng, fixed, labels, moving, field, A, b, 4, spacing=SPACING, jac_scale=scale)
    if fshape == (3, 37, 130):
        assert sum(row[0] for row in table) == int((labels > 0).sum()) and sum(row[1] for row in table) > 0
        if kind in ("random", "special"):
            assert sum(row[2] for row in table) > 0  # some samples leave the moving volume
        if kind == "special":
            assert sum(row[3] for row in table) > 0
    check_pair(eng, fixed, labels, moving, field, A, b, 3, spacing=SPACING, jac_scale=scale, keep=(0, 2), air=-990.5, fixed_thr=-900.0,
               moving_thr=-800.0, lo=-1100.0, hi=-300.0)


def run_pair_dtypes(eng, fdtype, mdtype):
    A, b = rot_scale()
    fixed, moving = lungish((5, 7, 9), fdtype, 35), lungish((4, 6, 11), mdtype, 36)
    field = make_field("random", (5, 7, 9), 37)
    labels = labels_of((5, 7, 9), 38, 3)
    if np.dtype(fdtype).kind == "f":
        labels[np.isnan(fixed)] = 1
    table, _ = check_pair(eng, fixed, labels, moving, field, A, b, 3, jac_scale=abs(float(np.linalg.det(A))))
    if np.dtype(fdtype).kind == "f":
        assert sum(row[3] for row in table) >= 1  # the NaN of the fixed volume


def run_label_patterns(eng):
    """Unkept values, values >= n_labels, all 16 rows in use; and each output NULL in turn."""
    shape = (3, 37, 130)
    A, b = rot_scale()
    fixed, moving, field = lungish(shape, np.int16, 39), lungish(shape, np.int16, 40), make_field("random", shape, 41, SPACING)
    labels = np.random.default_rng(42).integers(0, 20, shape).astype(np.uint8)
    labels[0, :2] = 255
    table, _ = check_pair(eng, fixed, labels, moving, field, A, b, 16, spacing=SPACING, keep=range(0, 256))
    assert all(row[0] > 0 for row in table) and sum(row[0] for row in table) == int((labels < 16).sum())
    table, _ = check_pair(eng, fixed, labels, moving, field, A, b, 16, spacing=SPACING, keep=(1, 5, 15, 17, 255))
    assert [i for i, row in enumerate(table) if row[0]] == [1, 5, 15]
    check_pair(eng, fixed, labels, moving, field, A, b, 7, spacing=SPACING)
    full = check_pair(eng, fixed, labels, moving, field, A, b, 9, spacing=SPACING)
    for maps in (("change", "jacobian"), ("classes", "jacobian"), ("classes", "change"), ()):
        part = check_pair(eng, fixed, labels, moving, field, A, b, 9, maps, spacing=SPACING)
        assert part[0] == full[0] and all(same_bits(part[1][k], full[1][k]) for k in maps)


def run_folded(eng):
    """The folded field of the Jacobian cases: column 4, and the NaN of the field in column 3."""
    fold = np.zeros((3, 4, 9, 20), np.float32)
    fold[2, :, :, 8:14] = -1.5 * np.arange(6, dtype=np.float32)
    fold[0, 2, 4, 3] = np.nan
    shape = fold.shape[1:]
    fixed, moving = lungish(shape, np.int16, 43), lungish(shape, np.int16, 44)
    labels = np.ones(shape, np.uint8)
    labels[:, :, 10:] = 2
    table, out = check_pair(eng, fixed, labels, moving, fold, np.eye(3), np.zeros(3), 3)
    det = jacobian_oracle(fold)[0]
    inside = domain(coordinate(np.eye(3), np.zeros(3), shape, fold, [1.0] * 3), shape)[0]
    assert table[1][4] + table[2][4] == int(((det <= 0) & inside).sum()) > 0 and table[1][4] > 0 and table[2][4] > 0
    assert table[1][3] + table[2][3] >= 6  # the six neighbours of the NaN, and the voxel itself (its coordinate is outside: column 2)
    folded = (det <= 0) & inside
    assert same_bits(out["jacobian"][folded], det[folded]) and not out["change"][folded].any() and not out["classes"][folded].any()


def run_large_sum(eng):
    """A constant 41 x 41 x 41 pair: every term of column 7 is the cap 2^24 * 16 = 2^28, the sum passes 2^32."""
    fixed, moving = np.full((41, 41, 41), 3000, np.int16), np.full((41, 41, 41), -1096, np.int16)
    labels = np.ones((41, 41, 41), np.uint8)
    zero = np.zeros((3, 41, 41, 41), np.float32)
    table, out = check_pair(eng, fixed, labels, moving, zero, np.eye(3), np.zeros(3), 2, air=0.0)
    n = 41 ** 3
    assert table[1] == [n, n, 0, 0, 0, n << 20, -4096 * 16 * n, n << 28, n, 0, 0, 0, 0] and table[1][7] > 2 ** 32 and table[0] == [0] * COLS
    assert np.all(out["change"] == -4096.0) and np.all(out["jacobian"] == 1.0)


def run_bounds(eng):
    """Values exactly on lo, hi and both thresholds: lo and hi are inside the window, a value equal to a threshold is not low."""
    values = np.array([-1001, -1000, -999, -951, -950, -949, -857, -856, -855, -501, -500, -499], np.int16)
    fixed, moving = np.meshgrid(values, values, indexing="ij")
    fixed, moving = np.ascontiguousarray(fixed[None]), np.ascontiguousarray(moving[None])
    labels = np.ones(fixed.shape, np.uint8)
    table, out = check_pair(eng, fixed, labels, moving, None, np.eye(3), np.zeros(3), 2)
    cls = out["classes"][0]
    f, m = fixed[0].astype(np.int64), moving[0].astype(np.int64)
    window = (f >= -1000) & (f <= -500) & (m >= -1000) & (m <= -500)
    assert np.array_equal(cls, np.where(window, 1 + (f < -950) + 2 * (m < -856), 0))
    at = lambda fv, mv: int(cls[list(values).index(fv), list(values).index(mv)])  # noqa: E731
    assert (at(-1000, -500), at(-950, -856), at(-951, -857), at(-951, -856), at(-950, -857)) == (2, 1, 4, 2, 3)
    assert (at(-1001, -949), at(-949, -499), at(-500, -1000)) == (0, 0, 3)
    assert table[1][0] == table[1][1] == 144 and table[1][8] == int((~window).sum()) and sum(table[1][9:]) == int(window.sum())
    assert np.array_equal(out["change"], (moving.astype(np.float64) - fixed).astype(np.float32))  # (J = 1: mc = m exactly here)


def run_properties(eng):
    shape = (3, 37, 130)
    A, b = rot_scale()
    fixed, moving = lungish(shape, np.int16, 45), lungish(shape, np.float32, 46)
    labels = labels_of(shape, 47, 6)
    fs, _ = scales(SPACING)
    # a field of zeros, jac_scale 1, air 0: J == 1, column 5 is analysed << 20, change is (float)(m - f)
    zero = np.zeros((3,) + shape, np.float32)
    table, out = check_pair(eng, fixed, labels, moving, zero, A, b, 6, spacing=SPACING, air=0.0)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        c = coordinate(A, b, shape, None, fs)
        m = trilinear(moving, c)
        inside = domain(c, shape)[0]
    valid = (labels > 0) & inside & ~np.isnan(m) & ~np.isnan(m - fixed)
    assert sum(row[1] for row in table) == int(valid.sum()) > 0
    assert np.all(out["jacobian"][valid] == 1.0) and all(row[5] == row[1] << 20 for row in table)
    assert same_bits(out["change"][valid], (m - fixed.astype(np.float64)).astype(np.float32)[valid])
    null = check_pair(eng, fixed, labels, moving, None, A, b, 6, spacing=SPACING, air=0.0)
    assert null[0] == table and all(same_bits(null[1][k], out[k]) for k in MAPS)  # p = o exactly
    # jac_scale 1: the Jacobian map has lm_jacobian_dev's bits at the valid voxels; the classes are the thresholds applied to
    # lm_warp_dev's float64 value
    field = make_field("random", shape, 48, SPACING)
    table, out = check_pair(eng, fixed, labels, moving, field, A, b, 6, spacing=SPACING)
    det, _, _ = eng.jacobian(field, SPACING)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        c = coordinate(A, b, shape, field, fs)
        m = trilinear(moving, c)
        inside = domain(c, shape)[0]
    valid = (labels > 0) & inside & ~np.isnan(m) & (det > 0)
    valid &= ~np.isnan(det64(field, SPACING) * (m + 1000.0) - 1000.0 - fixed)
    assert sum(row[1] for row in table) == int(valid.sum()) > 0 and same_bits(out["jacobian"][valid], det[valid])
    warped = warp_oracle(moving, field, A, b, shape, "linear", np.nan, np.float32, SPACING)
    assert same_bits(np.where(inside, m, np.nan).astype(np.float32), warped)
    f = fixed.astype(np.float64)
    window = (f >= -1000.0) & (f <= -500.0) & (m >= -1000.0) & (m <= -500.0)
    assert np.array_equal(out["classes"], np.where(valid & window, 1 + (f < -950.0) + 2 * (m < -856.0), 0))
    assert len(np.unique(out["classes"])) == 5
    # the lung row (the exact column sum of the labels >= 1) is the table of one label for the same voxels
    merged = ((labels >= 1) & (labels < 6)).astype(np.uint8)
    one, one_out = check_pair(eng, fixed, merged, moving, field, A, b, 2, spacing=SPACING)
    assert lung_row(table) == one[1] and all(same_bits(one_out[k], out[k]) for k in MAPS)


# ------------------------------------------------------------------------------------------------ the mass pair
_MASS = {}


def mass_pair():
    """(fixed int16, moving int16, the true field float32 [3][n][h][w] in voxels, the analytic Jacobian): the sinusoid field of
    `recovery_pair` at peak 2 voxels, fixed = rint(air + J (content(o + u) - air) + N(0, 20)), moving = rint(content(o) + N(0, 20)),
    air = -1000: the fixed image is the moving one deformed and diluted by the local volume change."""
    if not _MASS:
        n, h, w = RECOVERY_SHAPE
        z, y, x = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        ax = [(z, n - 1), (y, h - 1), (x, w - 1)]
        e = [np.sin(np.pi * q / L) for q, L in ax]
        de = [np.pi / L * np.cos(np.pi * q / L) for q, L in ax]
        s = [np.sin(2 * np.pi * q / L) for q, L in ax]
        ds = [2 * np.pi / L * np.cos(2 * np.pi * q / L) for q, L in ax]
        env = e[0] * e[1] * e[2]
        denv = [de[0] * e[1] * e[2], e[0] * de[1] * e[2], e[0] * e[1] * de[2]]
        carrier = (1, 2, 0)  # u_0 carries sin(y), u_1 sin(x), u_2 sin(z)
        raw = np.stack([2.0 * env * s[carrier[i]] for i in range(3)])
        k = 2.0 / np.abs(raw).max()
        u = raw * k
        a = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                g = 2.0 * k * (denv[j] * s[carrier[i]] + (env * ds[carrier[i]] if j == carrier[i] else 0.0))
                a[i][j] = (1.0 if i == j else 0.0) + g
        J = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) + \
            a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0])
        rng = np.random.default_rng(7)
        fixed = np.rint(-1000.0 + J * (content(z + u[0], y + u[1], x + u[2]) + 1000.0) + rng.normal(0.0, 20.0, z.shape)).astype(np.int16)
        moving = np.rint(content(z, y, x) + rng.normal(0.0, 20.0, z.shape)).astype(np.int16)
        _MASS["pair"] = (fixed, moving, u.astype(np.float32), J)
    return _MASS["pair"]


def run_mass_pair(eng):
    fixed, moving, u, J = mass_pair()
    labels = np.ones(fixed.shape, np.uint8)
    labels[:, :, 22:] = 2
    table, out = check_pair(eng, fixed, labels, moving, u, np.eye(3), np.zeros(3), 3, lo=-2000.0, hi=2000.0)
    lung = lung_row(table)
    bound = 400.0 * (1.0 + float(J.max()) ** 2)
    corrected = lung[7] / 16.0 / lung[1]
    m = trilinear(moving, coordinate(np.eye(3), np.zeros(3), fixed.shape, u, [1.0] * 3))
    plain = float(((m - fixed) ** 2).mean())
    fd = float(np.abs(det64(u) - J).max())
    print(f"mass pair {fixed.shape}: J {J.min():.3f} .. {J.max():.3f} (finite differences within {fd:.4f}), bound rms {bound ** 0.5:.1f}; "
          f"mass-corrected rms {corrected ** 0.5:.1f} HU, uncorrected rms {plain ** 0.5:.1f} HU; mean Jacobian {lung[5] / 2 ** 20 / lung[1]:.4f}, "
          f"mean change {lung[6] / 16.0 / lung[1]:.2f} HU; {lung[1]} of {lung[0]} voxels analysed, {lung[2]} outside")
    assert lung[0] == lung[1] == fixed.size and lung[2] == 0  # all voxels are inside
    assert corrected <= bound < plain
    assert fd < 0.01 and same_bits(out["jacobian"], det64(u).astype(np.float32))


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shapes", SHAPES, ids=SHAPE_IDS)
def test_pair_map(emu_engine, shapes, kind):
    run_pair_cases(emu_engine, shapes, kind)


@pytest.mark.parametrize("mdtype", DEMONS_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fdtype", DEMONS_DTYPES, ids=lambda d: np.dtype(d).name)
def test_pair_dtypes(emu_engine, fdtype, mdtype):
    run_pair_dtypes(emu_engine, fdtype, mdtype)


def test_label_patterns_and_null_outputs(emu_engine):
    run_label_patterns(emu_engine)


def test_folded_field(emu_engine):
    run_folded(emu_engine)


def test_sum_passes_2_32(emu_engine):
    run_large_sum(emu_engine)


def test_values_on_the_bounds(emu_engine):
    run_bounds(emu_engine)


def test_properties(emu_engine):
    run_properties(emu_engine)


def test_mass_pair(emu_engine):
    run_mass_pair(emu_engine)


def test_det64_is_the_jacobian_oracle_before_rounding():
    for kind in ("random", "special"):
        field = make_field(kind, (3, 7, 9), 49, SPACING)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            assert same_bits(det64(field, SPACING).astype(np.float32), jacobian_oracle(field, SPACING)[0])


def test_refusals(emu_engine):
    """Every refusal of the header, as a returned error: no pointer is followed."""
    eng = emu_engine
    lib = eng.L.lib

    def params(**kw):
        p = nat.PairParams()
        p.A[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        p.field_scale[:] = [1.0, 1.0, 1.0]
        p.jac_scale, p.air, p.fixed_thr, p.moving_thr, p.lo, p.hi, p.n_labels = 1.0, -1000.0, -950.0, -856.0, -1000.0, -500.0, 2
        for k, v in kw.items():
            if k in ("A", "b", "field_scale"):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    with eng.scope() as dev:
        vol, lab, u = dev.upload(np.zeros((2, 3, 4), np.int16)), dev.upload(np.ones((2, 3, 4), np.uint8)), dev.upload(np.zeros((3, 2, 3, 4), np.float32))
        cls, chg, jac = dev.empty((2, 3, 4), np.uint8), dev.empty((2, 3, 4), np.float32), dev.empty((2, 3, 4), np.float32)
        table = dev.empty((2, COLS), np.int64)

        def call(p, fixed=vol.ptr, fdt=0, fdims=(2, 3, 4), labels=lab.ptr, moving=vol.ptr, mdt=0, mdims=(2, 3, 4), field=u.ptr, c=cls.ptr, d=chg.ptr,
                 j=jac.ptr, t=table.ptr):
            return lib.lm_pair_map_dev(eng.h, fixed, fdt, *fdims, labels, moving, mdt, *mdims, field, p, c, d, j, t)

        def refused(text, *a, **kw):
            assert call(*a, **kw) < 0 and text in lib.lm_last_error(), lib.lm_last_error()

        assert call(params()) == 0
        assert call(params(), field=None, c=None, d=None, j=None) == 0
        for dims in ((0, 3, 4), (2, 4097, 4), (2, 3, -1)):
            refused(b"4096", params(), fdims=dims)
            refused(b"4096", params(), mdims=dims)
        refused(b"below 2^31", params(), fdims=(4096, 4096, 128))
        refused(b"below 2^31", params(), mdims=(128, 4096, 4096))
        # the whole text of the checks the entry point shares with lm_joint_hist_dev and lm_demons_step_dev
        refused(b"lm_pair_map_dev: every dimension of the fixed volume must lie in 1 .. 4096 (got 0)", params(), fdims=(0, 3, 4))
        refused(b"lm_pair_map_dev: every dimension of the moving volume must lie in 1 .. 4096 (got 4097)", params(), mdims=(2, 4097, 4))
        refused(b"lm_pair_map_dev: volume too large (n * h * w must stay below 2^31)", params(), fdims=(4096, 4096, 128))
        refused(b"lm_pair_map_dev: dtype must be LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 (got 4, 0)", params(), fdt=4)
        refused(b"lm_pair_map_dev: dtype must be LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 (got 0, 5)", params(), mdt=5)
        refused(b"lm_pair_map_dev: A, b, field_scale, air, the thresholds, lo and hi must be finite, jac_scale finite and > 0, lo <= hi",
                params(b=(2, np.inf)))
        for name in ("fixed", "labels", "moving", "t"):
            refused(b"not NULL", params(), **{name: None})
        assert lib.lm_pair_map_dev(eng.h, vol.ptr, 0, 2, 3, 4, lab.ptr, vol.ptr, 0, 2, 3, 4, None, None, None, None, None, table.ptr) < 0
        assert b"not NULL" in lib.lm_last_error()
        for code in (4, 5, 7, -1, 99):  # uint8, uint16, float16, nonsense
            refused(b"dtype must be", params(), fdt=code)
            refused(b"dtype must be", params(), mdt=code)
        for n in (0, 17, -3):
            refused(b"n_labels", params(n_labels=n))
        for bad in (np.nan, np.inf, -np.inf):
            for kw in (dict(A=(4, bad)), dict(b=(1, bad)), dict(field_scale=(2, bad)), dict(jac_scale=bad), dict(air=bad), dict(fixed_thr=bad),
                       dict(moving_thr=bad), dict(lo=bad), dict(hi=bad)):
                refused(b"finite", params(**kw))
        refused(b"jac_scale", params(jac_scale=0.0))
        refused(b"jac_scale", params(jac_scale=-1.0))
        refused(b"lo <= hi", params(lo=-500.0, hi=-500.5))
        assert call(params(lo=-500.0, hi=-500.0)) == 0
        # an output that is, or lies inside, an input; two outputs that overlap
        refused(b"overlap an input", params(), c=lab.ptr)
        refused(b"overlap an input", params(), d=u.ptr + 96)
        refused(b"overlap an input", params(), j=u.ptr)
        refused(b"overlap an input", params(), t=vol.ptr)
        refused(b"overlap an input", params(), c=vol.ptr + 47)
        refused(b"overlap one another", params(), d=jac.ptr)
        assert call(params(), field=None, d=u.ptr) == 0  # (without a field that memory is no input)
        with pytest.raises(nat.LMError, match="same 3-D shape"):
            eng.pair_map_dev(vol, dev.upload(np.ones((2, 3, 5), np.uint8)), vol, None, np.eye(3), np.zeros(3), table, 2)
        with pytest.raises(nat.LMError, match="field must be"):
            eng.pair_map_dev(vol, lab, vol, dev.upload(np.zeros((3, 2, 3, 5), np.float32)), np.eye(3), np.zeros(3), table, 2)
        with pytest.raises(nat.LMError, match="dtype"):
            eng.pair_map_dev(dev.upload(np.zeros((2, 3, 4), np.uint16)), lab, vol, None, np.eye(3), np.zeros(3), table, 2)
        with pytest.raises(nat.LMError, match="table"):
            eng.pair_map_dev(vol, lab, vol, None, np.eye(3), np.zeros(3), table, 3)
        with pytest.raises(nat.LMError, match="classes"):
            eng.pair_map_dev(vol, lab, vol, None, np.eye(3), np.zeros(3), table, 2, classes=chg)
        with pytest.raises(ValueError, match="n_labels"):
            eng.pair_map_dev(vol, lab, vol, None, np.eye(3), np.zeros(3), table, 17)
        with pytest.raises(ValueError, match="keep"):
            eng.pair_map_dev(vol, lab, vol, None, np.eye(3), np.zeros(3), table, 2, keep=(256,))
    with pytest.raises(nat.LMError, match="too large"):
        eng.pair_map(np.zeros((1, 1, 4097), np.int16), np.zeros((1, 1, 4097), np.uint8), np.zeros((1, 1, 1), np.int16), None, np.eye(3), np.zeros(3), 2)
    with pytest.raises(ValueError, match="maps"):
        eng.pair_map(np.zeros((1, 1, 2), np.int16), np.zeros((1, 1, 2), np.uint8), np.zeros((1, 1, 1), np.int16), None, np.eye(3), np.zeros(3), 2,
                     maps=("labels",))


def test_host_form(emu_engine):
    fixed, moving, labels = lungish((2, 3, 5), np.int16, 50), lungish((4, 2, 7), np.int16, 51), labels_of((2, 3, 5), 52, 3)
    A, b = rot_scale()
    field = make_field("random", (2, 3, 5), 53)
    table, out = emu_engine.pair_map(fixed, labels, moving, field, A, b, 3, maps=("classes", "jacobian"), jac_scale=0.5)
    want_table, want = pair_map_oracle(fixed, labels, moving, field, A, b, 3, jac_scale=0.5)
    assert table.dtype == np.int64 and table.tolist() == want_table and sorted(out) == ["classes", "jacobian"]
    assert all(same_bits(out[k], want[k]) for k in out)
