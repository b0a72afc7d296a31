"""lm_skeleton_dev, lm_skeleton_points_dev and lm_calibre_dev on the emulator engine against a numpy restatement of the header's
definitions, bit for bit.  The oracle labels every 3 x 3 x 3 neighbourhood with scipy.ndimage.label (26-connected object voxels of
N26, 6-connected background voxels of N18) and walks the 48 sub-steps of a pass over the WHOLE volume, deciding every sub-step on a
snapshot of its start; the calibre oracle composes test_metrics_emu's oracle_edt and test_morph_emu's oracle_nearest.  The oracle
and the case functions are shared with tests/test_gpu_skeleton.py."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

from lungmask_amd import _native as nat
from tests.test_metrics_emu import oracle_edt
from tests.test_morph_emu import oracle_nearest, table

S26 = np.ones((3, 3, 3), bool)
S6 = ndi.generate_binary_structure(3, 1)
N18 = ndi.generate_binary_structure(3, 2).copy()
N18[1, 1, 1] = False
N6 = S6.copy()
N6[1, 1, 1] = False
DIRECTIONS = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]  # -z, +z, -y, +y, -x, +x
WEIGHTS = (1 << np.arange(27)).reshape(3, 3, 3)


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def simple_word(word: int) -> bool:
    """The header's simple-point test of the neighbourhood whose voxel (dz, dy, dx) is bit (dz + 1) * 9 + (dy + 1) * 3 + dx + 1."""
    obj = ((word >> np.arange(27)) & 1).astype(bool).reshape(3, 3, 3)
    obj[1, 1, 1] = False
    if ndi.label(obj, structure=S26)[1] != 1:
        return False
    bg = ~obj & N18
    lab = ndi.label(bg, structure=S6)[0]
    return len(set(lab[bg & N6].tolist())) == 1


def oracle_skeleton(sel: np.ndarray, keep=None):
    """(codes u8, info) of lm_skeleton_dev by the definition, on the whole volume padded with background."""
    S = table(keep)[sel]
    n, h, w = S.shape
    P = np.zeros((n + 2, h + 2, w + 2), bool)
    P[1:-1, 1:-1, 1:-1] = S
    z, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
    field = np.zeros_like(P, dtype=np.int8) - 1
    field[1:-1, 1:-1, 1:-1] = ((z & 1) << 2) | ((y & 1) << 1) | (x & 1)
    selected, passes = int(S.sum()), 0
    while True:
        passes += 1
        deleted = 0
        for d in DIRECTIONS:
            for f in range(8):
                inner = P[1:-1, 1:-1, 1:-1]
                towards = P[1 + d[0]:n + 1 + d[0], 1 + d[1]:h + 1 + d[1], 1 + d[2]:w + 1 + d[2]]
                cand = np.argwhere(inner & ~towards & (field[1:-1, 1:-1, 1:-1] == f)) + 1
                gone = []
                for cz, cy, cx in cand:  # decided on the state at the start of the sub-step
                    nb = P[cz - 1:cz + 2, cy - 1:cy + 2, cx - 1:cx + 2]
                    word = int((nb * WEIGHTS).sum()) & ~(1 << 13)
                    if bin(word).count("1") <= 1:  # end point or isolated voxel
                        continue
                    if simple_word(word):
                        gone.append((cz, cy, cx))
                for v in gone:
                    P[v] = False
                deleted += len(gone)
        if deleted == 0:
            break
    K = P[1:-1, 1:-1, 1:-1]
    count = ndi.convolve(P.astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant")[1:-1, 1:-1, 1:-1]  # the voxel and its neighbours
    codes = np.where(K, count, 0).astype(np.uint8)
    return codes, {"selected": selected, "skeleton": int(K.sum()), "passes": passes}


def topology(mask: np.ndarray):
    """(26-components of the mask, cavities = 6-components of the background of the padded volume other than the outside)."""
    return ndi.label(mask, structure=S26)[1], ndi.label(~np.pad(mask, 1), structure=S6)[1] - 1


def oracle_calibre(skel, sel, edges_mm, spacing=None, keep=None, lab=None, n_labels=16):
    """(class_out, counts, d2) of lm_calibre_dev from oracle_edt and oracle_nearest."""
    M = table(keep)[sel]
    d2 = oracle_edt((~M).astype(np.uint8), spacing)
    e2 = [np.float32(float(e) * float(e)) for e in edges_mm]
    cls = np.where(M & (skel != 0), 1 + sum((d2 >= t).astype(np.int64) for t in e2), 0).astype(np.uint8)
    near = oracle_nearest(cls, None, spacing)[1]
    out = np.where(M, near, 0).astype(np.uint8)
    rows = np.ones(sel.shape, np.int64) if lab is None else lab.astype(np.int64)
    hit = M & (rows >= 1) & (rows < n_labels)
    counts = np.bincount(rows[hit] * 9 + out[hit], minlength=n_labels * 9).reshape(n_labels, 9)
    return out, counts, d2


# ---- volumes --------------------------------------------------------------------------------------------------------------------------
def torus(shape, centre, major, minor):
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    ring = np.sqrt((y - centre[1]) ** 2 + (x - centre[2]) ** 2) - major
    return ((ring ** 2 + (z - centre[0]) ** 2) <= minor ** 2).astype(np.uint8)


def random_volume(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def shapes_volume():
    """(14, 20, 24): a tube, a branch off it, a torus, a block with a cavity and an isolated voxel."""
    v = np.zeros((14, 20, 24), np.uint8)
    v[1:4, 1:4, 1:22] = 1            # tube along x
    v[1:4, 4:10, 10:13] = 1          # branch along y
    v |= torus(v.shape, (9, 7, 7), 4.0, 1.5)
    v[6:12, 12:19, 14:22] = 1        # block ...
    v[8:10, 14:17, 17:19] = 0        # ... with a cavity
    v[12, 1, 22] = 1                 # isolated voxel
    return v


def rods_volume():
    """(5, 33, 130): rods along x, one across the whole row, on both parities of y and z, and a thick one."""
    v = np.zeros((5, 33, 130), np.uint8)
    v[0, 0, :] = 1
    v[2, 5:8, 3:127] = 1
    v[1:4, 12:15, 60:130] = 1
    v[4, 20:22, 1:70] = 1
    v[3:5, 30:33, 64:129] = 1
    return v


def faces_volume():
    """(6, 7, 8): three bars through the centre that reach all six faces."""
    v = np.zeros((6, 7, 8), np.uint8)
    v[:, 3:5, 3:5] = 1
    v[2:4, :, 3:5] = 1
    v[2:4, 3:5, :] = 1
    return v


def block_volume(shift=(0, 0, 0)):
    """The 5 x 5 x 9 block in (10, 12, 14), moved by `shift`."""
    v = np.zeros((10, 12, 14), np.uint8)
    v[2 + shift[0]:7 + shift[0], 3 + shift[1]:8 + shift[1], 2 + shift[2]:11 + shift[2]] = 1
    return v


def labelled_volume():
    """Several label values, of which one or two are kept."""
    v = np.zeros((9, 12, 13), np.uint8)
    v[1:8, 1:6, 1:12] = 3
    v[2:7, 6:11, 2:6] = 5
    v[3:6, 6:11, 6:12] = 200
    return v


CASES = {
    "random_0.2": lambda: (random_volume((9, 12, 13), 0.2, 1), None),
    "random_0.5": lambda: (random_volume((9, 12, 13), 0.5, 2), None),
    "random_0.8": lambda: (random_volume((9, 12, 13), 0.8, 3), None),
    "shapes": lambda: (shapes_volume(), None),
    "torus": lambda: (torus((7, 16, 17), (3, 8, 8), 5.0, 1.5), None),
    "everything": lambda: (np.full((4, 5, 6), 7, np.uint8), None),
    "faces": lambda: (faces_volume(), None),
    "rods": lambda: (rods_volume(), None),
    "block": lambda: (block_volume(), None),
    "block_z": lambda: (block_volume((1, 0, 0)), None),
    "block_y": lambda: (block_volume((0, 1, 0)), None),
    "block_x": lambda: (block_volume((0, 0, 1)), None),
    "keep_one": lambda: (labelled_volume(), (5,)),
    "keep_two": lambda: (labelled_volume(), (3, 200)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(sel, keep, oracle codes, oracle info), computed once per process; the arrays are read-only."""
    sel, keep = CASES[name]()
    codes, info = oracle_skeleton(sel, keep)
    sel.setflags(write=False)
    codes.setflags(write=False)
    return sel, keep, codes, info


# ---- case functions (engine: the emulator's or the device's) --------------------------------------------------------------------------
def run_thinning_case(engine, name):
    sel, keep, want, info = case(name)
    got, got_info = engine.skeleton(sel, keep, return_info=True)  # in place: out_dev == sel_dev
    assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int((got != want).sum()))
    assert got_info == info, (name, got_info, info)
    sd = engine.to_device(sel)
    try:
        out, again_info = engine.skeleton_dev(sd, keep)  # an output of its own: the input is unchanged
        assert np.array_equal(out.download(), want) and again_info == info and np.array_equal(sd.download(), sel)
        out.free()
    finally:
        sd.free()


def run_idempotent(engine, name):
    _, _, want, info = case(name)
    got, got_info = engine.skeleton(want, None, return_info=True)
    assert np.array_equal(got, want)
    assert got_info == {"selected": info["skeleton"], "skeleton": info["skeleton"], "passes": 1}


def run_points(engine, name="shapes"):
    _, _, codes, info = case(name)
    total = info["skeleton"]
    want = np.flatnonzero(codes.ravel()).astype(np.int32)
    d2 = np.random.default_rng(5).random(codes.shape).astype(np.float32)
    kd, dd = engine.to_device(codes), engine.to_device(d2)
    try:
        for cap in (None, total, total + 7, total - 5, 1, 0):
            idx, code, dist, n = engine.skeleton_points_dev(kd, dd, cap)
            m = total if cap is None else min(cap, total)
            assert n == total and idx.dtype == np.int32 and code.dtype == np.uint8 and dist.dtype == np.float32
            assert np.array_equal(idx, want[:m]) and np.array_equal(code, codes.ravel()[want[:m]])
            assert np.array_equal(dist.view(np.uint32), d2.ravel()[want[:m]].view(np.uint32))
        idx, code, dist, n = engine.skeleton_points_dev(kd)
        assert dist is None and n == total and np.array_equal(idx, want)
    finally:
        kd.free()
        dd.free()
    # more than one chunk of 4096 voxels and a last chunk that is not full
    big = np.zeros((3, 50, 61), np.uint8)
    rng = np.random.default_rng(6)
    big[rng.random(big.shape) < 0.1] = 3
    big[0, 0, 0] = big[-1, -1, -1] = 2
    kd = engine.to_device(big)
    try:
        idx, code, _, n = engine.skeleton_points_dev(kd)
        want = np.flatnonzero(big.ravel())
        assert n == want.size and np.array_equal(idx, want) and np.array_equal(code, big.ravel()[want])
    finally:
        kd.free()


CALIBRE_SPACINGS = [None, (2.5, 0.75, 1.25)]


def calibre_volume():
    """A mask of a thick and a thin tube with a branch, its skeleton codes, and labels that split it."""
    sel = np.zeros((9, 20, 26), np.uint8)
    sel[1:8, 2:9, 1:25] = 2
    sel[3:6, 9:18, 10:13] = 2
    sel[4, 12:15, 13:24] = 9
    lab = np.zeros_like(sel)
    lab[:, :, :13] = 1
    lab[:, :, 13:] = 2
    lab[0:4, 0:10, 20:] = 40  # beyond n_labels
    return sel, lab


def run_calibre(engine, spacing):
    sel, lab = calibre_volume()
    skel = engine.skeleton(sel)
    d2 = oracle_edt((sel == 0).astype(np.uint8), spacing)
    occurring = np.unique(d2[(skel != 0)])
    exact = float(np.sqrt(float(occurring[len(occurring) // 2])))  # an edge whose square IS an occurring distance
    assert np.float32(exact * exact) in occurring
    for edges, keep, labels in (((0.9, exact, 4.0), None, lab), ((1.5,), (2,), None), ((0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 1e14), None, lab)):
        want, counts, dist = oracle_calibre(skel, sel, edges, spacing, keep, labels, 16)
        got, got_counts, got_d2 = engine.calibre(skel, sel, edges, lab=labels, spacing=spacing, keep=keep, return_distance=True)
        assert np.array_equal(got, want), (edges, keep, int((got != want).sum()))
        assert got_counts.dtype == np.int64 and np.array_equal(got_counts, counts)
        assert np.array_equal(got_d2.view(np.uint32), dist.view(np.uint32))
        assert len(np.unique(want[want > 0])) >= (2 if len(edges) > 1 else 1)
    got, got_counts = engine.calibre(skel, sel, (0.9, exact), lab=lab, spacing=spacing, n_labels=2)
    want, counts, _ = oracle_calibre(skel, sel, (0.9, exact), spacing, None, lab, 2)
    assert np.array_equal(got, want) and got_counts.shape == (2, 9) and np.array_equal(got_counts, counts)
    # the whole volume is mask: every distance is +inf, every voxel of the top class
    full = np.ones((3, 4, 5), np.uint8)
    got, got_counts = engine.calibre(engine.skeleton(full), full, (1.0, 2.0), spacing=spacing)
    assert (got == 3).all() and got_counts[1, 3] == full.size and got_counts.sum() == full.size
    # no skeleton voxel inside the mask: class 0
    got, got_counts = engine.calibre(np.zeros_like(full), full, (1.0,), spacing=spacing)
    assert (got == 0).all() and got_counts[1, 0] == full.size


def run_state_rule(engine):
    """Results do not depend on what the workspaces held: filled with 0x00 and with 0xFF, and after a larger call."""
    sel, keep, want, info = case("shapes")
    csel, clab = calibre_volume()

    def results():
        codes, got_info = engine.skeleton(sel, keep, return_info=True)
        assert got_info == info
        kd = engine.to_device(codes)
        try:
            idx, code, _, _ = engine.skeleton_points_dev(kd)
        finally:
            kd.free()
        cls, counts, d2 = engine.calibre(engine.skeleton(csel), csel, (1.0, 2.0), lab=clab, return_distance=True)
        return codes, idx, code, cls, counts, d2.view(np.uint32)

    first = results()
    assert np.array_equal(first[0], want)
    big = random_volume((12, 30, 40), 0.6, 9)  # a larger call grows the workspaces
    engine.calibre(engine.skeleton(big), big, (1.0,))
    for byte in (None, 0x00, 0xFF):
        if byte is not None:
            assert engine.debug_fill_workspaces(byte) > 0
        for got, ref in zip(results(), first):
            assert np.array_equal(got, ref)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_simple_point_words():
    """The oracle's test on neighbourhoods whose answer is known."""
    def word(*offsets):
        return sum(1 << ((dz + 1) * 9 + (dy + 1) * 3 + dx + 1) for dz, dy, dx in offsets)

    assert not simple_word(word())                                  # isolated: no object neighbour
    assert simple_word(word((0, 0, 1)))                             # the end of a curve (kept as an end point, but simple)
    assert not simple_word(word((0, 0, 1), (0, 0, -1)))             # the middle of a curve
    assert simple_word(word((0, 0, 1), (0, 1, 1)))                  # two adjacent neighbours
    assert not simple_word(((1 << 27) - 1) & ~(1 << 13))            # interior: no background 6-neighbour
    assert simple_word(((1 << 27) - 1) & ~(1 << 13) & ~(1 << 4))    # a dent in a flat surface
    plane = word(*[(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)])
    assert not simple_word(plane)                                   # a sheet: two background sides


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_preserves_topology(name):
    sel, keep, codes, info = case(name)
    S = table(keep)[sel]
    assert topology(codes != 0) == topology(S), name
    assert not (codes != 0)[~S].any() and info["selected"] == int(S.sum()) and info["skeleton"] == int((codes != 0).sum())
    assert info["passes"] >= 1 and (info["passes"] > 1) == (info["skeleton"] < info["selected"])
    count = ndi.convolve((codes != 0).astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant")
    assert np.array_equal(codes, np.where(codes != 0, count, 0))


def test_oracle_torus_is_a_closed_curve():
    _, _, codes, info = case("torus")
    assert (info["selected"], info["skeleton"]) == (252, 28) and (codes[codes != 0] == 3).all()  # every voxel has two neighbours
    assert topology(codes != 0) == (1, 0)


def test_oracle_subfield_uses_the_volume_index():
    """Moving the block by one voxel moves it into the other subfields: the skeleton is not the moved skeleton for every shift, which is
    what a parity taken inside the working box would give."""
    base = case("block")[2]
    moved = [np.array_equal(np.roll(base, 1, axis), case(name)[2]) for axis, name in enumerate(("block_z", "block_y", "block_x"))]
    print("block: skeleton voxels", [case(n)[3]["skeleton"] for n in ("block", "block_z", "block_y", "block_x")], "moved equal", moved)
    assert not all(moved)
    assert case("block")[3]["skeleton"] == 9 and case("block_x")[3]["skeleton"] == 7


@pytest.mark.parametrize("name", sorted(CASES))
def test_thinning(emu_engine, name):
    run_thinning_case(emu_engine, name)


@pytest.mark.parametrize("name", ["torus", "random_0.5", "block_x"])
def test_second_call_is_identity(emu_engine, name):
    run_idempotent(emu_engine, name)


def test_points(emu_engine):
    run_points(emu_engine)


@pytest.mark.parametrize("spacing", CALIBRE_SPACINGS)
def test_calibre(emu_engine, spacing):
    run_calibre(emu_engine, spacing)


def test_state_rule(emu_engine):
    run_state_rule(emu_engine)


def test_argument_errors(emu_engine):
    sel = case("shapes")[0]
    with pytest.raises(nat.NoKeptVoxel):
        emu_engine.skeleton(np.zeros((3, 4, 5), np.uint8))
    with pytest.raises(nat.NoKeptVoxel):
        emu_engine.skeleton(sel, keep=(9,))
    with pytest.raises(nat.NoKeptVoxel):
        emu_engine.skeleton(np.zeros((0, 4, 5), np.uint8))
    skel = emu_engine.skeleton(sel)
    for edges in ((), (1.0,) * 2, (2.0, 1.0), (0.0, 1.0), (-1.0,), (1.0, float("nan")), (1e15,), tuple(range(1, 9))):
        with pytest.raises(ValueError, match="edges_mm"):
            emu_engine.calibre(skel, sel, edges)
    with pytest.raises(ValueError, match="n_labels"):
        emu_engine.calibre(skel, sel, (1.0,), n_labels=17)
    with pytest.raises(nat.LMError, match="shape"):
        emu_engine.calibre(skel, sel[1:], (1.0,))
    # the C entry points refuse the same things themselves, before anything is read
    lib, sd = emu_engine.L.lib, emu_engine.to_device(sel)
    out = emu_engine.empty(sel.shape, np.uint8)
    keep, info, total = nat.Engine._keep_table(None), (C.c_int64 * 4)(), C.c_int64()
    counts = (C.c_int64 * (16 * 9))()
    n, h, w = sel.shape

    def err():
        return lib.lm_last_error().decode()

    try:
        assert lib.lm_skeleton_dev(emu_engine.h, sd.ptr, n, h, w, nat.Engine._keep_table((9,)), out.ptr, info) == -1 and "no kept voxel" in err()
        assert lib.lm_skeleton_dev(emu_engine.h, sd.ptr, 1, 1, 4097, keep, out.ptr, info) == -1 and "too large" in err()
        assert lib.lm_skeleton_dev(emu_engine.h, sd.ptr, 2048, 2048, 512, keep, out.ptr, info) == -1 and "too large" in err()
        assert lib.lm_skeleton_dev(emu_engine.h, sd.ptr, n, h, w, keep, None, info) == -1
        assert lib.lm_skeleton_points_dev(emu_engine.h, sd.ptr, None, 1, 4097, 1, 0, None, None, None, C.byref(total)) == -1 and "too large" in err()
        assert lib.lm_skeleton_points_dev(emu_engine.h, sd.ptr, None, n, h, w, -1, None, None, None, C.byref(total)) == -1
        assert lib.lm_skeleton_points_dev(emu_engine.h, sd.ptr, None, n, h, w, 4, None, None, None, C.byref(total)) == -1

        def calibre(edges, n_labels=16, shape=(n, h, w), dst=out):
            arr = (C.c_double * max(1, len(edges)))(*edges)
            return lib.lm_calibre_dev(emu_engine.h, sd.ptr, sd.ptr, keep, None, shape[0], shape[1], shape[2], None, arr, len(edges), n_labels,
                                      dst.ptr, None, counts)

        assert calibre((1.0, 2.0)) == 0
        for edges in ((), (1.0, 1.0), (2.0, 1.0), (0.0,), (float("nan"),), (1e15,), tuple(range(1, 9))):
            assert calibre(edges) == -1 and "edges_mm" in err(), edges
        assert calibre((1.0,), n_labels=1) == -1 and calibre((1.0,), n_labels=17) == -1
        assert calibre((1.0,), shape=(4097, 1, 1)) == -1 and "too large" in err()
        assert calibre((1.0,), dst=sd) == -1  # in place
    finally:
        sd.free()
        out.free()
