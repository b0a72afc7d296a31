"""lm_seed_cost_dev and lm_airway_mask_dev on the emulator engine against numpy restatements of the header's definitions, bit for
bit, and the airway segmentation on a synthetic phantom.

`cost_oracle` is the definition with a heap (the minimax path cost is what Dijkstra's algorithm computes with max in the place of +);
`cost_jacobi` is the plain fixed-point iteration over the whole volume, an independent second restatement used on the smallest case.
The cases are chosen for where a tiled relaxation goes wrong (the brick is 8 x 8 x 32 voxels): extents one voxel past a brick face, a
corridor that crosses one face many times, regions that touch only across a brick edge or corner, seeds on a brick corner and in the
last voxel, dense ties.  The oracles, the cases, the runners and the phantom are shared with tests/test_gpu_airway.py.

The phantom (`phantom()`, 64 x 72 x 72 voxels of 1 mm, fixed seed): outside air around a body, two ellipsoid lungs at -860 HU, a
five-generation binary tube tree with radius 3.6 x 0.72^g, walls at -100 HU (-750 HU where the radius is below 1.5), lumen at -990,
-970, -940, -900, -860 HU by generation with N(0, 25) noise.  Measured on it (the numpy oracle and the engine agree bit for bit, so
the figures are both's; test_phantom_quality prints them, PHANTOM_MEASURED holds them): threshold -830 HU, first leaking threshold
-820, 2384 mask voxels, none outside the true lumen grown by one voxel; lumen recall by generation 1.0, 1.0, 1.0, 1.0, 0.597 (the
deep generations are not barred); 17 rounds of the flood; the tree has 1, 2, 4, 8, 6 segments by generation after 29 spurs were
pruned at spur_factor 1.5 (0.5 and 1.0: 28 spurs, 1, 2, 4, 8, 8; 2.0: as 1.5; 2.5: 31 spurs, 1, 2, 4, 8, 2 -- real twigs go).
"""
import heapq

import numpy as np
import pytest
from scipy import ndimage as ndi

from lungmask_amd import _native as nat

UNREACHED = 32767
BRICK = (8, 8, 32)
S6 = ndi.generate_binary_structure(3, 1)


# ---- oracles --------------------------------------------------------------------------------------------------------------------------
def hu_of(vol):
    """(hu int64 saturated to int32, nan) by the statistics' rule: integers as they are, floats rint (half to even)."""
    vol = np.asarray(vol)
    if vol.dtype.kind == "f":
        nan = np.isnan(vol)
        with np.errstate(invalid="ignore"):
            r = np.rint(np.where(nan, 0, vol).astype(np.float64))
        hu = np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    else:
        nan = np.zeros(vol.shape, bool)
        hu = np.clip(vol.astype(np.int64), -2 ** 31, 2 ** 31 - 1)
    return hu, nan


def x_and_passable(vol, cap_hu):
    hu, nan = hu_of(vol)
    return np.maximum(hu, -1024), ~nan & (hu <= cap_hu)


def cost_oracle(vol, seeds, cap_hu):
    """(cost int16, curve int64 [cap_hu + 1025], reached, seeds_passable) by the definition, with a heap."""
    x, ok = x_and_passable(vol, cap_hu)
    n, h, w = x.shape
    xs, oks = x.ravel().tolist(), ok.ravel().tolist()
    cost = [UNREACHED] * (n * h * w)
    heap, passable = [], 0
    for z, y, xx in seeds:
        v = (z * h + y) * w + xx
        if oks[v]:
            passable += 1
            if xs[v] < cost[v]:
                cost[v] = xs[v]
                heap.append((xs[v], v))
    heapq.heapify(heap)
    hw = h * w
    while heap:
        c, v = heapq.heappop(heap)
        if c > cost[v]:
            continue
        z, r = divmod(v, hw)
        y, xx = divmod(r, w)
        for ok_, u in ((z > 0, v - hw), (z < n - 1, v + hw), (y > 0, v - w), (y < h - 1, v + w), (xx > 0, v - 1), (xx < w - 1, v + 1)):
            if ok_ and oks[u]:
                nc = c if c > xs[u] else xs[u]
                if nc < cost[u]:
                    cost[u] = nc
                    heapq.heappush(heap, (nc, u))
    cost = np.asarray(cost, np.int16).reshape(n, h, w)
    curve = np.bincount(cost[cost != UNREACHED].astype(np.int64) + 1024, minlength=cap_hu + 1025)
    return cost, curve.astype(np.int64), int((cost != UNREACHED).sum()), passable


def cost_jacobi(vol, seeds, cap_hu):
    """(cost, sweeps): c <- max(x, min(c, the six neighbours' c)) on the whole volume until nothing changes."""
    x, ok = x_and_passable(vol, cap_hu)
    xe = np.where(ok, x, UNREACHED).astype(np.int64)
    c = np.full(x.shape, UNREACHED, np.int64)
    for s in seeds:
        if ok[tuple(s)]:
            c[tuple(s)] = xe[tuple(s)]
    sweeps = 0
    while True:
        p = np.pad(c, 1, constant_values=UNREACHED)
        m = np.minimum.reduce([c, p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1], p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1], p[1:-1, 1:-1, :-2],
                               p[1:-1, 1:-1, 2:]])
        new = np.maximum(xe, m)
        sweeps += 1
        if (new == c).all():
            return c.astype(np.int16), sweeps
        c = new


def mask_oracle(cost, threshold, lab=None):
    mask = (cost <= threshold).astype(np.uint8)
    if lab is None:
        counts = np.zeros(256, np.int64)
        counts[0] = int(mask.sum())
    else:
        counts = np.bincount(lab[mask != 0].astype(np.int64), minlength=256).astype(np.int64)
    return mask, counts


# ---- cases: name -> (volume, seeds, cap_hu) ----------------------------------------------------------------------------------------------
def noise(shape, lo, hi, seed, dtype=np.int16):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(dtype)


def serpentine():
    """(2, 24, 40): a corridor one voxel wide in the plane z = 1 that runs back and forth over the brick face between x = 31 and
    x = 32, twelve crossings; everything else is tissue.  The HU along the corridor vary, so the cost is a running maximum."""
    vol = np.full((2, 24, 40), 40, np.int16)
    path = []
    for row in range(12):
        y = 2 * row
        xs = list(range(28, 36)) if row % 2 == 0 else list(range(35, 27, -1))
        path += [(1, y, x) for x in xs]
        if row < 11:
            path.append((1, y + 1, xs[-1]))
    rng = np.random.default_rng(5)
    for v, hu in zip(path, rng.integers(-1000, -880, len(path))):
        vol[v] = hu
    return vol, [path[0]], -800, path


def edge_contact():
    """(10, 10, 34): two air blocks that touch only across a brick edge / corner (no 6-connection), and a third that is joined to
    the first by a corridor along the brick edge y = 7 | 8, z = 7 | 8."""
    vol = np.full((10, 10, 34), 40, np.int16)
    vol[6:8, 6:8, 30:32] = -950       # A: up to the corner (7, 7, 31) of brick (0, 0, 0)
    vol[8:10, 8:10, 32:34] = -940     # B: from the corner (8, 8, 32) of brick (1, 1, 1): diagonal to A only
    vol[8:10, 8:10, 20:30] = -930     # C: across the edge from the corridor below, diagonal only
    vol[7, 7, 0:30] = -960            # corridor along the edge inside brick (0, 0, 0), joined to A
    vol[8, 7, 0] = -920               # ... one step over the z face at x = 0
    vol[8, 8, 0:5] = -910             # ... and over the y face: D, reachable
    return vol, [(6, 6, 30)], -800


def float_volume():
    vol = np.random.default_rng(11).normal(-900, 120, (9, 10, 35)).astype(np.float32)
    vol[0, 0, :6] = [np.nan, np.inf, -np.inf, -5000.5, -1024.5, -1023.5]
    vol[4, 4, 4] = np.nan
    vol[8, 9, 34] = -2000.0
    vol[3, :, 17] = -999.5  # (a tie: rounds to -1000)
    return vol


def int32_volume():
    vol = noise((5, 9, 33), -1100, -700, 12, np.int32)
    vol[1, 1, 1:6] = [-100000, 100000, -2 ** 31, 2 ** 31 - 1, 40000]
    return vol


def cases():
    basins = np.full((6, 12, 40), 40, np.int16)
    basins[1:4, 1:5, 1:12] = noise((3, 4, 11), -1000, -900, 7)
    basins[2:6, 6:11, 30:39] = noise((4, 5, 9), -990, -850, 8)
    walled = noise((4, 9, 33), -1000, -900, 9)
    walled[2, 4, 16] = 500  # the seed itself is impassable
    twice = noise((9, 9, 33), -1100, 200, 6)
    twice[4, 4, 4], twice[8, 8, 32] = -900, -800
    c = {
        "odd_17_9_33": (noise((17, 9, 33), -1100, 200, 1), [(8, 4, 16)], -500),
        "flat_1_6_8": (noise((1, 6, 8), -1100, 0, 2), [(0, 3, 3)], -400),
        "long_3_4_70": (noise((3, 4, 70), -1100, 0, 3), [(1, 1, 0)], -400),
        "serpentine": serpentine()[:3],
        "edge_contact": edge_contact(),
        "seed_on_corner": (noise((10, 12, 40), -1100, 200, 4), [(8, 8, 32)], -500),
        "seed_last_voxel": (noise((10, 12, 40), -1100, 200, 4), [(9, 11, 39)], -500),
        "two_basins": (basins, [(2, 2, 2), (3, 8, 34)], -800),
        "impassable_seed": (walled, [(2, 4, 16)], -800),
        "duplicate_seed": (twice, [(4, 4, 4), (4, 4, 4), (8, 8, 32)], -500),
        "ties_cap_low": (noise((9, 10, 34), -1030, -1018, 13), [(0, 0, 0), (8, 9, 33), (4, 5, 17)], -1023),
        "ties_cap_mid": (noise((9, 10, 34), -1003, -997, 14), [(4, 5, 17)], -999),
        "noise_cap_high": (noise((9, 10, 34), -1100, 3300, 15), [(4, 5, 17), (0, 0, 0)], 3071),
        "float32": (float_volume(), [(4, 5, 17), (0, 0, 3)], -850),
        "int32": (int32_volume(), [(2, 4, 16), (1, 1, 1)], 3071),
        "int64": (noise((3, 9, 33), -1100, -600, 16, np.int64), [(1, 4, 16)], -800),
        "float64": (float_volume().astype(np.float64), [(4, 5, 17)], -900),
    }
    return c


CASES = cases()


def run_cost_case(eng, name):
    """The engine's (cost, curve, info) of a case, checked against the heap oracle bit for bit."""
    vol, seeds, cap = CASES[name]
    cost, curve, info = eng.seed_cost(vol, seeds, cap_hu=cap)
    want, want_curve, reached, passable = cost_oracle(vol, seeds, cap)
    assert cost.dtype == np.int16 and cost.shape == vol.shape
    np.testing.assert_array_equal(cost, want)
    np.testing.assert_array_equal(curve, want_curve)
    assert info["reached"] == reached == int(curve.sum())
    assert info["seeds_passable"] == passable
    assert info["converged"] is True
    x, ok = x_and_passable(vol, cap)
    hit = cost != UNREACHED
    assert (cost[hit] >= x[hit]).all() and ok[hit].all()
    return cost, curve, info


def run_mask_case(eng, name):
    vol, seeds, cap = CASES[name]
    want = cost_oracle(vol, seeds, cap)[0]
    lab = np.random.default_rng(21).integers(0, 7, vol.shape).astype(np.uint8)
    lab[0, 0, 0] = 255
    reached = np.sort(want[want != UNREACHED])
    thresholds = [-32768, 32766] + ([int(reached[len(reached) // 2]), int(reached[-1])] if len(reached) else [])
    with eng.scope() as dev:
        cd, ld = dev.upload(want), dev.upload(lab)
        for t in thresholds:
            for labels, labels_dev in ((None, None), (lab, ld)):
                mask, counts = eng.airway_mask_dev(cd, t, lab=labels_dev)
                dev.add(mask)
                want_mask, want_counts = mask_oracle(want, t, labels)
                np.testing.assert_array_equal(mask.download(), want_mask)
                np.testing.assert_array_equal(counts, want_counts)


# ---- the kernels against the oracles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_cost_matches_oracle(emu_engine, name):
    run_cost_case(emu_engine, name)


def test_jacobi_restatement_agrees_with_heap():
    vol, seeds, cap = CASES["flat_1_6_8"]
    np.testing.assert_array_equal(cost_jacobi(vol, seeds, cap)[0], cost_oracle(vol, seeds, cap)[0])
    vol, seeds, cap = CASES["edge_contact"]
    np.testing.assert_array_equal(cost_jacobi(vol, seeds, cap)[0], cost_oracle(vol, seeds, cap)[0])


def test_smallest_case_matches_jacobi(emu_engine):
    vol, seeds, cap = CASES["flat_1_6_8"]
    np.testing.assert_array_equal(emu_engine.seed_cost(vol, seeds, cap_hu=cap)[0], cost_jacobi(vol, seeds, cap)[0])


def check_serpentine(eng):
    vol, seeds, cap, path = serpentine()
    cost, _, info = run_cost_case(eng, "serpentine")
    assert info["rounds"] > 1  # the corridor crosses the face twelve times: one round cannot finish it
    running = np.maximum.accumulate([int(vol[v]) for v in path])
    assert [int(cost[v]) for v in path] == running.tolist()
    assert info["reached"] == len(path)
    with pytest.raises(nat.LMError, match="max_rounds"):
        eng.seed_cost(vol, seeds, cap_hu=cap, max_rounds=1)
    again = eng.seed_cost(vol, seeds, cap_hu=cap, max_rounds=info["rounds"])  # exactly enough, and the engine is usable after the error
    np.testing.assert_array_equal(again[0], cost)


def test_serpentine_needs_rounds_and_max_rounds_stops(emu_engine):
    check_serpentine(emu_engine)


def check_edge_contact(eng):
    vol, seeds, cap = CASES["edge_contact"]
    cost = run_cost_case(eng, "edge_contact")[0]
    assert (cost[8:10, 8:10, 32:34] == UNREACHED).all()  # B: diagonal across the corner
    assert (cost[8:10, 8:10, 20:30] == UNREACHED).all()  # C: diagonal across the edge
    assert (cost[8, 8, 0:5] == -910).all()               # D: through two faces
    assert (cost[6:8, 6:8, 30:32] == -950).all()


def test_no_diagonal_passage_over_brick_edges(emu_engine):
    check_edge_contact(emu_engine)


def test_impassable_seed_reaches_nothing(emu_engine):
    cost, curve, info = run_cost_case(emu_engine, "impassable_seed")
    assert (cost == UNREACHED).all() and curve.sum() == 0
    assert info == {"rounds": 0, "reached": 0, "seeds_passable": 0, "converged": True}


def test_two_basins_and_duplicate(emu_engine):
    cost, _, info = run_cost_case(emu_engine, "two_basins")
    assert info["seeds_passable"] == 2 and (cost[1:4, 1:5, 1:12] != UNREACHED).all() and (cost[2:6, 6:11, 30:39] != UNREACHED).all()
    assert run_cost_case(emu_engine, "duplicate_seed")[2]["seeds_passable"] == 3


def check_cap_monotone(eng):
    vol, seeds, _ = CASES["odd_17_9_33"]
    low = eng.seed_cost(vol, seeds, cap_hu=-700)[0]
    high = eng.seed_cost(vol, seeds, cap_hu=-300)[0]
    hit = low != UNREACHED
    np.testing.assert_array_equal(high[hit], low[hit])
    assert (high != UNREACHED).sum() > hit.sum()


def test_cost_is_monotone_under_the_cap(emu_engine):
    check_cap_monotone(emu_engine)


def check_mask_is_seed_component(eng):
    vol, seeds, cap = CASES["odd_17_9_33"]
    cost = eng.seed_cost(vol, seeds, cap_hu=cap)[0]
    x, ok = x_and_passable(vol, cap)
    for t in (-900, -700, cap):
        comp, _ = ndi.label(ok & (x <= t), structure=S6)
        k = comp[tuple(seeds[0])]
        want = (comp == k) if k else np.zeros(vol.shape, bool)
        np.testing.assert_array_equal(cost <= t, want)


def test_mask_is_the_seed_component_of_the_threshold(emu_engine):
    check_mask_is_seed_component(emu_engine)


@pytest.mark.parametrize("name", ["odd_17_9_33", "flat_1_6_8", "impassable_seed", "float32"])
def test_mask_and_counts(emu_engine, name):
    run_mask_case(emu_engine, name)


def check_history_independent(eng, name="odd_17_9_33"):
    vol, seeds, cap = CASES[name]
    runs = [eng.seed_cost(vol, seeds, cap_hu=cap) for _ in range(3)]
    eng.debug_fill_workspaces(0xA5)
    runs.append(eng.seed_cost(vol, seeds, cap_hu=cap))
    eng.debug_fill_workspaces(0x00)
    runs.append(eng.seed_cost(vol, seeds, cap_hu=cap))
    for cost, curve, info in runs[1:]:
        assert cost.tobytes() == runs[0][0].tobytes() and curve.tobytes() == runs[0][1].tobytes()
        assert info["reached"] == runs[0][2]["reached"]


def test_three_runs_and_filled_workspaces_give_identical_bytes(emu_engine):
    check_history_independent(emu_engine)
    check_history_independent(emu_engine, "serpentine")


def test_fill_workspaces_covers_the_airway_workspace(emu_engine):
    vol, seeds, cap = CASES["odd_17_9_33"]
    emu_engine.seed_cost(vol, seeds, cap_hu=cap)
    bricks, brick = emu_engine.seed_cost_bricks(vol.shape)
    assert brick == BRICK and bricks == 3 * 2 * 2
    assert emu_engine.debug_fill_workspaces(1) >= vol.size * 2 + bricks * 12


def test_argument_checks(emu_engine):
    eng = emu_engine
    vol = CASES["flat_1_6_8"][0]
    with pytest.raises(ValueError, match="cap_hu"):
        eng.seed_cost(vol, [(0, 0, 0)], cap_hu=-1024)
    with pytest.raises(ValueError, match="cap_hu"):
        eng.seed_cost(vol, [(0, 0, 0)], cap_hu=3072)
    with pytest.raises(ValueError, match="outside"):
        eng.seed_cost(vol, [(0, 6, 0)])
    with pytest.raises(ValueError, match="seeds"):
        eng.seed_cost(vol, [])
    with pytest.raises(ValueError, match="seeds"):
        eng.seed_cost(vol, [(0, 0)])
    with pytest.raises(ValueError, match="1 to 64"):
        eng.seed_cost(vol, [(0, 0, 0)] * 65)
    with pytest.raises(ValueError, match="max_rounds"):
        eng.seed_cost(vol, [(0, 0, 0)], max_rounds=-1)
    with pytest.raises(nat.LMError, match="dtype"):
        eng.seed_cost(vol.astype(np.uint8), [(0, 0, 0)])
    with pytest.raises(nat.LMError, match="3-D"):
        eng.seed_cost(vol[0], [(0, 0, 0)])
    with eng.scope() as dev:
        vd = dev.upload(vol)
        with pytest.raises(nat.LMError, match="out must be"):
            eng.seed_cost_dev(vd, [(0, 0, 0)], out=vd)
        cost = dev.add(eng.seed_cost_dev(vd, [(0, 0, 0)])[0])
        with pytest.raises(ValueError, match="threshold"):
            eng.airway_mask_dev(cost, 32767)
        with pytest.raises(nat.LMError, match="int16"):
            eng.airway_mask_dev(dev.upload(vol.astype(np.int32)), 0)
        with pytest.raises(nat.LMError, match="u8"):
            eng.airway_mask_dev(cost, 0, lab=cost)


# ---- the phantom ------------------------------------------------------------------------------------------------------------------------
PHANTOM_SHAPE = (64, 72, 72)
GEN_RADIUS = [3.6 * 0.72 ** g for g in range(5)]
GEN_HU = [-990, -970, -940, -900, -860]
GEN_LENGTH = [24.0, 15.0, 11.0, 8.0, 6.0]


def _branches():
    """The tube tree as (generation, start, end) in (z, y, x): the trachea comes in through the top slice, every branch forks into
    two children turned by +-38 degrees, in the z-x plane at even generations and in the z-y plane at odd ones."""
    out = []

    def grow(g, start, direction):
        end = start + direction * GEN_LENGTH[g]
        out.append((g, start, end))
        if g == 4:
            return
        axis = 2 if g % 2 == 0 else 1
        for sign in (-1.0, 1.0):
            a = np.deg2rad(38.0) * sign
            d = direction.copy()
            d[0] = direction[0] * np.cos(a) - direction[axis] * np.sin(a)
            d[axis] = direction[0] * np.sin(a) + direction[axis] * np.cos(a)
            grow(g + 1, end, d / np.linalg.norm(d))

    grow(0, np.array([-3.0, 36.0, 36.0]), np.array([1.0, 0.0, 0.0]))
    return out


def _distance_to_segment(grid, a, b):
    ab = b - a
    t = np.clip(((grid - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(grid - (a + t[..., None] * ab), axis=-1)


_PHANTOM = {}


def phantom():
    """(image int16, labels u8, lumen_generation int8 [-1: no lumen], spacing): see the module's head."""
    if _PHANTOM:
        return _PHANTOM["v"]
    n, h, w = PHANTOM_SHAPE
    z, y, x = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    grid = np.stack([z, y, x], axis=-1)
    vol = np.full(PHANTOM_SHAPE, 40.0)
    vol[((y - 35.5) / 33.0) ** 2 + ((x - 35.5) / 34.0) ** 2 > 1.0] = -1000.0  # outside air: it touches every y and x border
    lab = np.zeros(PHANTOM_SHAPE, np.uint8)
    for k, cx in ((1, 19.0), (2, 52.0)):
        lung = ((z - 40.0) / 21.0) ** 2 + ((y - 36.0) / 21.0) ** 2 + ((x - cx) / 14.0) ** 2 <= 1.0
        vol[lung] = -860.0
        lab[lung] = k
    gen = np.full(PHANTOM_SHAPE, -1, np.int8)
    dist = [(g, _distance_to_segment(grid, a, b)) for g, a, b in _branches()]
    for g, d in dist:  # the walls first, so that the lumen stays open at the forks
        r = GEN_RADIUS[g]
        vol[d <= r + (1.5 if r >= 1.5 else 1.2)] = -100.0 if r >= 1.5 else -750.0
    for g, d in sorted(dist, key=lambda t: -t[0]):  # (a voxel of two lumina belongs to the earlier generation)
        inside = d <= GEN_RADIUS[g]
        vol[inside] = GEN_HU[g]
        gen[inside] = g
    lab[gen >= 0] = 0  # the networks leave the airways out of their labels
    lab[(vol == -100.0)] = 0
    vol += np.random.default_rng(2024).normal(0.0, 25.0, PHANTOM_SHAPE)
    _PHANTOM["v"] = (np.rint(vol).astype(np.int16), lab, gen, (1.0, 1.0, 1.0))
    return _PHANTOM["v"]


# ---- quality on the phantom ---------------------------------------------------------------------------------------------------------------
PHANTOM_SEED = (0, 33, 35)  # the first voxel of the trachea's air: what find_trachea picks
PHANTOM_MEASURED = {"threshold": -830, "first_leaking": -820, "voxels": 2384, "recall": [1.0, 1.0, 1.0, 1.0, 0.597],
                    "segments_per_generation": [1, 2, 4, 8, 6], "pruned_spurs": 29, "rounds": 17}
DILATE = np.ones((3, 3, 3), bool)


def phantom_oracle():
    """The numpy oracle alone on the phantom: (cost, curve, the rule's choice)."""
    from lungmask_amd import airways as aw

    if "oracle" not in _PHANTOM:
        img = phantom()[0]
        cost, curve, _, _ = cost_oracle(img, [PHANTOM_SEED], -800)
        _PHANTOM["oracle"] = (cost, curve, aw.choose_threshold(curve, 1e-3))
    return _PHANTOM["oracle"]


def recall_by_generation(mask, gen):
    return [float((mask & (gen == g)).sum() / (gen == g).sum()) for g in range(5)]


def test_phantom_meets_the_conditions_by_the_oracle_alone():
    _, _, gen, _ = phantom()
    cost, _, chosen = phantom_oracle()
    assert chosen["first_leaking"] is not None and -950 <= chosen["threshold"] < chosen["first_leaking"]
    mask = cost <= chosen["threshold"]
    assert not (mask & ~ndi.binary_dilation(gen >= 0, structure=DILATE)).any()
    assert min(recall_by_generation(mask, gen)[:3]) >= 0.95
    assert mask.sum() == chosen["voxels"] and (cost <= chosen["first_leaking"]).sum() > 10 * mask.sum()  # the leak is the lungs


def check_phantom_quality(eng):
    from lungmask_amd import airways as aw

    img, lab, gen, sp = phantom()
    cost, curve, chosen = phantom_oracle()
    trachea = aw.find_trachea(img, lab, spacing=sp, engine=eng)
    assert trachea["index"] == PHANTOM_SEED and gen[trachea["index"]] == 0  # the trachea, not the outside air the phantom holds
    assert trachea["rejected"]["touches_border"] >= 1
    res = aw.segment_airways(img, lab, spacing=sp, names={1: "left", 2: "right"}, engine=eng)
    np.testing.assert_array_equal(res.cost, cost)  # the same bits as the oracle's
    np.testing.assert_array_equal(res.curve, curve)
    assert res.threshold == chosen["threshold"] and res.analysis["first_leaking"] == chosen["first_leaking"]
    np.testing.assert_array_equal(res.mask, (cost <= chosen["threshold"]).astype(np.uint8))
    mask = res.mask != 0
    recall = recall_by_generation(mask, gen)
    per_gen = [g["segments"] for g in res.tree["generations"]]
    print("phantom: threshold", res.threshold, "first leaking", res.analysis["first_leaking"], "voxels", int(mask.sum()), "rounds",
          res.analysis["rounds"], "recall by generation", [round(r, 3) for r in recall], "segments by generation", per_gen, "spurs pruned",
          res.tree["totals"]["pruned_spurs"])
    assert -950 <= res.threshold < chosen["first_leaking"]
    assert not (mask & ~ndi.binary_dilation(gen >= 0, structure=DILATE)).any()
    assert min(recall[:3]) >= 0.95
    assert per_gen[:3] == [1, 2, 4]
    assert res.tree["totals"]["cycles"] == 0 and res.tree["totals"]["unreached_segments"] == 0
    assert res.analysis["by_label"]["0"]["voxels"] == int(mask.sum()) and res.analysis["volume_ml"] == pytest.approx(mask.sum() * 1e-3)
    assert res.analysis["error"] is None and res.seed == [list(PHANTOM_SEED)]
    import json

    assert json.loads(json.dumps(res.meta())) == res.meta()
    return res


def test_phantom_quality(emu_engine):
    res = check_phantom_quality(emu_engine)
    assert res.threshold == PHANTOM_MEASURED["threshold"] and res.analysis["voxels"] == PHANTOM_MEASURED["voxels"]
    assert [g["segments"] for g in res.tree["generations"]] == PHANTOM_MEASURED["segments_per_generation"]
