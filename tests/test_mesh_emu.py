"""lm_mesh_plan_dev / lm_mesh_dev on the g++ emulation of the kernel sources, bit for bit and in order against a numpy oracle that
restates the surface-nets definition of include/lungmask_hip.h (cells, vertices, quads and their winding, Taubin smoothing), against
an unvectorised second form of it on tiny volumes, and -- independently of both -- the mesh's own properties: closedness, Euler
characteristic, orientation, enclosed volume."""
import ctypes as C
import itertools

import numpy as np
import pytest

from lungmask_amd import _native as nat
from tests.test_roi_emu import blobs, keep_table

E3 = np.eye(3, dtype=np.int64)
CORNERS = list(itertools.product((0, 1), repeat=3))
EDGES = [(p, q) for p in CORNERS for q in CORNERS if p < q and sum(abs(a - b) for a, b in zip(p, q)) == 1]  # the 12 cell edges
NEIGHBOURS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]  # -z, +z, -y, +y, -x, +x
assert len(EDGES) == 12


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle_mesh(lab, keep=None, smooth=0, lam=0.5, mu=-0.53):
    """-> (vertices float32 [V][3], quads int32 [Q][4]).  Cell (k, j, i) of the definition sits at array index (k + 1, j + 1, i + 1)."""
    sel = keep_table(keep)[lab]
    if not sel.any():
        raise ValueError("no kept voxel")
    n, h, w = lab.shape
    pad = np.zeros((n + 2, h + 2, w + 2), bool)  # the volume with its one-voxel border of unselected voxels
    pad[1:-1, 1:-1, 1:-1] = sel
    corner = {o: pad[o[0]:o[0] + n + 1, o[1]:o[1] + h + 1, o[2]:o[2] + w + 1] for o in CORNERS}
    nsel = sum(corner[o].astype(np.int64) for o in CORNERS)
    active = (nsel > 0) & (nsel < 8)
    cnt = np.zeros(active.shape, np.int64)
    s2 = np.zeros((3,) + active.shape, np.int64)
    for p, q in EDGES:
        d = corner[p] != corner[q]
        cnt += d
        for ax in range(3):
            s2[ax] += d * (p[ax] + q[ax])
    vid = np.full(active.shape, -1, np.int64)
    vid[active] = np.arange(int(active.sum()))  # raster order
    cells = np.argwhere(active)  # [V][3], raster order
    verts = np.empty((len(cells), 3), np.float32)
    den = (2 * cnt[active]).astype(np.float32)
    for ax in range(3):
        verts[:, ax] = (cells[:, ax] - 1).astype(np.float32) + s2[ax][active].astype(np.float32) / den
    # quads: the lower voxel v of a differing pair is corner 0 of the cell with v's index
    differ = np.stack([corner[(0, 0, 0)] != corner[tuple(E3[a])] for a in range(3)], axis=-1)
    at = np.argwhere(differ)  # sorted by cell raster index, then axis
    quads = np.empty((len(at), 4), np.int64)
    for a in range(3):
        b, c = [ax for ax in range(3) if ax != a]
        rows = at[:, 3] == a
        cell = at[rows, :3]
        c00 = cell - E3[b] - E3[c]  # the smallest raster index of the four cells round the edge
        ring = [c00, c00 + E3[b], c00 + E3[b] + E3[c], c00 + E3[c]]
        normal = int(np.cross(E3[b], E3[b] + E3[c])[a])  # of the ring as listed, components in (z, y, x) order: +1 or -1 along a
        lower_selected = corner[(0, 0, 0)][tuple(cell.T)]
        keep_order = (normal > 0) == lower_selected  # the normal has to point from the selected voxel to the unselected one
        ids = [vid[tuple(r.T)] for r in ring]
        quads[rows, 0] = ids[0]
        quads[rows, 1] = np.where(keep_order, ids[1], ids[3])
        quads[rows, 2] = ids[2]
        quads[rows, 3] = np.where(keep_order, ids[3], ids[1])
    assert quads.min(initial=0) >= 0
    # Taubin smoothing
    if smooth:
        nb_ids, nb_ok = [], []
        for ax, sign in NEIGHBOURS:
            face = sum(corner[o].astype(np.int64) for o in CORNERS if o[ax] == (sign > 0))[active]
            ok = (face > 0) & (face < 4)
            other = cells + sign * E3[ax]
            other = np.where(ok[:, None], other, cells)
            ids = vid[tuple(other.T)]
            assert (ids >= 0).all()
            nb_ids.append(ids)
            nb_ok.append(ok)
        count = sum(ok.astype(np.int64) for ok in nb_ok)
        assert count.min() >= 2
        countf = count.astype(np.float32)[:, None]
        for _ in range(smooth):
            for f in (np.float32(lam), np.float32(mu)):
                m = np.zeros_like(verts)
                for ids, ok in zip(nb_ids, nb_ok):
                    m = np.where(ok[:, None], m + verts[ids], m)
                avg = m / countf
                verts = verts + f * (avg - verts)
                assert verts.dtype == np.float32
    return verts, quads.astype(np.int32)


def oracle_mesh_loops(lab, keep=None):
    """The definition once more, cell by cell, for tiny volumes: the winding is decided by the cross product of the cells' positions."""
    sel = keep_table(keep)[lab]
    n, h, w = lab.shape

    def s(z, y, x):
        return bool(0 <= z < n and 0 <= y < h and 0 <= x < w and sel[z, y, x])

    vid, verts = {}, []
    for k, j, i in itertools.product(range(-1, n), range(-1, h), range(-1, w)):
        crossing = [(p, q) for p, q in EDGES if s(k + p[0], j + p[1], i + p[2]) != s(k + q[0], j + q[1], i + q[2])]
        if not crossing:
            continue
        vid[(k, j, i)] = len(verts)
        base = (k, j, i)
        verts.append([np.float32(base[d]) + np.float32(sum(p[d] + q[d] for p, q in crossing)) / np.float32(2 * len(crossing))
                      for d in range(3)])
    quads = []
    for k, j, i in itertools.product(range(-1, n), range(-1, h), range(-1, w)):
        v = np.array([k, j, i])
        for a in range(3):
            u = v + E3[a]
            if s(*v) == s(*u):
                continue
            b, c = [ax for ax in range(3) if ax != a]
            ring = [v - E3[b] - E3[c], v - E3[c], v, v - E3[b]]
            nrm = np.cross(ring[1] - ring[0], ring[2] - ring[0])
            out = (u - v) if s(*v) else (v - u)
            if np.dot(nrm, out) < 0:
                ring = [ring[0], ring[3], ring[2], ring[1]]
            assert np.dot(np.cross(ring[1] - ring[0], ring[2] - ring[0]), out) > 0
            quads.append([vid[tuple(int(t) for t in r)] for r in ring])
    return np.array(verts, np.float32).reshape(-1, 3), np.array(quads, np.int32).reshape(-1, 4)


def same_mesh(got, want):
    gv, gq = got[0], got[1]
    wv, wq = want
    return (gv.dtype == np.float32 and gq.dtype == np.int32 and gv.shape == wv.shape and gq.shape == wq.shape and
            np.array_equal(gv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(gq, wq))


def check(eng, lab, what="", **kw):
    want = oracle_mesh(lab, **kw)
    got = eng.mesh(lab, **kw)
    assert got[2]["n_vertices"] == len(want[0]) and got[2]["n_quads"] == len(want[1]), (what, got[2], len(want[0]), len(want[1]))
    assert np.array_equal(got[1], want[1]), what
    assert same_mesh(got, want), (what, int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum()), "of", got[0].size, "differ")
    return got


def noise(shape, seed=0):
    return (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)


def ball(size, radius, cavity=0.0):
    g = np.arange(size, dtype=np.float64) - (size - 1) / 2
    r2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    return ((r2 <= radius * radius) & ((r2 > cavity * cavity) | (cavity <= 0))).astype(np.uint8)


def triangles(quads):
    return np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])


def signed_volume(verts, quads):
    p = verts.astype(np.float64)[triangles(quads)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def directed_sides(quads):
    a = np.concatenate([quads[:, [k, (k + 1) % 4]] for k in range(4)]).astype(np.int64)
    return a


def side_counts(sides):
    key, counts = np.unique(sides[:, 0] * (1 << 32) + sides[:, 1], return_counts=True)
    return dict(zip(key.tolist(), counts.tolist()))


def is_closed(quads):
    sides = directed_sides(quads)
    return side_counts(sides) == side_counts(sides[:, ::-1])


def euler(verts, quads):
    sides = np.sort(directed_sides(quads), axis=1)
    return len(verts) - len(np.unique(sides, axis=0)) + len(quads)


def cell_counts(lab, keep=None):
    """(cells with all 8 corners selected, active cells)."""
    sel = keep_table(keep)[lab]
    pad = np.pad(sel, 1)
    n, h, w = lab.shape
    nsel = sum(pad[o[0]:o[0] + n + 1, o[1]:o[1] + h + 1, o[2]:o[2] + w + 1].astype(np.int64) for o in CORNERS)
    return int((nsel == 8).sum()), int(((nsel > 0) & (nsel < 8)).sum())


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_single_voxel_and_full_unit_volume(emu_engine):
    lab = np.zeros((3, 3, 3), np.uint8)
    lab[1, 1, 1] = 1
    verts, quads, info = check(emu_engine, lab, "single voxel")
    assert same_mesh((verts, quads), oracle_mesh_loops(lab))
    assert len(verts) == 8 and len(quads) == 6 and info["bbox"] == [1, 2, 1, 2, 1, 2]
    third = np.float32(1) / np.float32(6)  # a cube of side 1/3 round the voxel's centre
    assert np.allclose(np.abs(verts - 1.0), third, atol=1e-6) and abs(signed_volume(verts, quads) - 1 / 27) < 1e-6
    one = np.ones((1, 1, 1), np.uint8)
    verts, quads, _ = check(emu_engine, one, "(1, 1, 1)")
    assert same_mesh((verts, quads), oracle_mesh_loops(one)) and len(verts) == 8 and len(quads) == 6


@pytest.mark.parametrize("keep", [[1], [2], None])
def test_blobs_each_label_and_both(emu_engine, keep):
    lab = blobs((11, 37, 45), 2)
    assert (lab == 1).any() and (lab == 2).any()
    verts, quads, _ = check(emu_engine, lab, keep, keep=keep)
    assert is_closed(quads) and signed_volume(verts, quads) > 0


def test_selection_touching_all_six_borders(emu_engine):
    lab = np.ones((7, 9, 11), np.uint8)
    verts, quads, info = check(emu_engine, lab, "full")
    assert info["bbox"] == [0, 7, 0, 9, 0, 11] and is_closed(quads) and euler(verts, quads) == 2
    assert verts.min() < 0 and verts[:, 0].max() > 6 and verts[:, 2].max() > 10


def test_noise_non_manifold(emu_engine):
    lab = noise((6, 7, 8))
    verts, quads, _ = check(emu_engine, lab, "noise")
    assert same_mesh((verts, quads), oracle_mesh_loops(lab))
    sides = side_counts(directed_sides(quads))
    assert max(sides.values()) >= 2  # an edge shared by four quads: the non-manifold configurations are there
    assert is_closed(quads)
    full, act = cell_counts(lab)
    assert full <= signed_volume(verts, quads) <= full + act


@pytest.mark.parametrize("shape", [(3, 70, 130), (24, 96, 128)])
def test_noise_several_workgroups(emu_engine, shape):
    lab = noise(shape, 1)
    verts, quads, info = check(emu_engine, lab, shape)
    assert info["n_vertices"] > 20000  # more than one scan block, several workgroups, several 64-cell chunks per row
    assert is_closed(quads)
    full, act = cell_counts(lab)
    assert full <= signed_volume(verts, quads) <= full + act


def test_keep_tables(emu_engine):
    lab = blobs((9, 33, 40), 13, n_labels=6)
    assert set(np.unique(lab)) >= {2, 5}
    boxes = [check(emu_engine, lab, keep, keep=keep)[2]["bbox"] for keep in ([2], [5], [2, 5])]
    assert boxes[0] != boxes[1]
    a, b = emu_engine.mesh(lab, keep=[2, 5]), emu_engine.mesh(((lab == 2) | (lab == 5)).astype(np.uint8))
    assert same_mesh(a, b[:2])


@pytest.mark.parametrize("smooth", [1, 3])
@pytest.mark.parametrize("factors", [None, (0.33, -0.34)])
def test_smoothing(emu_engine, smooth, factors):
    kw = {} if factors is None else {"lam": factors[0], "mu": factors[1]}
    for lab in (blobs((11, 37, 45), 2), noise((6, 7, 8)), noise((3, 70, 130), 1)):
        verts, quads, _ = check(emu_engine, lab, (smooth, factors), smooth=smooth, **kw)
        plain = emu_engine.mesh(lab)
        assert np.array_equal(quads, plain[1]) and not np.array_equal(verts, plain[0])  # smoothing leaves the quads unchanged


def test_ball_properties(emu_engine):
    for lab, chi in ((ball(15, 6.2), 2), (ball(17, 7.3, cavity=3.1), 4)):
        verts, quads, _ = check(emu_engine, lab, chi)
        assert euler(verts, quads) == chi
        assert is_closed(quads) and max(side_counts(directed_sides(quads)).values()) == 1
        vol = signed_volume(verts, quads)
        full, act = cell_counts(lab)
        assert vol > 0 and full <= vol <= full + act
        p = verts.astype(np.float64)[triangles(quads)]
        area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
        assert area.min() > 1e-6  # no triangle has zero area
        sm = emu_engine.mesh(lab, smooth=3)
        assert np.array_equal(sm[1], quads) and signed_volume(sm[0], sm[1]) > 0


def test_blobs_properties(emu_engine):
    lab = blobs((11, 37, 45), 2)
    verts, quads, _ = emu_engine.mesh(lab)
    full, act = cell_counts(lab)
    assert is_closed(quads) and full <= signed_volume(verts, quads) <= full + act
    p = verts.astype(np.float64)[triangles(quads)]
    assert np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).min() > 1e-6


def test_empty_selection(emu_engine):
    lab = np.zeros((4, 10, 12), np.uint8)
    with pytest.raises(ValueError, match="no voxel"):
        emu_engine.mesh(lab)
    lab[1, 2, 3] = 2
    with pytest.raises(ValueError, match="no voxel"):
        emu_engine.mesh(lab, keep=[1])
    ld = emu_engine.to_device(lab)
    bb = (C.c_int32 * 6)()
    nv, nq = C.c_int64(-5), C.c_int64(-5)
    lib = emu_engine.L.lib
    assert lib.lm_mesh_plan_dev(emu_engine.h, ld.ptr, 4, 10, 12, nat.Engine._keep_table([1]), bb, C.byref(nv), C.byref(nq)) < 0
    assert b"no kept voxel" in lib.lm_last_error() and nv.value == 0 and nq.value == 0
    buf = emu_engine.empty((8, 4), np.int32)
    assert lib.lm_mesh_dev(emu_engine.h, ld.ptr, 4, 10, 12, nat.Engine._keep_table([1]), 0, 0.5, -0.53, buf.ptr, 8, buf.ptr, 8) < 0
    assert b"no kept voxel" in lib.lm_last_error()
    assert lib.lm_mesh_plan_dev(emu_engine.h, ld.ptr, 4, 10, 12, nat.Engine._keep_table([2]), bb, C.byref(nv), C.byref(nq)) == 0
    assert list(bb) == [1, 2, 2, 3, 3, 4] and (nv.value, nq.value) == (8, 6)
    ld.free()
    buf.free()


def test_capacities_one_too_small(emu_engine):
    lab = blobs((9, 30, 33), 4)
    want = oracle_mesh(lab)
    nv, nq = len(want[0]), len(want[1])
    ld = emu_engine.to_device(lab)
    lib = emu_engine.L.lib
    table = nat.Engine._keep_table(None)
    guard = np.float32(-777.0)
    for vcap, qcap, planned in ((nv - 1, nq, True), (nv, nq - 1, True), (nv - 1, nq, False), (nv, nq, True), (nv, nq, False)):
        vd = emu_engine.to_device(np.full((nv + 4, 3), guard, np.float32))
        qd = emu_engine.to_device(np.full((nq + 4, 4), -777, np.int32))
        if planned:
            bbox, pv, pq = emu_engine.mesh_plan_dev(ld)
            assert (pv, pq) == (nv, nq)
        rc = lib.lm_mesh_dev(emu_engine.h, ld.ptr, 9, 30, 33, table, 0, 0.5, -0.53, vd.ptr, vcap, qd.ptr, qcap)
        emu_engine.sync()
        v, q = vd.download(), qd.download()
        if vcap < nv or qcap < nq:
            assert rc < 0 and b"capacity" in lib.lm_last_error()
            assert (v == guard).all() and (q == -777).all()  # nothing is written
        else:
            assert rc == 0 and same_mesh((v[:nv], q[:nq]), want)
            assert (v[nv:] == guard).all() and (q[nq:] == -777).all()  # nothing past the counts
        vd.free()
        qd.free()
    ld.free()


def test_limits_refused_before_anything_is_read(emu_engine):
    lib = emu_engine.L.lib
    bb = (C.c_int32 * 6)()
    nv, nq = C.c_int64(0), C.c_int64(0)
    table = nat.Engine._keep_table(None)
    for n, h, w in ((4097, 2, 2), (2, 4097, 2), (2, 2, 4097), (2048, 1024, 1024)):
        assert lib.lm_mesh_plan_dev(emu_engine.h, 8, n, h, w, table, bb, C.byref(nv), C.byref(nq)) < 0  # (the pointer is never used)
        assert b"too large" in lib.lm_last_error()
        assert lib.lm_mesh_dev(emu_engine.h, 8, n, h, w, table, 0, 0.5, -0.53, 8, 1, 8, 1) < 0
        assert b"too large" in lib.lm_last_error()
    with pytest.raises(ValueError, match="smooth"):
        emu_engine.mesh(np.ones((2, 2, 2), np.uint8), smooth=-1)
    with pytest.raises(ValueError, match="1..255"):
        emu_engine.mesh(np.ones((2, 2, 2), np.uint8), keep=[0])


def test_a_plan_is_used_once_and_only_for_its_labels(emu_engine):
    """lm_mesh_dev right after lm_mesh_plan_dev reuses the plan; with other labels, or a second time, it plans itself."""
    a, b = blobs((9, 30, 33), 4), blobs((9, 30, 33), 5)
    ad, bd = emu_engine.to_device(a), emu_engine.to_device(b)
    emu_engine.mesh_plan_dev(ad)
    vb, qb, _ = emu_engine.mesh_dev(bd)
    va, qa, _ = emu_engine.mesh_dev(ad, keep=[1])
    emu_engine.sync()
    assert same_mesh((vb.download(), qb.download()), oracle_mesh(b))
    assert same_mesh((va.download(), qa.download()), oracle_mesh(a, keep=[1]))
    for d in (ad, bd, vb, qb, va, qa):
        d.free()
