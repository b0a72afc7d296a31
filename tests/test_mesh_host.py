"""Host side of the surface meshes (lungmask_amd/mesh.py): coordinates and winding, area and volume, the STL / PLY / OBJ writers
re-read by a few lines of parser, save_all, meta(), and the command line's --mesh on the emulated engine."""
import json
import struct

import numpy as np
import pytest

from lungmask_amd import mesh as lmmesh
from lungmask_amd import volume_io
from tests.cli_fake import FakeInferer

# a unit cube [0, 1]^3 with outward quads (right-hand rule in the order the coordinates are listed)
CUBE_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
CUBE_Q = np.array([[0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [2, 3, 7, 6], [1, 2, 6, 5], [0, 4, 7, 3]], np.int32)


def cube(scale=(1.0, 1.0, 1.0)):
    return lmmesh.Mesh(CUBE_V * np.asarray(scale), CUBE_Q, "mm", [0, 1, 0, 1, 0, 1], [1], 0)


def test_area_and_volume_of_a_hand_made_cube():
    m = cube()
    assert m.surface_area == pytest.approx(6.0, abs=1e-12) and m.volume == pytest.approx(1.0, abs=1e-12)
    assert m.triangles.shape == (12, 3) and m.triangles.dtype == np.int32 and m.vertices.dtype == np.float64
    assert np.array_equal(m.triangles[0], [0, 3, 2]) and np.array_equal(m.triangles[1], [0, 2, 1])
    m = cube((2.0, 3.0, 0.5))
    assert m.surface_area == pytest.approx(2 * (6 + 1 + 1.5), abs=1e-12) and m.volume == pytest.approx(3.0, abs=1e-12)
    centre = m.vertices.mean(axis=0)
    mid = m.vertices[m.triangles].mean(axis=1)
    assert (np.einsum("ij,ij->i", m.triangle_normals(), mid - centre) > 0).all()  # outward


def test_winding_reversed_for_a_mirroring_geometry():
    ident = (np.eye(3), np.zeros(3), "voxel")
    m = lmmesh.to_mesh(CUBE_V.astype(np.float32), CUBE_Q, ident)
    assert np.array_equal(m.quads, CUBE_Q) and m.volume == pytest.approx(1.0)
    # array (z, y, x) -> LPS (x, y, z) with the identity direction: a reversal of the axes, determinant -1
    vol = volume_io.Volume(np.zeros((2, 2, 2), np.uint8), (0.5, 2.0, 3.0), (10.0, -20.0, 30.0))
    a, t, unit = lmmesh.index_affine(vol)
    assert unit == "mm" and np.linalg.det(a) < 0
    m = lmmesh.to_mesh(CUBE_V.astype(np.float32), CUBE_Q, (a, t, unit))
    assert np.array_equal(m.quads, CUBE_Q[:, [0, 3, 2, 1]])  # the first corner stays
    assert m.volume == pytest.approx(0.5 * 2.0 * 3.0) and m.surface_area == pytest.approx(2 * (1.0 + 6.0 + 1.5))
    for v_in, v_out in zip(CUBE_V, m.vertices):
        np.testing.assert_allclose(v_out, vol.index_to_physical(v_in[::-1]), atol=1e-12)
    # a flipped and permuted direction with determinant +1 after the axis reversal keeps the winding
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)
    vol2 = volume_io.Volume(np.zeros((2, 2, 2), np.uint8), (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), direction)
    a2, t2, _ = lmmesh.index_affine(vol2)
    m2 = lmmesh.to_mesh(CUBE_V.astype(np.float32), CUBE_Q, (a2, t2, "mm"))
    assert np.array_equal(m2.quads, CUBE_Q if np.linalg.det(a2) > 0 else CUBE_Q[:, [0, 3, 2, 1]])
    assert m2.volume == pytest.approx(0.7 * 0.8 * 2.5)
    for v_in, v_out in zip(CUBE_V, m2.vertices):
        np.testing.assert_allclose(v_out, vol2.index_to_physical(v_in[::-1]), atol=1e-12)
    # numpy input: index times spacing in array axis order; without a spacing, indices
    a3, t3, unit3 = lmmesh.index_affine(np.zeros((2, 2, 2), np.uint8), (2.5, 0.7, 0.8))
    assert unit3 == "mm" and np.array_equal(a3, np.diag([2.5, 0.7, 0.8])) and not t3.any()
    assert lmmesh.index_affine(np.zeros((2, 2, 2), np.uint8))[2] == "voxel"
    with pytest.raises(ValueError, match="spacing"):
        lmmesh.index_affine(vol, (1, 1, 1))


def read_stl(path):
    raw = open(path, "rb").read()
    (n,) = struct.unpack_from("<I", raw, 80)
    assert len(raw) == 84 + 50 * n
    rec = np.frombuffer(raw, dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")], offset=84)
    return rec["n"], rec["v"], rec["attr"]


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    nf = int(next(ln for ln in head if ln.startswith("element face")).split()[-1])
    has_label = "property uchar label" in head
    fdt = [("k", "u1"), ("i", "<i4", 4)] + ([("label", "u1")] if has_label else [])
    assert len(raw) == end + 24 * nv + np.dtype(fdt).itemsize * nf
    v = np.frombuffer(raw, "<f8", 3 * nv, end).reshape(nv, 3)
    f = np.frombuffer(raw, fdt, nf, end + 24 * nv)
    assert (f["k"] == 4).all()
    return v, f["i"], (f["label"] if has_label else None)


def read_obj(path):
    groups, v, cur = {}, [], None
    for ln in open(path):
        t = ln.split()
        if not t or t[0] == "#":
            continue
        if t[0] == "g":
            cur = t[1]
        elif t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t[0] == "f":
            groups.setdefault(cur, []).append([int(x) - 1 for x in t[1:]])
    return np.array(v, np.float64), {k: np.array(f, np.int32) for k, f in groups.items()}


def test_stl_ply_obj_round_trips(tmp_path):
    m = cube((2.0, 3.0, 0.5))
    m.save(str(tmp_path / "c.stl"))
    n, v, attr = read_stl(tmp_path / "c.stl")
    assert len(v) == 12 and not attr.any()
    assert np.array_equal(v, m.vertices[m.triangles].astype(np.float32))
    assert np.array_equal(n, m.triangle_normals().astype(np.float32))
    m.save(str(tmp_path / "c.ply"))
    pv, pf, pl = read_ply(tmp_path / "c.ply")
    assert np.array_equal(pv, m.vertices) and np.array_equal(pf, m.quads) and pl is None
    m.save(str(tmp_path / "c.obj"))
    ov, og = read_obj(tmp_path / "c.obj")
    assert np.array_equal(ov, m.vertices) and list(og) == [None] and np.array_equal(og[None], m.quads)  # repr() round-trips a float64
    with pytest.raises(ValueError, match="unsupported"):
        m.save(str(tmp_path / "c.vtk"))


def test_save_all_groups(tmp_path):
    meshes = {1: cube(), 4: cube((2.0, 2.0, 2.0)), "lung": cube((3.0, 1.0, 1.0))}
    lmmesh.save_all(meshes, str(tmp_path / "all.obj"))
    ov, og = read_obj(tmp_path / "all.obj")
    assert list(og) == ["1", "4", "lung"] and len(ov) == 24
    for k, (name, m) in enumerate(meshes.items()):
        assert np.array_equal(og[str(name)], m.quads + 8 * k) and np.array_equal(ov[8 * k:8 * k + 8], m.vertices)
    lmmesh.save_all(meshes, str(tmp_path / "all.ply"))
    pv, pf, pl = read_ply(tmp_path / "all.ply")
    assert len(pv) == 24 and len(pf) == 18 and pl.tolist() == [1] * 6 + [4] * 6 + [0] * 6
    assert np.array_equal(pf[6:12], CUBE_Q + 8) and np.array_equal(pv[8:16], CUBE_V * 2.0)
    with pytest.raises(ValueError, match="save_all"):
        lmmesh.save_all(meshes, str(tmp_path / "all.stl"))


def test_meta_is_json_serialisable():
    d = json.loads(json.dumps(cube().meta()))
    assert d["n_vertices"] == 8 and d["n_quads"] == 6 and d["n_triangles"] == 12 and d["unit"] == "mm" and d["labels"] == [1]
    assert d["surface_area"] == pytest.approx(6.0) and d["volume"] == pytest.approx(1.0) and d["bbox"] == [0, 1, 0, 1, 0, 1]


def test_extract_surface_on_the_emulated_engine(emu_engine):
    from tests.test_mesh_emu import ball, oracle_mesh

    lab = ball(11, 4.2) * 3
    lab[0, 0, 0] = 7
    sp = (2.0, 0.5, 0.75)
    vol = volume_io.Volume(lab, sp[::-1], (5.0, 6.0, 7.0))
    want_v, want_q = oracle_mesh(lab, keep=[3])
    m = lmmesh.extract_surface(vol, label=3, engine=emu_engine)
    assert np.array_equal(m.quads, want_q[:, [0, 3, 2, 1]]) and m.unit == "mm" and m.labels == [3]
    np.testing.assert_allclose(m.vertices, want_v.astype(np.float64)[:, ::-1] * np.asarray(sp[::-1]) + [5.0, 6.0, 7.0], atol=1e-12)
    n_vox = int((lab == 3).sum())
    assert m.volume > 0 and abs(m.volume - n_vox * np.prod(sp)) < 0.35 * n_vox * np.prod(sp)  # (surface nets shrink a small ball)
    a = lmmesh.extract_surface(lab, spacing=sp, label=[3], engine=emu_engine)
    assert np.array_equal(a.quads, want_q) and a.volume == pytest.approx(m.volume) and a.surface_area == pytest.approx(m.surface_area)
    np.testing.assert_allclose(a.vertices, want_v.astype(np.float64) * np.asarray(sp), atol=1e-12)
    idx = lmmesh.extract_surface(lab, engine=emu_engine)  # every label >= 1: the ball and the stray voxel
    assert idx.unit == "voxel" and len(idx.vertices) == len(want_v) + 8 and idx.labels is None
    both = lmmesh.extract_surfaces(lab, engine=emu_engine)
    assert sorted(both) == [3, 7] and np.array_equal(both[3].quads, want_q) and len(both[7].quads) == 6
    assert list(lmmesh.extract_surfaces(lab, per_label=False, engine=emu_engine)) == ["lung"]
    with pytest.raises(ValueError, match="no voxel"):
        lmmesh.extract_surface(lab, label=5, engine=emu_engine)
    with pytest.raises(ValueError, match="1..255"):
        lmmesh.extract_surface(lab, label=0, engine=emu_engine)


def test_cli_mesh(emu_engine, tmp_path, monkeypatch):
    import lungmask_amd.__main__ as cli
    from tests.test_mesh_emu import ball

    lab = np.zeros((12, 14, 16), np.uint8)
    lab[1:10, 1:10, 1:10] = ball(9, 3.6)
    lab[2:11, 4:13, 6:15][ball(9, 2.9) > 0] = 2
    img = volume_io.Volume(np.zeros(lab.shape, np.int16), (0.7, 0.8, 2.5), (1.0, 2.0, 3.0))
    ip = tmp_path / "in.nii.gz"
    volume_io.write_nifti(str(ip), img)
    FakeInferer.engine, FakeInferer.labels = emu_engine, lab
    monkeypatch.setattr(cli, "LMInferer", FakeInferer)
    loaded = volume_io.load_input_image(str(ip))
    assert cli.main([str(ip), str(tmp_path / "o.npy"), "--noprogress", "--mesh", str(tmp_path / "lobe_{label}.ply"), "--mesh-smooth", "2"]) == 0
    for k in (1, 2):
        want = lmmesh.extract_surface(loaded.like(lab), label=k, smooth=2, engine=emu_engine)
        pv, pf, _ = read_ply(tmp_path / f"lobe_{k}.ply")
        assert np.array_equal(pv, want.vertices) and np.array_equal(pf, want.quads) and want.volume > 0
    assert cli.main([str(ip), str(tmp_path / "o2.npy"), "--noprogress", "--mesh", str(tmp_path / "lung.stl")]) == 0
    whole = lmmesh.extract_surface(loaded.like(lab), engine=emu_engine)
    _, sv, _ = read_stl(tmp_path / "lung.stl")
    assert np.array_equal(sv, whole.vertices[whole.triangles].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "o2.npy"), lab)
    out = str(tmp_path / "o3.npy")
    with pytest.raises(SystemExit, match="--mesh"):  # refused before anything is loaded
        cli.main([str(ip), out, "--mesh", str(tmp_path / "m.vtk")])
    with pytest.raises(SystemExit, match="--mesh-smooth"):
        cli.main([str(ip), out, "--mesh-smooth", "3"])
    with pytest.raises(SystemExit, match="--mesh-smooth"):
        cli.main([str(ip), out, "--mesh", str(tmp_path / "m.obj"), "--mesh-smooth", "-1"])
    a = cli.build_parser().parse_args([str(ip), out, "--mesh", "m.obj", "--stats", "s.json", "--roi", "r.mha", "--probabilities", "p.npy"])
    assert a.mesh == "m.obj" and a.mesh_smooth is None
