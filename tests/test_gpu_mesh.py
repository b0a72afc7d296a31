"""The surface meshes on the MI355X: lm_mesh_dev bit for bit and in order against the numpy oracle of tests/test_mesh_emu.py (the
same shapes), LMInferer.apply_mesh (R231, LTRCLobes, a non-LPS Volume) against extract_surface, and determinism over two calls."""
import numpy as np
import pytest

from lungmask_amd import mesh as lmmesh
from lungmask_amd import synthetic as syn
from lungmask_amd import volume_io
from tests.test_mesh_emu import ball, blobs, cell_counts, check, is_closed, noise, oracle_mesh, same_mesh, signed_volume

pytestmark = pytest.mark.gpu


def test_mesh_small_shapes(gpu_engine):
    one = np.zeros((3, 3, 3), np.uint8)
    one[1, 1, 1] = 1
    check(gpu_engine, one, "single voxel")
    check(gpu_engine, np.ones((1, 1, 1), np.uint8), "(1, 1, 1)")
    check(gpu_engine, np.ones((7, 9, 11), np.uint8), "full")
    lab = blobs((11, 37, 45), 2)
    for keep in ([1], [2], None):
        check(gpu_engine, lab, keep, keep=keep)
    six = blobs((9, 33, 40), 13, n_labels=6)
    for keep in ([2], [5], [2, 5]):
        check(gpu_engine, six, keep, keep=keep)
    for lab in (ball(15, 6.2), ball(17, 7.3, cavity=3.1)):
        verts, quads, _ = check(gpu_engine, lab, "ball")
        assert is_closed(quads) and signed_volume(verts, quads) > 0


@pytest.mark.parametrize("shape", [(6, 7, 8), (3, 70, 130), (24, 96, 128)])
def test_mesh_noise(gpu_engine, shape):
    lab = noise(shape, 0 if shape == (6, 7, 8) else 1)
    verts, quads, _ = check(gpu_engine, lab, shape)
    full, act = cell_counts(lab)
    assert is_closed(quads) and full <= signed_volume(verts, quads) <= full + act


@pytest.mark.parametrize("smooth", [1, 3])
@pytest.mark.parametrize("factors", [None, (0.33, -0.34)])
def test_mesh_smoothing(gpu_engine, smooth, factors):
    kw = {} if factors is None else {"lam": factors[0], "mu": factors[1]}
    for lab in (blobs((11, 37, 45), 2), noise((6, 7, 8)), noise((3, 70, 130), 1)):
        check(gpu_engine, lab, (smooth, factors), smooth=smooth, **kw)


def test_mesh_dev_resident_and_deterministic(gpu_engine):
    lab = noise((24, 96, 128), 1)
    want = oracle_mesh(lab, smooth=2)
    ld = gpu_engine.to_device(lab)
    runs = []
    for _ in range(2):
        verts, quads, info = gpu_engine.mesh_dev(ld, smooth=2)
        gpu_engine.sync()
        runs.append((verts.download(), quads.download()))
        assert info["n_vertices"] == len(want[0]) and info["n_quads"] == len(want[1])
        verts.free()
        quads.free()
    ld.free()
    assert same_mesh(runs[0], want) and same_mesh(runs[1], want)


def _same(a, b):
    return (np.array_equal(a.vertices, b.vertices) and np.array_equal(a.quads, b.quads) and np.array_equal(a.triangles, b.triangles) and
            a.meta() == b.meta())


@pytest.mark.parametrize("model", ["R231", "LTRCLobes"])
def test_apply_mesh_models(gpu_engine, model):
    from lungmask_amd.mask import LMInferer

    c = 3 if model == "R231" else 6
    inf = LMInferer(modelname=model, state_dict=syn.synthetic_state_dict(c, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(12, 512, 512)
    expect = inf.apply(vol).copy()
    present = [int(v) for v in np.unique(expect) if v > 0]
    assert len(present) >= 2
    labels, meshes = inf.apply_mesh(vol, spacing=(2.0, 0.75, 0.75), smooth=1)
    assert np.array_equal(labels, expect) and sorted(meshes) == present
    for k in present:
        want = lmmesh.extract_surface(expect, spacing=(2.0, 0.75, 0.75), label=k, smooth=1, engine=gpu_engine)
        assert _same(meshes[k], want) and want.volume > 0 and want.unit == "mm"
    labels2, meshes2 = inf.apply_mesh(vol, spacing=(2.0, 0.75, 0.75), smooth=1)  # two identical calls, identical results
    assert np.array_equal(labels2, labels) and all(_same(meshes2[k], meshes[k]) for k in present)
    labels3, whole = inf.apply_mesh(vol, per_label=False)
    assert np.array_equal(labels3, expect) and list(whole) == ["lung"]
    assert _same(whole["lung"], lmmesh.extract_surface(expect, engine=gpu_engine)) and whole["lung"].unit == "voxel"
    assert inf.apply_mesh(vol, labels=[200])[1] == {}
    with pytest.raises(ValueError, match="no voxel"):
        inf.apply_mesh(vol, labels=[200], per_label=False)


def test_apply_mesh_non_lps_volume(gpu_engine):
    """Vertices are LPS millimetres: each lies within one source voxel diagonal of a selected voxel's physical position."""
    from scipy.spatial import cKDTree

    from lungmask_amd.mask import LMInferer

    inf = LMInferer(state_dict=syn.synthetic_state_dict(3, head="lunglike"), engine=gpu_engine)
    vol = syn.phantom(12, 512, 512)
    direction = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0)  # permuted and flipped
    axes, flips = volume_io.lps_transform(direction)
    arr = np.ascontiguousarray(volume_io.apply_transform(vol, *volume_io.inverse_transform(axes, flips)))
    img = volume_io.Volume(arr, (0.7, 0.8, 2.5), (-12.0, 30.0, 4.5), direction)
    expect = inf.apply(img).copy()
    labels, meshes = inf.apply_mesh(img)
    assert np.array_equal(labels, expect) and len(meshes) >= 1
    diagonal = float(np.linalg.norm(img.spacing))
    for k, m in meshes.items():
        assert _same(m, lmmesh.extract_surface(img.like(expect), label=k, engine=gpu_engine))
        assert m.volume > 0 and m.unit == "mm"
        idx = np.argwhere(expect == k).astype(np.float64)  # (z, y, x)
        phys = np.asarray(img.origin) + (idx[:, ::-1] * np.asarray(img.spacing)) @ np.asarray(img.direction, np.float64).reshape(3, 3).T
        dist, _ = cKDTree(phys).query(m.vertices)
        assert dist.max() <= diagonal
