"""Lung and lobe surface meshes extracted on the GPU from a label mask (not in the reference: what callers run
`skimage.measure.marching_cubes` on the finished mask for), with STL / PLY / OBJ writers that need no other package.

The device passes (`lm_mesh_plan_dev`, `lm_mesh_dev`; lungmask_amd/csrc/mesh_kernels.hip) follow the definition in
include/lungmask_hip.h -- SURFACE NETS of the binary selection "the voxel's label is one of `label`":

- Voxel centres sit at the integer indices; voxels outside the volume are unselected, so the surface closes at the border.
- One vertex per 2 x 2 x 2 cell of voxels that are not all equal: the mean of the midpoints of the cell's edges whose ends differ.
- One quad per pair of axis neighbours whose selection differs, joining the four cells round that grid edge, wound so that the
  normal points out of the selection.  Triangles are corners (0, 1, 2) and (0, 2, 3) of each quad.
- `smooth` Taubin iterations (factor `lam`, then `mu`) over the vertices joined across a cell face the surface passes through;
  uniform weights in index space, which commute with the affine map to millimetres.

The mesh is closed.  It can be non-manifold where two selected voxels meet only across an edge or a corner, and unsmoothed surface
nets shrink features one voxel wide (a single voxel becomes a cube of side 1/3).

The host maps the vertices to the caller's coordinates (`Mesh.vertices`), reverses the winding when that map mirrors (array (z, y, x)
to LPS (x, y, z) does), and derives the triangles, the surface area and the enclosed volume in float64.
"""
from __future__ import annotations

import struct
from typing import Dict, Optional

import numpy as np

from . import _native

MESH_EXTENSIONS = (".stl", ".ply", ".obj")


class Mesh:
    """What `extract_surface` / `LMInferer.apply_mesh` return.  `vertices` float64 [V][3]: LPS millimetres (x, y, z) for a Volume or
    a SimpleITK image; index times spacing in array axis order for a numpy array with a spacing; array indices (z, y, x) without one
    (`unit`: "mm" or "voxel").  `quads` int32 [Q][4] and `triangles` int32 [2 Q][3] index them, normals pointing out of the
    selection.  `bbox`: zmin, zmax, ymin, ymax, xmin, xmax of the selected voxels in array indices, exclusive maxima.
    `surface_area` (unit^2) and `volume` (unit^3, the signed volume the triangles enclose), float64 on the host."""

    def __init__(self, vertices, quads, unit="voxel", bbox=None, labels=None, smooth=0):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.quads = np.ascontiguousarray(quads, dtype=np.int32).reshape(-1, 4)
        self.triangles = np.ascontiguousarray(np.concatenate([self.quads[:, [0, 1, 2]], self.quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3))
        self.unit = unit
        self.bbox = None if bbox is None else [int(v) for v in bbox]
        self.labels = None if labels is None else [int(v) for v in labels]
        self.smooth = int(smooth)
        p = self.vertices[self.triangles]
        cross = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        self.surface_area = float(0.5 * np.linalg.norm(cross, axis=1).sum())
        self.volume = float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)

    def triangle_normals(self) -> np.ndarray:
        """Unit normals float64 [T][3] (zero for a degenerate triangle)."""
        p = self.vertices[self.triangles]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        return np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)

    def meta(self) -> dict:
        """The non-array fields, JSON-serialisable."""
        return {"n_vertices": int(len(self.vertices)), "n_quads": int(len(self.quads)), "n_triangles": int(len(self.triangles)),
                "unit": self.unit, "bbox": None if self.bbox is None else list(self.bbox),
                "labels": None if self.labels is None else list(self.labels), "smooth": self.smooth,
                "surface_area": self.surface_area, "volume": self.volume}

    def save(self, path: str) -> None:
        """Binary .stl (triangles), binary little-endian .ply (quads) or .obj (quads), by the file name."""
        low = str(path).lower()
        if low.endswith(".stl"):
            _write_stl(path, self)
        elif low.endswith(".ply"):
            _write_ply(path, [self], None)
        elif low.endswith(".obj"):
            _write_obj(path, {None: self})
        else:
            raise ValueError(f"unsupported mesh file type {path!r} (use .stl, .ply or .obj)")


def _write_stl(path, mesh: Mesh) -> None:
    tri = mesh.vertices[mesh.triangles].astype("<f4")
    rec = np.zeros(len(tri), dtype=[("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")])
    rec["n"] = mesh.triangle_normals().astype("<f4")
    rec["v"] = tri
    with open(path, "wb") as f:
        f.write(b"lungmask_amd surface mesh".ljust(80, b" "))
        f.write(struct.pack("<I", len(tri)))
        f.write(rec.tobytes())


def _write_ply(path, meshes, face_labels) -> None:
    nv, nf = sum(len(m.vertices) for m in meshes), sum(len(m.quads) for m in meshes)
    header = ["ply", "format binary_little_endian 1.0", "comment lungmask_amd surface mesh", f"element vertex {nv}",
              "property double x", "property double y", "property double z", f"element face {nf}",
              "property list uchar int vertex_indices"]
    dt = [("k", "u1"), ("i", "<i4", 4)]
    if face_labels is not None:
        header.append("property uchar label")
        dt.append(("label", "u1"))
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        for m in meshes:
            f.write(m.vertices.astype("<f8").tobytes())
        base = 0
        for k, m in enumerate(meshes):
            rec = np.zeros(len(m.quads), dtype=dt)
            rec["k"] = 4
            rec["i"] = m.quads + base
            if face_labels is not None:
                rec["label"] = face_labels[k]
            f.write(rec.tobytes())
            base += len(m.vertices)


def _write_obj(path, groups) -> None:
    with open(path, "w") as f:
        f.write("# lungmask_amd surface mesh\n")
        base = 1
        for name, m in groups.items():
            if name is not None:
                f.write(f"g {name}\n")
            for v in m.vertices:
                f.write("v %s %s %s\n" % (repr(float(v[0])), repr(float(v[1])), repr(float(v[2]))))
            for q in m.quads + base:
                f.write("f %d %d %d %d\n" % (q[0], q[1], q[2], q[3]))
            base += len(m.vertices)


def save_all(meshes: Dict[object, Mesh], path: str) -> None:
    """Several meshes in one file: .obj with one group (`g name`) per mesh, or .ply with a `label` face property (uchar: the mesh's
    name when it is a label value 0..255, else 0)."""
    low = str(path).lower()
    if low.endswith(".obj"):
        _write_obj(path, {str(k): m for k, m in meshes.items()})
    elif low.endswith(".ply"):
        labels = [int(k) if isinstance(k, (int, np.integer)) and 0 <= int(k) <= 255 else 0 for k in meshes]
        _write_ply(path, list(meshes.values()), labels)
    else:
        raise ValueError(f"save_all: one .obj or .ply file, got {path!r}")


def index_affine(image, spacing=None):
    """(A [3][3], t [3], unit) with output coordinate = A @ (z, y, x) + t: LPS millimetres (x, y, z) for a Volume / SimpleITK image
    (`Volume.index_to_physical`), index times spacing for a numpy array with a spacing, the identity without one."""
    from . import stats as st
    from . import volume_io

    if isinstance(image, np.ndarray):
        _, sp, _ = st.geometry(image, spacing)
        if sp is None:
            return np.eye(3), np.zeros(3), "voxel"
        if not all(v > 0 and np.isfinite(v) for v in sp):
            raise ValueError(f"spacing needs three positive values in the array's axis order, got {spacing!r}")
        return np.diag(np.asarray(sp, np.float64)), np.zeros(3), "mm"
    if spacing is not None:
        raise ValueError("spacing is taken from the image (Volume / SimpleITK image): do not pass it as well")
    if isinstance(image, volume_io.Volume):
        sp_xyz, origin, direction = image.spacing, image.origin, image.direction
    else:
        sp_xyz, origin, direction = image.GetSpacing(), image.GetOrigin(), image.GetDirection()
    d = np.asarray(direction, np.float64).reshape(3, 3)
    a = (d * np.asarray(sp_xyz, np.float64)[None, :])[:, ::-1]  # physical = origin + D @ (index_xyz * spacing), index_xyz = (z, y, x)[::-1]
    return a, np.asarray(origin, np.float64), "mm"


def to_mesh(verts_zyx: np.ndarray, quads: np.ndarray, affine, bbox=None, labels=None, smooth=0) -> Mesh:
    """The host `Mesh` of lm_mesh_dev's arrays: vertices through the affine map, the winding reversed when that map mirrors."""
    a, t, unit = affine
    v = verts_zyx.astype(np.float64) @ np.asarray(a, np.float64).T + np.asarray(t, np.float64)
    q = np.asarray(quads, np.int32)
    if np.linalg.det(np.asarray(a, np.float64)) < 0:
        q = q[:, [0, 3, 2, 1]]
    return Mesh(v, q, unit, bbox, labels, smooth)


def label_list(label):
    """None (every label >= 1), one value or a sequence -> the keep list of the engine (None or a sorted list)."""
    if label is None:
        return None
    vals = [label] if np.ndim(label) == 0 else list(label)
    if not vals:
        raise ValueError("label: at least one label value")
    _native.Engine._keep_table(vals)  # (1..255, integers)
    return sorted(set(int(v) for v in vals))


def from_device(verts, quads, info, affine, labels=None, smooth=0) -> Mesh:
    """The host `Mesh` of mesh_dev's device arrays (downloaded and freed here)."""
    try:
        verts.eng.sync()
        return to_mesh(verts.download(), quads.download(), affine, info["bbox"], labels, smooth)
    finally:
        verts.free()
        quads.free()


def _labels_u8(labels) -> np.ndarray:
    from . import stats as st

    lab = np.ascontiguousarray(st._label_array(labels))
    if lab.ndim != 3:
        raise ValueError(f"labels must be a 3-D volume, got shape {lab.shape}")
    if lab.dtype != np.uint8:
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("labels must lie in 0..255")
        lab = lab.astype(np.uint8)
    return lab


def extract_surface(labels, spacing=None, label=None, smooth=0, lam=0.5, mu=-0.53, engine=None) -> Mesh:
    """The surface of the voxels of `labels` (numpy [n, h, w], a `volume_io.Volume` or a SimpleITK image; u8-valued: a mask from
    `apply`, from the reference or edited by hand) whose value is `label`: None = every label >= 1 together, one value, or a
    sequence of values meshed together.  Computed on the GPU -> `Mesh`.  No such voxel: ValueError.

    `spacing`: numpy input only, in the array's axis order.  `smooth`: Taubin iterations with the factors `lam` and `mu`.
    `engine`: a _native.Engine (default: a new one on device 0)."""
    affine = index_affine(labels, spacing)
    lab = _labels_u8(labels)
    keep = label_list(label)
    with _native.engine_scope(engine) as eng:
        verts, quads, info = eng.mesh(lab, keep=keep, smooth=smooth, lam=lam, mu=mu)
    return to_mesh(verts, quads, affine, info["bbox"], keep, smooth)


def surfaces_dev(eng, lab_dev, affine, labels=None, per_label=True, smooth=0, lam=0.5, mu=-0.53, all_labels=None) -> Dict[object, Mesh]:
    """The meshes of device-resident labels, one device call per mesh: per_label -> {label value: Mesh} for each of `labels`
    (None: `all_labels`) that has a voxel; otherwise {"lung": Mesh} of `labels` together (None: every label >= 1)."""
    out: Dict[object, Mesh] = {}
    if not per_label:
        keep = label_list(labels)
        out["lung"] = from_device(*eng.mesh_dev(lab_dev, keep=keep, smooth=smooth, lam=lam, mu=mu), affine, keep, smooth)
        return out
    wanted = label_list(labels) if labels is not None else sorted(int(v) for v in (all_labels or []))
    for k in wanted:
        try:
            res = eng.mesh_dev(lab_dev, keep=[k], smooth=smooth, lam=lam, mu=mu)
        except ValueError:
            continue  # the label has no voxel in this volume
        out[int(k)] = from_device(*res, affine, [k], smooth)
    return out


def extract_surfaces(labels, spacing=None, label_values=None, per_label=True, smooth=0, lam=0.5, mu=-0.53, engine=None) -> Dict[object, Mesh]:
    """`surfaces_dev` for host labels (uploaded once): per_label with label_values None meshes every label value present."""
    affine = index_affine(labels, spacing)
    lab = _labels_u8(labels)
    present: Optional[list] = None
    if per_label and label_values is None:
        present = [int(v) for v in np.unique(lab) if v > 0]
    with _native.engine_scope(engine) as eng, eng.scope() as dev:
        return surfaces_dev(eng, dev.upload(lab), affine, label_values, per_label, smooth, lam, mu, all_labels=present)
