"""`python -m lungmask_amd INPUT OUTPUT [...]` -- the reference's command line (lungmask/__main__.py:20-144)
on the MI355X engine.  Same flags; thin by design (all I/O, off the hot path):

* `.npy` / `.npz`, NIfTI-1 (`.nii`, `.nii.gz`), MetaImage (`.mha`, `.mhd`) and uncompressed DICOM (files and series
  folders) are read and written by `volume_io.py` without any imaging dependency -- DICOM output as one multi-frame file
  with the carried-over study / patient tags of __main__.py:125-141 (`--removemetadata` drops them);
* every other format (NRRD, compressed DICOM, ...) goes through SimpleITK like the reference (imported lazily; this image
  does not ship it);
* `--cpu` is an error by default (there is no CPU path in this engine); with LUNGMASK_AMD_ALLOW_CPU_FLAG=1 it is accepted, warned about, and the work runs on the MI355X.
"""
import argparse
import functools
import json
import os
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import airways as lmairways
from . import components as lmcomp
from . import deformable as lmdef
from . import filters as lmfilters
from . import mesh as lmmesh
from . import metrics as lmmetrics
from . import morphology as lmmorph
from . import pairs as lmpairs
from . import registration as lmreg
from . import resample as lmresample
from . import roi as lmroi
from . import skeleton as lmskeleton
from . import stats as lmstats
from . import texture as lmtexture
from . import vessels as lmvessels
from . import volume_io
from .logger import logger
from .mask import LMInferer

VERSION = "0.2.20+mi355x"

# utils.py:17-30
DICOM_METADATA_TO_KEEP = ("0008|0020", "0008|0030", "0008|0050", "0008|0090", "0008|1030", "0010|0010", "0010|0020",
                          "0010|0030", "0010|0040", "0018|5100", "0020|000d", "0020|0010")


def path(string):  # __main__.py:13-17
    if os.path.exists(string):
        return string
    sys.exit(f"File not found: {string}")


def build_parser():
    p = argparse.ArgumentParser(prog="lungmask_amd", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("input", metavar="input", type=path, help="Path to the input image, can be a folder for dicoms")
    p.add_argument("output", metavar="output", type=str, help="Filepath for output lungmask")
    p.add_argument("--modelname", help="spcifies the trained model, Default: R231", type=str,
                   choices=["R231", "LTRCLobes", "LTRCLobes_R231", "R231CovidWeb"], default="R231")
    p.add_argument("--modelpath", help="spcifies the path to the trained model", default=None)
    p.add_argument("--cpu", help="Force using the CPU (not available in this engine: an error unless LUNGMASK_AMD_ALLOW_CPU_FLAG=1, then ignored with a warning)", action="store_true")
    p.add_argument("--nopostprocess", help="Deactivates postprocessing (removal of unconnected components and hole filling)", action="store_true")
    p.add_argument("--batchsize", type=int, help="Number of slices processed simultaneously.", default=20)
    p.add_argument("--noprogress", action="store_true", help="If set, no tqdm progress bar will be shown")
    p.add_argument("--version", help="Shows the current version of lungmask", action="version", version=VERSION)
    p.add_argument("--removemetadata", action="store_true", help="Do not keep study/patient related metadata of the input, if any.")
    p.add_argument("--probabilities", metavar="PATH", default=None,
                   help="Also write the per-class probability maps at the input's geometry (not in the reference): .npy = float32 "
                        "[C][n][h][w], .nii / .nii.gz = 4-D float32 NIfTI with the class as the 4th axis. One forward pass gives both.")
    p.add_argument("--stats", metavar="PATH.json", default=None,
                   help="Also write per-label volume (mL) and density statistics (mean / std HU, percentiles, share below -950 HU, "
                        "centroid, box) of the saved labels as JSON (not in the reference). Computed on the GPU.")
    p.add_argument("--texture", metavar="PATH.json", default=None,
                   help="Also write per-label GLCM and GLRLM texture features (IBSI definitions, 13 directions averaged) of the saved "
                        "labels as JSON (not in the reference). The matrices are computed on the GPU.")
    p.add_argument("--texture-bin-width", metavar="HU", type=int, default=None,
                   help="Width in HU of the grey-level bins of --texture (default 25).")
    p.add_argument("--texture-range", metavar=("LO", "HI"), type=int, nargs=2, default=None,
                   help="HU range of --texture: voxels outside LO..HI are excluded (default -1000 199). At most 64 bins.")
    p.add_argument("--compare-to", metavar="MASK", default=None,
                   help="A label volume of the input's shape (e.g. a ground truth) to compare the result with; needs --metrics.")
    p.add_argument("--metrics", metavar="PATH.json", default=None,
                   help="Write Dice, Jaccard, Hausdorff and surface distances (mm) per label between the result (a) and the "
                        "--compare-to mask (b) as JSON (not in the reference). Computed on the GPU.")
    p.add_argument("--roi", metavar="PATH", default=None,
                   help="Also write the lung ROI (not in the reference): the input cropped to the box of the labels plus 5 mm, "
                        "blanked to -1024 outside them, float32. .nii / .nii.gz / .mha / .mhd carry the ROI's geometry, .npy the array. "
                        "Computed on the GPU.")
    p.add_argument("--roi-spacing", metavar="MM", type=float, default=None,
                   help="Isotropic spacing (mm) the --roi volume is resampled to (default: the source spacing, a pure crop).")
    p.add_argument("--mesh", metavar="PATH", default=None,
                   help="Also write the surface of the result as a mesh (not in the reference): .stl, .ply or .obj, vertices in LPS "
                        "millimetres. PATH is the whole lung; with {label} in it, one file per label value. Extracted on the GPU.")
    p.add_argument("--mesh-smooth", metavar="N", type=int, default=None,
                   help="Taubin smoothing iterations of the --mesh surface (default 0: the unsmoothed surface).")
    p.add_argument("--closed", metavar="PATH", default=None,
                   help="Also write the morphologically closed mask (not in the reference): the labels closed as a whole by a ball of "
                        "--close-mm, each new voxel with the label of the nearest lung or lobe, so that juxta-pleural nodules and "
                        "consolidations cut out of the mask come back. Same file formats as the mask, which is unchanged. "
                        "Computed on the GPU.")
    p.add_argument("--close-mm", metavar="MM", type=float, default=None,
                   help="Radius in mm of the ball of --closed (default 10).")
    p.add_argument("--clusters", metavar="PATH.json", default=None,
                   help="Also write the cluster analysis of the saved labels as JSON (not in the reference): per label and for the whole "
                        "lung the connected clusters of voxels below --cluster-threshold, their number, sizes, size histogram and the "
                        "cumulative cluster-size exponent D. Computed on the GPU.")
    p.add_argument("--cluster-threshold", metavar="HU", type=int, default=None,
                   help="Voxels with HU below this value form the clusters of --clusters (default -950).")
    p.add_argument("--cluster-connectivity", type=int, choices=[6, 26], default=None,
                   help="Connectivity of the clusters of --clusters (default 6).")
    p.add_argument("--cluster-ids", metavar="PATH", default=None,
                   help="Also write the int32 cluster ids of the whole lung (0: no cluster; 1 = the largest cluster, then by "
                        "descending size): .npy = the array, .nii / .nii.gz / .mha / .mhd with the input's geometry. Needs --clusters.")
    p.add_argument("--denoise", metavar="METHOD", default=None,
                   help="Noise reduction confined to the labelled voxels (not in the reference): median[:K] (window K = 3 or 5, default "
                        "3) or gaussian:MM (sigma in mm). --stats, --clusters, --texture and --roi then measure the filtered image, and "
                        "their JSON names the filter. Computed on the GPU.")
    p.add_argument("--denoised", metavar="PATH", default=None,
                   help="Also write the --denoise filtered volume (.nii / .nii.gz / .mha / .mhd with the input's geometry, .npy the array).")
    p.add_argument("--laa-map", metavar="PATH", default=None,
                   help="Also write the low-attenuation map (not in the reference): float32, per lung voxel the Gaussian-weighted local "
                        "fraction of lung voxels below --cluster-threshold (default -950), 0 outside the lung. Same file types as "
                        "--denoised. Computed on the GPU from the unfiltered input.")
    p.add_argument("--laa-sigma", metavar="MM", type=float, default=None,
                   help="Sigma in mm of the Gaussian of --laa-map (default 5).")
    p.add_argument("--vesselness", metavar="PATH", default=None,
                   help="Also write the vesselness map (not in the reference): float32, Frangi's multi-scale measure of bright tubes at "
                        "every lung voxel, 0 outside the lung. Same file types as --denoised. Computed on the GPU; after --denoise from "
                        "the filtered image.")
    p.add_argument("--vessel-mask", metavar="PATH", default=None,
                   help="Also write the vessel mask (uint8, 1 where the vesselness reaches --vessel-threshold inside the lung eroded by "
                        "2 mm). Same file types as --denoised.")
    p.add_argument("--vessels", metavar="PATH.json", default=None,
                   help="Also write the vessel analysis as JSON: per label and for the whole lung the vessel voxels, their volume, their "
                        "share of the eroded lung and their number per scale.")
    p.add_argument("--vessel-sigmas", metavar="MM", type=float, nargs="+", default=None,
                   help="Scales of the vessel filter in mm, 1 to 8 values (default 1 1.5 2 3).")
    p.add_argument("--vessel-threshold", metavar="T", type=float, default=None,
                   help="Vesselness from which a voxel counts as vessel (default 0.5; a conventional choice, not clinically validated).")
    p.add_argument("--vessel-skeleton", metavar="PATH", default=None,
                   help="Also write the centrelines of the vessel mask (not in the reference): uint8, 0 or 1 + the number of skeleton "
                        "voxels among the 26 neighbours (2 end, 3 curve, 4 and more junction). Same file types as --denoised. Computed "
                        "on the GPU by a topology-preserving thinning.")
    p.add_argument("--vessel-calibre", metavar="PATH", default=None,
                   help="Also write the calibre class of every vessel voxel (uint8, 1 = the smallest; the class of the nearest "
                        "centreline voxel, whose radius is its distance to the outside of the vessel mask). Same file types as --denoised.")
    p.add_argument("--vessel-tree", metavar="PATH.json", default=None,
                   help="Also write the vessel tree as JSON: per label and for the whole lung the centreline voxels, segments, length in "
                        "mm, junctions, ends and the vessel volume per calibre class, and the graph of segments and junctions.")
    p.add_argument("--vessel-calibres", metavar="MM2", type=float, nargs="+", default=None,
                   help="Cross-sectional areas in mm^2 that split the calibre classes, 1 to 7 ascending values (default 5 10, the "
                        "customary BV5 / BV10 split; conventional, not clinically validated).")
    p.add_argument("--airways", metavar="PATH", default=None,
                   help="Also write the airway mask (not in the reference): uint8, 1 in the trachea and the bronchi that one global "
                        "threshold reaches from the trachea before the first wall breaks (typically lobar to segmental). Same file "
                        "types as --denoised. A minimax flood on the GPU; of the unfiltered input.")
    p.add_argument("--airway-tree", metavar="PATH.json", default=None,
                   help="Also write the airway analysis and tree as JSON: seed, threshold, volume, volume per label, and per segment "
                        "its generation, parent, length and diameter in mm.")
    p.add_argument("--airway-cost", metavar="PATH", default=None,
                   help="Also write the flood's cost map (int16): per voxel the smallest HU threshold at which region growing from the "
                        "trachea reaches it, 32767 where it never does. Same file types as --denoised.")
    p.add_argument("--airway-seed", metavar=("Z", "Y", "X"), type=int, nargs=3, default=None,
                   help="The voxel (array index z y x) the airway flood starts from (default: the trachea is looked for).")
    p.add_argument("--airway-cap", metavar="HU", type=int, default=None,
                   help="The HU value above which no voxel is ever airway (default -800).")
    p.add_argument("--airway-threshold", metavar="HU", type=int, default=None,
                   help="The airway threshold in HU (default: chosen by the explosion rule; conventional, not clinically validated).")
    p.add_argument("--resampled", metavar="PATH", default=None,
                   help="Also write the input resampled onto another grid (not in the reference): float32 (order 0: the input's type), to --resample-spacing "
                        "(default 1 mm isotropic) or onto the grid of --resample-like. .nii / .nii.gz / .mha / .mhd carry the grid's "
                        "geometry, .npy the array. Computed on the GPU; after --denoise from the filtered image.")
    p.add_argument("--resampled-labels", metavar="PATH", default=None,
                   help="Also write the result's labels resampled onto the same grid (uint8). Same file types as --resampled.")
    p.add_argument("--resample-spacing", metavar="MM", type=float, nargs="+", default=None,
                   help="Spacing in mm of the resampling grid: one value (isotropic) or three in the file's x y z order (default 1).")
    p.add_argument("--resample-like", metavar="IMAGE", default=None,
                   help="An image whose grid (size, spacing, origin, direction) the resampled volumes are written on.")
    p.add_argument("--resample-order", type=int, choices=[0, 1, 3], default=None,
                   help="Interpolation of --resampled: 0 nearest, 1 linear, 3 cubic B-spline (default 3).")
    p.add_argument("--resample-label-mode", choices=["nearest", "linear"], default=None,
                   help="Interpolation of --resampled-labels: nearest, or linear = the largest trilinear label indicator (default).")
    p.add_argument("--compare-resample", action="store_true",
                   help="Resample the --compare-to mask (nearest neighbour) onto the input's grid first when its grid differs.")
    p.add_argument("--register-moving", metavar="IMAGE", default=None,
                   help="Also register a second image onto the input by mutual information on the GPU (not in the reference), sampled in "
                        "the lungs and a 10 mm rim around them. Needs --registered PATH or --registration PATH.json.")
    p.add_argument("--registered", metavar="PATH", default=None,
                   help="Write the --register-moving image on the input's grid (cubic B-spline, float32). .nii / .nii.gz / .mha / .mhd "
                        "carry the geometry, .npy the array.")
    p.add_argument("--registration", metavar="PATH.json", default=None,
                   help="Write the registration: matrix and translation (input space to moving space, LPS mm), parameters, metric, levels.")
    p.add_argument("--register-deformable", action="store_true",
                   help="Turn --register-moving into a two-stage registration: the rigid / affine stage, then a demons displacement field "
                        "inside the same dilated lungs (not in the reference). --registered then goes through the field too.")
    p.add_argument("--register-metric", choices=["ssd", "lcc"], default=None,
                   help="The metric of --register-deformable: ssd (default), the squared intensity difference, for two scans of one "
                        "intensity scale; lcc, the local correlation metric, for an inspiration / expiration pair, whose lung density differs.")
    p.add_argument("--register-window", metavar="MM", type=float, default=None,
                   help="The window of --register-metric lcc: it reaches MM millimetres to either side (default: 4 voxels of each level; "
                        "at most 8 voxels of any level).")
    p.add_argument("--deformation", metavar="PATH", default=None,
                   help="Write the displacement field of --register-deformable (mm along the array axes z, y, x on the input's grid). "
                        ".npz (with grid and affine), .nii or .nii.gz (4-D float32).")
    p.add_argument("--jacobian", metavar="PATH", default=None,
                   help="Write the Jacobian determinant map of the field, the local volume change (float32). .npy / .nii / .nii.gz / .mha / .mhd.")
    p.add_argument("--inverse-deformation", metavar="PATH", default=None,
                   help="Write the INVERSE of the --register-deformable transform: a displacement field on the --register-moving image's "
                        "grid (mm along its array axes) over the inverse affine. .npz (with grid and affine), .nii or .nii.gz.")
    p.add_argument("--labels-on-moving", metavar="PATH", default=None,
                   help="Write the mask carried onto the --register-moving image's grid through that inverse (per-label trilinear). "
                        ".nii / .nii.gz / .mha / .mhd carry the geometry, .npy the array.")
    p.add_argument("--register-transform", choices=["translation", "rigid", "similarity", "affine"], default=None,
                   help="The transform of --register-moving (default rigid).")
    p.add_argument("--pair", metavar="PATH.json", default=None,
                   help="Write the paired analysis of the input and the --register-moving image through the registration (with "
                        "--register-deformable: through the field): per label and for the lung the parametric response map's classes, the "
                        "mass-corrected density change and the mean Jacobian (lungmask_amd.pairs).")
    p.add_argument("--pair-classes", metavar="PATH", default=None,
                   help="Write the class map of the paired analysis (uint8; 0 not classified). .nii / .nii.gz / .mha / .mhd / .npy.")
    p.add_argument("--pair-change", metavar="PATH", default=None,
                   help="Write the mass-corrected density change map of the paired analysis (float32 HU). .nii / .nii.gz / .mha / .mhd / .npy.")
    p.add_argument("--pair-roles", choices=["insp-exp", "exp-insp", "longitudinal"], default=None,
                   help="What the input and the --register-moving image are: inspiration and expiration (default), the reverse, or two "
                        "scans of the same phase.")
    p.add_argument("--pair-thresholds", metavar=("F", "M"), type=float, nargs=2, default=None,
                   help="The class thresholds in HU for the input and for the moving image (default: by --pair-roles, -950 / -856).")
    p.add_argument("--pair-range", metavar=("LO", "HI"), type=float, nargs=2, default=None,
                   help="The HU window inside which a voxel is classified (default -1000 -500).")
    return p


# Below the parser main() is four steps, each with one definition of what it repeats: the table of outputs, the check of the
# arguments, the run on the engine, the writing of the files.

# ---- 1. the outputs: the kinds of file and what each path-valued flag takes
JSON = (".json",)
VOLUME = (".nii", ".nii.gz", ".mha", ".mhd", ".npy")
CLUSTER_IDS = (".npy", ".nii", ".nii.gz", ".mha", ".mhd")  # VOLUME as the refusal of --cluster-ids lists it (the writers of volume_io take int32 as they stand)
PROBABILITIES = (".npy", ".nii", ".nii.gz")
MESH = (".stl", ".ply", ".obj")
FIELD = (".npz", ".nii", ".nii.gz")

# dest: argparse's name; noun: the X of "Save X to: PATH"; product: the value out of the results `r` of run(), asked for only when
# the flag is given; volume: the product as a Volume for the image containers where it does not lie on the input's grid.
Output = namedtuple("Output", "dest flag noun kind product volume", defaults=(None,))

# In the order the files are written.  The mask itself (args.output) and --closed are not here: they take any type that
# volume_io.save_image takes and carry the kept DICOM tags.
OUTPUTS = (
    Output("metrics", "--metrics", "metrics", JSON, lambda r: r.metrics()),
    Output("denoised", "--denoised", "denoised volume", VOLUME, lambda r: r.filtered),
    Output("laa_map", "--laa-map", "low-attenuation map", VOLUME, lambda r: r.laa),
    Output("vesselness", "--vesselness", "vesselness map", VOLUME, lambda r: r.vessels.vesselness),
    Output("vessel_mask", "--vessel-mask", "vessel mask", VOLUME, lambda r: r.vessels.mask.astype(np.uint8)),
    Output("vessel_skeleton", "--vessel-skeleton", "vessel skeleton", VOLUME, lambda r: r.vessels.skeleton),
    Output("vessel_calibre", "--vessel-calibre", "vessel calibre classes", VOLUME, lambda r: r.vessels.calibre),
    Output("vessels", "--vessels", "vessel analysis", JSON, lambda r: r.vessels.analysis),
    Output("vessel_tree", "--vessel-tree", "vessel tree", JSON, lambda r: r.vessels.tree),
    Output("airways", "--airways", "airway mask", VOLUME, lambda r: r.airways.mask),
    Output("airway_cost", "--airway-cost", "airway cost map", VOLUME, lambda r: r.airways.cost),
    Output("airway_tree", "--airway-tree", "airway tree", JSON, lambda r: r.airways.meta()),
    Output("mesh", "--mesh", "mesh", MESH, lambda r: r.meshes),
    Output("roi", "--roi", "ROI", VOLUME, lambda r: r.roi.image, lambda r: r.roi.as_volume()),
    Output("resampled", "--resampled", "resampled volume", VOLUME, lambda r: r.resampled.image, lambda r: r.resampled.as_volume()),
    Output("resampled_labels", "--resampled-labels", "resampled labels", VOLUME, lambda r: r.resampled.labels,
           lambda r: r.resampled.labels_volume()),
    Output("registered", "--registered", "registered image", VOLUME, lambda r: r.registration.image),
    Output("deformation", "--deformation", "displacement field", FIELD, lambda r: r.registration.field),
    Output("jacobian", "--jacobian", "Jacobian determinant", VOLUME, lambda r: r.registration.jacobian(engine=r.engine)[0]),
    Output("inverse_deformation", "--inverse-deformation", "inverse displacement field", FIELD, lambda r: r.registration.inverse_field),
    Output("labels_on_moving", "--labels-on-moving", "labels on the moving grid", VOLUME, lambda r: r.registration.labels_on_moving,
           lambda r: r.moving.like(r.registration.labels_on_moving)),
    Output("pair_classes", "--pair-classes", "pair class map", VOLUME, lambda r: r.pair.classes),
    Output("pair_change", "--pair-change", "pair density change map", VOLUME, lambda r: r.pair.change),
    Output("pair", "--pair", "paired analysis", JSON, lambda r: r.pair.analysis),
    Output("registration", "--registration", "registration", JSON, lambda r: r.registration.meta()),
    Output("clusters", "--clusters", "cluster analysis", JSON, lambda r: r.clusters),
    Output("cluster_ids", "--cluster-ids", "cluster ids", CLUSTER_IDS, lambda r: r.cluster_ids),
    Output("texture", "--texture", "texture features", JSON, lambda r: r.texture),
    Output("stats", "--stats", "statistics", JSON, lambda r: r.stats),
    Output("probabilities", "--probabilities", "probabilities", PROBABILITIES, lambda r: r.probs),
)


def use(extensions):
    """The extensions as a refusal names them: '.npy, .nii or .nii.gz'."""
    return extensions[0] if len(extensions) == 1 else ", ".join(extensions[:-1]) + " or " + extensions[-1]


# ---- 2. the check of the arguments
TREE_OUTPUTS = ("vessel_skeleton", "vessel_calibre", "vessel_tree")
VESSEL_OUTPUTS = ("vesselness", "vessel_mask", "vessels") + TREE_OUTPUTS
AIRWAY_OUTPUTS = ("airways", "airway_cost", "airway_tree")
RESAMPLE_OUTPUTS = ("resampled", "resampled_labels")
INVERSE_OUTPUTS = ("inverse_deformation", "labels_on_moving")
PAIR_OUTPUTS = ("pair", "pair_classes", "pair_change")
GO_TOGETHER = "--compare-to MASK and --metrics PATH.json go together"
NEED_CLUSTERS = "--cluster-threshold HU, --cluster-connectivity N and --cluster-ids PATH need --clusters PATH.json"

# (any of these given, none of these given, the refusal)
NEEDS = (
    (("texture_bin_width", "texture_range"), ("texture",), "--texture-bin-width HU and --texture-range LO HI need --texture PATH.json"),
    (("compare_to",), ("metrics",), GO_TOGETHER),
    (("metrics",), ("compare_to",), GO_TOGETHER),
    (("roi_spacing",), ("roi",), "--roi-spacing MM needs --roi PATH"),
    (("mesh_smooth",), ("mesh",), "--mesh-smooth N needs --mesh PATH"),
    (("close_mm",), ("closed",), "--close-mm MM needs --closed PATH"),
    (("cluster_threshold",), ("clusters", "laa_map"), NEED_CLUSTERS),  # (the threshold is also that of --laa-map)
    (("cluster_connectivity", "cluster_ids"), ("clusters",), NEED_CLUSTERS),
    (("denoised",), ("denoise",), "--denoised PATH needs --denoise METHOD"),
    (("laa_sigma",), ("laa_map",), "--laa-sigma MM needs --laa-map PATH"),
    (("vessel_calibres",), TREE_OUTPUTS, "--vessel-calibres MM2 needs --vessel-skeleton PATH, --vessel-calibre PATH or --vessel-tree PATH.json"),
    (("vessel_sigmas", "vessel_threshold"), VESSEL_OUTPUTS,
     "--vessel-sigmas MM and --vessel-threshold T need --vesselness PATH, --vessel-mask PATH, --vessels PATH.json, "
     "--vessel-skeleton PATH, --vessel-calibre PATH or --vessel-tree PATH.json"),
    (("airway_seed", "airway_cap", "airway_threshold"), AIRWAY_OUTPUTS,
     "--airway-seed Z Y X, --airway-cap HU and --airway-threshold HU need --airways PATH, --airway-tree PATH.json or --airway-cost PATH"),
    (("resample_spacing", "resample_like", "resample_order", "resample_label_mode"), RESAMPLE_OUTPUTS,
     "--resample-spacing MM, --resample-like IMAGE, --resample-order N and --resample-label-mode MODE need --resampled PATH "
     "or --resampled-labels PATH"),
    (("compare_resample",), ("compare_to",), "--compare-resample needs --compare-to MASK"),
    (("registered", "registration", "register_transform"), ("register_moving",),
     "--registered PATH, --registration PATH.json and --register-transform KIND need --register-moving IMAGE"),
    (("deformation", "jacobian"), ("register_deformable",), "--deformation PATH and --jacobian PATH need --register-deformable"),
    (INVERSE_OUTPUTS, ("register_deformable",), "--inverse-deformation PATH and --labels-on-moving PATH need --register-deformable"),
    (("register_metric", "register_window"), ("register_deformable",), "--register-metric NAME and --register-window MM need --register-deformable"),
    (("register_deformable",), ("register_moving",), "--register-deformable needs --register-moving IMAGE"),
    (("pair_roles", "pair_thresholds", "pair_range"), PAIR_OUTPUTS,
     "--pair-roles, --pair-thresholds and --pair-range need --pair PATH.json, --pair-classes PATH or --pair-change PATH"),
    (PAIR_OUTPUTS, ("register_moving",), "--pair PATH.json, --pair-classes PATH and --pair-change PATH need --register-moving IMAGE"),
    (("register_moving",), ("registered", "registration", "deformation", "jacobian") + INVERSE_OUTPUTS + PAIR_OUTPUTS,
     "--register-moving IMAGE needs --registered PATH or --registration PATH.json"),
)


def parse_denoise(text):
    """--denoise median[:K] | gaussian:MM -> (keyword arguments of LMInferer.apply_denoised, the JSON entry)."""
    method, _, par = text.partition(":")
    try:
        if method == "median":
            k = int(par) if par else 3
            if k not in (3, 5):
                raise ValueError
            return dict(method="median", size=k), {"method": "median", "size": k, "masked": True}
        if method == "gaussian":
            mm = float(par)
            if not (0 < mm < float("inf")):
                raise ValueError
            return dict(method="gaussian", sigma_mm=mm), {"method": "gaussian", "sigma_mm": mm, "masked": True}
    except ValueError:
        pass
    sys.exit(f"--denoise: median, median:3, median:5 or gaussian:MM with MM > 0, got {text!r}")


def check_arguments(args):
    """Every refusal of an argv that parses, before anything is loaded -> the keyword arguments and the want_* flags of run().

    An argv with one fault gets that fault's text.  Of several faults the first in this order is reported: a flag without the
    flag it needs (in the order of NEEDS), two flags that exclude each other, a file type (in the order of OUTPUTS), a value
    (in the order of the lines below), a file that does not exist (--compare-to, --resample-like, --register-moving)."""
    def given(dest):
        return getattr(args, dest) is not None and getattr(args, dest) is not False

    for flags, needed, text in NEEDS:
        if any(map(given, flags)) and not any(map(given, needed)):
            sys.exit(text)
    if args.resample_spacing is not None and args.resample_like is not None:
        sys.exit("--resample-spacing MM and --resample-like IMAGE exclude each other")
    if args.probabilities is not None and args.modelname == "LTRCLobes_R231":
        sys.exit("--probabilities is not available with --modelname LTRCLobes_R231: the fused mode has labels only "
                 "(run LTRCLobes and R231 on their own for their probabilities)")
    for o in OUTPUTS:
        dest = getattr(args, o.dest)
        if dest is not None and not dest.lower().endswith(o.kind):
            sys.exit(f"{o.flag}: unsupported file type {dest!r} (use {use(o.kind)})")

    c = SimpleNamespace(want_tree=any(map(given, TREE_OUTPUTS)), want_vessels=any(map(given, VESSEL_OUTPUTS)),
                        want_airways=any(map(given, AIRWAY_OUTPUTS)), want_resampled=any(map(given, RESAMPLE_OUTPUTS)), want_register=args.register_moving is not None,
                        want_deform=bool(args.register_deformable), want_inverse=any(map(given, INVERSE_OUTPUTS)),
                        want_pair=any(map(given, PAIR_OUTPUTS)), transform=args.register_transform or "rigid")
    c.texture_kw = {}
    if args.texture is not None:
        c.texture_kw = dict(hu_range=tuple(args.texture_range or (-1000, 199)), bin_width=25 if args.texture_bin_width is None else args.texture_bin_width)
        try:
            lmtexture.check_parameters(c.texture_kw["hu_range"], c.texture_kw["bin_width"], 1)
        except ValueError as e:
            sys.exit(f"--texture: {e}")
    if args.roi_spacing is not None and not (0 < args.roi_spacing < float("inf")):
        sys.exit(f"--roi-spacing: a positive spacing in mm, got {args.roi_spacing!r}")
    if args.mesh_smooth is not None and not 0 <= args.mesh_smooth <= 100000:
        sys.exit(f"--mesh-smooth: a number of iterations in 0..100000, got {args.mesh_smooth!r}")
    c.mesh_kw = dict(per_label="{label}" in (args.mesh or ""), smooth=args.mesh_smooth or 0)
    if args.close_mm is not None and not (0 <= args.close_mm < float("inf")):
        sys.exit(f"--close-mm: a radius in mm >= 0, got {args.close_mm!r}")
    c.close_mm = 10.0 if args.close_mm is None else args.close_mm
    c.denoise_kw, c.denoise_meta = (None, None) if args.denoise is None else parse_denoise(args.denoise)
    if args.laa_sigma is not None and not (0 < args.laa_sigma < float("inf")):
        sys.exit(f"--laa-sigma: a sigma in mm > 0, got {args.laa_sigma!r}")
    c.laa_sigma = 5.0 if args.laa_sigma is None else args.laa_sigma
    if args.cluster_threshold is not None and not -2 ** 31 < args.cluster_threshold < 2 ** 31:
        sys.exit(f"--cluster-threshold: an HU value in the int32 range, got {args.cluster_threshold!r}")
    c.cluster_kw = dict(threshold=-950 if args.cluster_threshold is None else args.cluster_threshold, connectivity=args.cluster_connectivity or 6)
    c.calibres = tuple(args.vessel_calibres or (5.0, 10.0))
    if c.want_tree:
        try:
            lmskeleton.calibre_edges_mm(c.calibres)
        except ValueError as e:
            sys.exit(f"--vessel-calibres: {e}")
    c.vessel_kw = dict(sigmas_mm=tuple(args.vessel_sigmas or (1.0, 1.5, 2.0, 3.0)), threshold=0.5 if args.vessel_threshold is None else args.vessel_threshold)
    if c.want_vessels:
        try:
            lmvessels.scale_sigmas(c.vessel_kw["sigmas_mm"])
            lmvessels.check_analysis_arguments(c.vessel_kw["threshold"], 2.0)
        except ValueError as e:
            sys.exit(f"--vessel-sigmas / --vessel-threshold: {e}")
    c.airway_kw = dict(seed=None if args.airway_seed is None else tuple(args.airway_seed),
                       cap_hu=lmairways.DEFAULT_CAP_HU if args.airway_cap is None else args.airway_cap, threshold=args.airway_threshold)
    if c.want_airways:
        try:
            lmairways.check_arguments(**c.airway_kw)
        except ValueError as e:
            sys.exit(f"--airway-seed / --airway-cap / --airway-threshold: {e}")
    spacing = args.resample_spacing
    if spacing is not None and (len(spacing) not in (1, 3) or not all(0 < v < float("inf") for v in spacing)):
        sys.exit(f"--resample-spacing: one positive spacing in mm or three (x y z), got {spacing!r}")
    c.resample_kw = dict(order=3 if args.resample_order is None else args.resample_order, label_mode=args.resample_label_mode or "linear")
    if spacing is not None:  # (array axis order)
        c.resample_kw["spacing_out"] = spacing[0] if len(spacing) == 1 else tuple(spacing[::-1])
    if args.register_window is not None and args.register_metric != "lcc":
        sys.exit("--register-window MM needs --register-metric lcc")
    if args.register_window is not None and not (0 < args.register_window < float("inf")):
        sys.exit(f"--register-window: a length in mm > 0, got {args.register_window!r}")
    c.deform_kw = {}  # (without the two flags: the calls are what they were)
    if args.register_metric is not None:
        c.deform_kw["metric"] = args.register_metric
    if args.register_window is not None:
        c.deform_kw["window_mm"] = args.register_window
    c.pair_kw = {}
    if c.want_pair:
        c.pair_kw = dict(roles={"insp-exp": ("inspiration", "expiration"), "exp-insp": ("expiration", "inspiration"),
                                "longitudinal": None}[args.pair_roles or "insp-exp"],
                         maps=("classes", "change"))
        if args.pair_thresholds is not None:
            c.pair_kw["fixed_threshold"], c.pair_kw["moving_threshold"] = args.pair_thresholds
        if args.pair_range is not None:
            c.pair_kw["hu_range"] = tuple(args.pair_range)
        try:
            lmpairs.check_arguments(**c.pair_kw)
        except ValueError as e:
            sys.exit(f"--pair: {e}")
    for dest in ("compare_to", "resample_like", "register_moving"):
        if getattr(args, dest) is not None and not os.path.exists(getattr(args, dest)):
            sys.exit(f"File not found: {getattr(args, dest)}")
    return c


# ---- 3. the run on the engine
def apply_once(args, c, inferer, r):
    """The one apply* call that gets the volume: the first product in this order comes back from the labelling's own upload,
    every other one is computed beside() it from the labels."""
    image, moving = r.image, r.moving
    if args.denoise is not None and args.probabilities is None:
        r.result, r.filtered = inferer.apply_denoised(image, **c.denoise_kw)
    elif args.probabilities is not None:
        r.result, r.probs = inferer.apply_probabilities(image)  # the labels are those of apply(image)
    elif args.stats is not None:
        r.result, r.stats = inferer.apply_with_stats(image)
    elif args.texture is not None:
        r.result, r.texture = inferer.apply_with_texture(image, **c.texture_kw)
    elif args.roi is not None:
        r.result, r.roi = inferer.apply_roi(image, spacing_out=args.roi_spacing)
    elif args.mesh is not None:
        r.result, r.meshes = inferer.apply_mesh(image, **c.mesh_kw)
    elif args.closed is not None:
        r.result, r.closed = inferer.apply_closed(image, radius_mm=c.close_mm)
    elif args.clusters is not None:
        r.result, r.clusters = inferer.apply_with_clusters(image, **c.cluster_kw)
    elif c.want_tree:
        r.result, r.vessels = inferer.apply_with_vessel_tree(image, calibres_mm2=c.calibres, **c.vessel_kw)
    elif c.want_vessels:
        r.result, r.vessels = inferer.apply_with_vessels(image, **c.vessel_kw)
    elif c.want_airways:
        r.result, r.airways = inferer.apply_with_airways(image, **c.airway_kw)
    elif c.want_resampled:
        r.result, r.resampled = inferer.apply_resampled(image, **c.resample_kw)
    elif c.want_pair and not c.want_inverse:
        extra = dict(deformable_kw=c.deform_kw) if c.deform_kw else {}
        r.result, r.registration, r.pair = inferer.apply_pair(image, moving, deformable=c.want_deform, transform=c.transform, **c.pair_kw, **extra)
    elif c.want_deform:
        r.result, r.registration = inferer.apply_deformable(image, moving, transform=c.transform, inverse=c.want_inverse, **c.deform_kw)
    elif c.want_register:
        r.result, r.registration = inferer.apply_registered(image, moving, transform=c.transform)
    else:
        r.result = inferer.apply(image)


def labelling(inferer, r):
    """(n_labels, names) of the model's labels: asked of the engine once, by the first product that needs them (a run without
    such a product does not ask)."""
    if r.labelling is None:
        n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
        r.labelling = n_labels, lmstats.label_names(inferer.modelname, n_labels)
    return r.labelling


def register_beside(c, r):
    """--register-moving beside another product: on the labels' 10 mm rim, as LMInferer's own registration."""
    image, moving, labels, engine = r.image, r.moving, r.image.like(r.result), r.engine
    if not np.any(r.result):
        sys.exit("--register-moving: no voxel is labelled, nothing to register on")
    rim = lmmorph.dilate(labels, 10.0, engine=engine)
    registration = lmreg.register(image, moving, c.transform, labels=rim, engine=engine)
    if c.want_deform:
        first = registration
        registration = lmdef.register_deformable(image, moving, initial=first, labels=rim, engine=engine, **c.deform_kw)
        registration.affine_registration = first
    registration.image = registration.resample(moving, engine=engine).array
    if c.want_inverse:
        registration.labels_on_moving = registration.resample_to_moving(labels, engine=engine).array
    return registration


def beside(args, c, inferer, r):
    """Every wanted product that apply_once() did not return, from the labels it returned.  --stats, --clusters, --texture, --roi,
    the vessels and the resampling measure the input or, after --denoise, its filtered form."""
    image, result, engine = r.image, r.result, r.engine
    measured = image
    if args.denoise is not None:
        if r.filtered is None and np.any(result):  # beside --probabilities
            if c.denoise_kw["method"] == "median":
                r.filtered = lmfilters.median(image, c.denoise_kw["size"], labels=result, engine=engine)
            else:
                r.filtered = lmfilters.gaussian(image, c.denoise_kw["sigma_mm"], labels=result, engine=engine)
        elif r.filtered is None:  # no labelled voxel: nothing is filtered
            r.filtered = np.asarray(image.array) if c.denoise_kw["method"] == "median" else np.asarray(image.array, dtype=np.float32)
        measured = image.like(r.filtered)
    if args.stats is not None and r.stats is None:
        n_labels, names = labelling(inferer, r)
        r.stats = lmstats.label_statistics(measured, result, names=names, engine=engine, n_labels=n_labels)
    if c.want_vessels and r.vessels is None:
        _, names = labelling(inferer, r)
        if c.want_tree:
            r.vessels = lmskeleton.vessel_tree(measured, result, calibres_mm2=c.calibres, names=names, engine=engine, **c.vessel_kw)
        else:
            r.vessels = lmvessels.vessel_result(measured, result, names=names, engine=engine, **c.vessel_kw)
    if c.want_airways and r.airways is None:  # (of the unfiltered input: a smoothed wall is a broken wall)
        _, names = labelling(inferer, r)
        r.airways = lmairways.segment_or_empty(image, result, names=names, engine=engine, **c.airway_kw)
    if args.laa_map is not None:  # (of the unfiltered input)
        r.laa = np.zeros(result.shape, np.float32)
        if np.any(result):
            r.laa = lmfilters.low_attenuation_map(image, result, threshold=c.cluster_kw["threshold"], sigma_mm=c.laa_sigma, engine=engine)
    if args.clusters is not None and r.clusters is None:
        _, names = labelling(inferer, r)
        r.clusters = lmcomp.cluster_analysis(measured, result, names=names, engine=engine, **c.cluster_kw)
    if args.cluster_ids is not None:  # the whole lung's clusters, largest first
        r.cluster_ids = lmcomp.find_components(measured, result, hu_range=lmcomp.cluster_range(c.cluster_kw["threshold"]), per_label=False,
                                               connectivity=c.cluster_kw["connectivity"], order="size", engine=engine).ids
    if args.closed is not None and r.closed is None:
        r.closed = lmmorph.close(image.like(result), c.close_mm, engine=engine) if np.any(result) else np.array(result, copy=True)
    if args.texture is not None and r.texture is None:
        n_labels, names = labelling(inferer, r)
        r.texture = lmtexture.texture_features(measured, result, n_labels=n_labels, names=names, engine=engine, **c.texture_kw)
    if args.mesh is not None and r.meshes is None:
        r.meshes = lmmesh.extract_surfaces(image.like(result), engine=engine, **c.mesh_kw)
    if args.roi is not None and r.roi is None:
        r.roi = lmroi.extract_roi(measured, result, spacing_out=args.roi_spacing, engine=engine)
    if c.want_resampled and r.resampled is None:
        kw = c.resample_kw
        grid = kw.get("like") or lmresample.Grid.isotropic(image, kw.get("spacing_out", 1.0))
        img = lmresample.resample_image(measured, grid, order=kw["order"], dtype=None if kw["order"] == 0 else np.float32, engine=engine)
        lab = lmresample.resample_labels(image.like(result), grid, mode=kw["label_mode"], engine=engine)
        r.resampled = lmresample.Resampled(img.array, lab.array, grid, kw["order"], kw["label_mode"], True)
    if c.want_register and r.registration is None:
        r.registration = register_beside(c, r)
    if c.want_pair and r.pair is None:  # through the registration, whoever made it
        n_labels, names = labelling(inferer, r)
        r.pair = lmpairs.pair_analysis(image, r.moving, image.like(result), r.registration, n_labels=n_labels, names=names, engine=engine,
                                       **c.pair_kw)


def compare(args, inferer, r):
    """--metrics: the agreement of the result with the --compare-to mask."""
    n_labels, names = labelling(inferer, r)
    other = volume_io.load_input_image(args.compare_to)
    if args.compare_to.lower().endswith((".npy", ".npz")):  # a bare array: it lies on the input's grid
        other = r.image.like(np.asarray(other.array))
    return lmmetrics.compare_labels(r.image.like(r.result), other, n_labels=n_labels, names=names, engine=r.engine,
                                    resample_b=args.compare_resample)


def run(args, c):
    """Loads the images, makes the inferer and its one apply* call, then the other products -> the results, every product that
    was not asked for None."""
    logger.info("Load model")
    image = volume_io.load_input_image(args.input)  # utils.load_input_image (utils.py:233-269)
    logger.info("Infer lungmask")
    if args.modelname == "LTRCLobes_R231":
        assert args.modelpath is None, "Modelpath can not be specified for LTRCLobes_R231 mode"
        inferer = LMInferer(modelname="LTRCLobes", force_cpu=args.cpu, fillmodel="R231", batch_size=args.batchsize,
                            volume_postprocessing=not args.nopostprocess, tqdm_disable=args.noprogress)
    else:
        inferer = LMInferer(modelname=args.modelname, modelpath=args.modelpath, force_cpu=args.cpu, batch_size=args.batchsize,
                            volume_postprocessing=not args.nopostprocess, tqdm_disable=args.noprogress)
    r = SimpleNamespace(image=image, moving=None, engine=inferer.engine, labelling=None, result=None, probs=None, stats=None, roi=None,
                        meshes=None, texture=None, closed=None, clusters=None, cluster_ids=None, filtered=None, laa=None, vessels=None,
                        airways=None, resampled=None, registration=None, pair=None, metrics=None)
    if c.want_register:
        r.moving = volume_io.load_input_image(args.register_moving)
    if args.resample_like is not None:
        c.resample_kw["like"] = lmresample.Grid.of(volume_io.load_input_image(args.resample_like))
    apply_once(args, c, inferer, r)
    beside(args, c, inferer, r)
    r.metrics = functools.partial(compare, args, inferer, r)  # made when they are written: after the mask, like the Jacobian map
    return r


# ---- 4. the writing of the files
def save_array(dest, noun, array, save_container):
    """An array or volume product: .npy takes the array as it is, every other type is written by `save_container()`, which makes
    the Volume only then (the ROI and the resampling of a bare array have no geometry to make one of)."""
    logger.info(f"Save {noun} to: {dest}")
    if dest.lower().endswith(".npy"):
        np.save(dest, array)
    else:
        save_container()


def save_json(dest, noun, obj):
    logger.info(f"Save {noun} to: {dest}")
    with open(dest, "w") as f:
        json.dump(obj, f, indent=2)


def write(args, c, r):
    """The mask, --closed, then the OUTPUTS that were asked for, in their order."""
    image = r.image
    logger.info(f"Save result to: {args.output}")
    keep = None
    if not args.removemetadata:  # __main__.py:125-141 (only formats that store tags use them)
        keep = {k: v for k, v in image.meta.items() if k in DICOM_METADATA_TO_KEEP}
        keep.update({"0008|103e": "Created with lungmask", "0028|1050": "1", "0028|1051": "2"})
    volume_io.save_image(args.output, image.like(r.result), keep)
    if r.closed is not None:
        logger.info(f"Save closed mask to: {args.closed}")
        volume_io.save_image(args.closed, image.like(r.closed), keep)
    # The JSON of what measured the filtered image names the filter.  (Stamped before the loop, not between its array and its
    # JSON outputs: it touches none of the arrays and precedes every JSON it touches, so no file differs.)
    if c.denoise_meta is not None:
        for product in (r.stats, r.clusters, r.texture, getattr(r.vessels, "analysis", None), getattr(r.vessels, "tree", None)):
            if product is not None:
                product["denoise"] = c.denoise_meta
    for o in OUTPUTS:
        dest = getattr(args, o.dest)
        if dest is None:
            continue
        value = o.product(r)
        if o.kind is JSON:
            save_json(dest, o.noun, value)
        elif o.kind is MESH:  # {label} in the path: one file per label
            for k, m in value.items():
                logger.info(f"Save {o.noun} to: {dest.replace('{label}', str(k))}")
                m.save(dest.replace("{label}", str(k)))
        elif o.kind is FIELD:
            logger.info(f"Save {o.noun} to: {dest}")
            value.save(dest)
        elif o.kind is PROBABILITIES:
            save_array(dest, o.noun, value, lambda: volume_io.write_nifti_channels(dest, image, value))
        else:
            volume = o.volume or (lambda r: image.like(value))
            save_array(dest, o.noun, value, lambda: volume_io.save_image(dest, volume(r)))


def main(argv=None):
    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    checked = check_arguments(args)
    results = run(args, checked)
    write(args, checked, results)
    return 0


if __name__ == "__main__":
    sys.exit(main())
