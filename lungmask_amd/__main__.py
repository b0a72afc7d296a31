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
import os
import sys

import numpy as np

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


PROB_EXTENSIONS = (".npy", ".nii", ".nii.gz")
ROI_EXTENSIONS = (".nii", ".nii.gz", ".mha", ".mhd", ".npy")
CLUSTER_ID_EXTENSIONS = (".npy", ".nii", ".nii.gz", ".mha", ".mhd")  # (the writers of volume_io take int32 as they stand)


def main(argv=None):
    from . import volume_io

    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    keepmetadata = not args.removemetadata
    if args.probabilities is not None:  # refused before anything is loaded
        if not args.probabilities.lower().endswith(PROB_EXTENSIONS):
            sys.exit(f"--probabilities: unsupported file type {args.probabilities!r} (use .npy, .nii or .nii.gz)")
        if args.modelname == "LTRCLobes_R231":
            sys.exit("--probabilities is not available with --modelname LTRCLobes_R231: the fused mode has labels only "
                     "(run LTRCLobes and R231 on their own for their probabilities)")
    if args.stats is not None and not args.stats.lower().endswith(".json"):  # refused before anything is loaded
        sys.exit(f"--stats: unsupported file type {args.stats!r} (use .json)")
    texture_kw = {}
    if args.texture is not None or args.texture_bin_width is not None or args.texture_range is not None:  # refused before anything is loaded
        from . import texture as lmtexture

        if args.texture is None:
            sys.exit("--texture-bin-width HU and --texture-range LO HI need --texture PATH.json")
        if not args.texture.lower().endswith(".json"):
            sys.exit(f"--texture: unsupported file type {args.texture!r} (use .json)")
        texture_kw = dict(hu_range=tuple(args.texture_range or (-1000, 199)), bin_width=25 if args.texture_bin_width is None else args.texture_bin_width)
        try:
            lmtexture.check_parameters(texture_kw["hu_range"], texture_kw["bin_width"], 1)
        except ValueError as e:
            sys.exit(f"--texture: {e}")
    if (args.compare_to is None) != (args.metrics is None):  # refused before anything is loaded
        sys.exit("--compare-to MASK and --metrics PATH.json go together")
    if args.metrics is not None and not args.metrics.lower().endswith(".json"):
        sys.exit(f"--metrics: unsupported file type {args.metrics!r} (use .json)")
    if args.compare_to is not None and not os.path.exists(args.compare_to):
        sys.exit(f"File not found: {args.compare_to}")
    if args.roi is not None and not args.roi.lower().endswith(ROI_EXTENSIONS):  # refused before anything is loaded
        sys.exit(f"--roi: unsupported file type {args.roi!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.roi_spacing is not None and args.roi is None:
        sys.exit("--roi-spacing MM needs --roi PATH")
    if args.roi_spacing is not None and not (0 < args.roi_spacing < float("inf")):
        sys.exit(f"--roi-spacing: a positive spacing in mm, got {args.roi_spacing!r}")
    if args.mesh is not None and not args.mesh.lower().endswith((".stl", ".ply", ".obj")):  # refused before anything is loaded
        sys.exit(f"--mesh: unsupported file type {args.mesh!r} (use .stl, .ply or .obj)")
    if args.mesh_smooth is not None and args.mesh is None:
        sys.exit("--mesh-smooth N needs --mesh PATH")
    if args.mesh_smooth is not None and not 0 <= args.mesh_smooth <= 100000:
        sys.exit(f"--mesh-smooth: a number of iterations in 0..100000, got {args.mesh_smooth!r}")
    if args.close_mm is not None and args.closed is None:  # refused before anything is loaded
        sys.exit("--close-mm MM needs --closed PATH")
    if args.close_mm is not None and not (0 <= args.close_mm < float("inf")):
        sys.exit(f"--close-mm: a radius in mm >= 0, got {args.close_mm!r}")
    close_mm = 10.0 if args.close_mm is None else args.close_mm
    if args.clusters is None and ((args.cluster_threshold is not None and args.laa_map is None) or args.cluster_connectivity is not None or
                                  args.cluster_ids is not None):
        sys.exit("--cluster-threshold HU, --cluster-connectivity N and --cluster-ids PATH need --clusters PATH.json")  # refused before anything is loaded
    denoise_kw = denoise_meta = None
    if args.denoise is not None:  # refused before anything is loaded
        denoise_kw, denoise_meta = parse_denoise(args.denoise)
    if args.denoised is not None and args.denoise is None:
        sys.exit("--denoised PATH needs --denoise METHOD")
    for flag, value in (("--denoised", args.denoised), ("--laa-map", args.laa_map)):
        if value is not None and not value.lower().endswith(ROI_EXTENSIONS):
            sys.exit(f"{flag}: unsupported file type {value!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.laa_sigma is not None and args.laa_map is None:
        sys.exit("--laa-sigma MM needs --laa-map PATH")
    if args.laa_sigma is not None and not (0 < args.laa_sigma < float("inf")):
        sys.exit(f"--laa-sigma: a sigma in mm > 0, got {args.laa_sigma!r}")
    if args.clusters is not None and not args.clusters.lower().endswith(".json"):
        sys.exit(f"--clusters: unsupported file type {args.clusters!r} (use .json)")
    if args.cluster_ids is not None and not args.cluster_ids.lower().endswith(CLUSTER_ID_EXTENSIONS):
        sys.exit(f"--cluster-ids: unsupported file type {args.cluster_ids!r} (use .npy, .nii, .nii.gz, .mha or .mhd)")
    if args.cluster_threshold is not None and not -2 ** 31 < args.cluster_threshold < 2 ** 31:
        sys.exit(f"--cluster-threshold: an HU value in the int32 range, got {args.cluster_threshold!r}")
    cluster_kw = dict(threshold=-950 if args.cluster_threshold is None else args.cluster_threshold, connectivity=args.cluster_connectivity or 6)
    want_tree = args.vessel_skeleton is not None or args.vessel_calibre is not None or args.vessel_tree is not None
    if not want_tree and args.vessel_calibres is not None:  # refused before anything is loaded
        sys.exit("--vessel-calibres MM2 needs --vessel-skeleton PATH, --vessel-calibre PATH or --vessel-tree PATH.json")
    for flag, value in (("--vessel-skeleton", args.vessel_skeleton), ("--vessel-calibre", args.vessel_calibre)):
        if value is not None and not value.lower().endswith(ROI_EXTENSIONS):
            sys.exit(f"{flag}: unsupported file type {value!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.vessel_tree is not None and not args.vessel_tree.lower().endswith(".json"):
        sys.exit(f"--vessel-tree: unsupported file type {args.vessel_tree!r} (use .json)")
    calibres = tuple(args.vessel_calibres or (5.0, 10.0))
    if want_tree:
        from . import skeleton as lmskeleton

        try:
            lmskeleton.calibre_edges_mm(calibres)
        except ValueError as e:
            sys.exit(f"--vessel-calibres: {e}")
    want_vessels = args.vesselness is not None or args.vessel_mask is not None or args.vessels is not None or want_tree
    if not want_vessels and (args.vessel_sigmas is not None or args.vessel_threshold is not None):  # refused before anything is loaded
        sys.exit("--vessel-sigmas MM and --vessel-threshold T need --vesselness PATH, --vessel-mask PATH, --vessels PATH.json, "
                 "--vessel-skeleton PATH, --vessel-calibre PATH or --vessel-tree PATH.json")
    for flag, value in (("--vesselness", args.vesselness), ("--vessel-mask", args.vessel_mask)):
        if value is not None and not value.lower().endswith(ROI_EXTENSIONS):
            sys.exit(f"{flag}: unsupported file type {value!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.vessels is not None and not args.vessels.lower().endswith(".json"):
        sys.exit(f"--vessels: unsupported file type {args.vessels!r} (use .json)")
    vessel_kw = dict(sigmas_mm=tuple(args.vessel_sigmas or (1.0, 1.5, 2.0, 3.0)), threshold=0.5 if args.vessel_threshold is None else args.vessel_threshold)
    if want_vessels:
        from . import vessels as lmvessels

        try:
            lmvessels.scale_sigmas(vessel_kw["sigmas_mm"])
            lmvessels.check_analysis_arguments(vessel_kw["threshold"], 2.0)
        except ValueError as e:
            sys.exit(f"--vessel-sigmas / --vessel-threshold: {e}")
    want_resampled = args.resampled is not None or args.resampled_labels is not None
    if not want_resampled and (args.resample_spacing is not None or args.resample_like is not None or args.resample_order is not None or
                               args.resample_label_mode is not None):  # refused before anything is loaded
        sys.exit("--resample-spacing MM, --resample-like IMAGE, --resample-order N and --resample-label-mode MODE need --resampled PATH "
                 "or --resampled-labels PATH")
    for flag, value in (("--resampled", args.resampled), ("--resampled-labels", args.resampled_labels)):
        if value is not None and not value.lower().endswith(ROI_EXTENSIONS):
            sys.exit(f"{flag}: unsupported file type {value!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.resample_spacing is not None and args.resample_like is not None:
        sys.exit("--resample-spacing MM and --resample-like IMAGE exclude each other")
    if args.resample_spacing is not None and (len(args.resample_spacing) not in (1, 3) or
                                              not all(0 < v < float("inf") for v in args.resample_spacing)):
        sys.exit(f"--resample-spacing: one positive spacing in mm or three (x y z), got {args.resample_spacing!r}")
    if args.resample_like is not None and not os.path.exists(args.resample_like):
        sys.exit(f"File not found: {args.resample_like}")
    if args.compare_resample and args.compare_to is None:
        sys.exit("--compare-resample needs --compare-to MASK")
    want_register = args.register_moving is not None
    if not want_register and (args.registered is not None or args.registration is not None or args.register_transform is not None):
        sys.exit("--registered PATH, --registration PATH.json and --register-transform KIND need --register-moving IMAGE")  # refused before anything is loaded
    want_deform = bool(args.register_deformable)
    if not want_deform and (args.deformation is not None or args.jacobian is not None):
        sys.exit("--deformation PATH and --jacobian PATH need --register-deformable")
    want_inverse = args.inverse_deformation is not None or args.labels_on_moving is not None
    if not want_deform and want_inverse:
        sys.exit("--inverse-deformation PATH and --labels-on-moving PATH need --register-deformable")
    if want_deform and not want_register:
        sys.exit("--register-deformable needs --register-moving IMAGE")
    want_pair = args.pair is not None or args.pair_classes is not None or args.pair_change is not None
    if not want_pair and (args.pair_roles is not None or args.pair_thresholds is not None or args.pair_range is not None):
        sys.exit("--pair-roles, --pair-thresholds and --pair-range need --pair PATH.json, --pair-classes PATH or --pair-change PATH")
    if want_pair and not want_register:
        sys.exit("--pair PATH.json, --pair-classes PATH and --pair-change PATH need --register-moving IMAGE")
    if want_register and args.registered is None and args.registration is None and args.deformation is None and args.jacobian is None \
            and not want_inverse and not want_pair:
        sys.exit("--register-moving IMAGE needs --registered PATH or --registration PATH.json")
    if args.pair is not None and not args.pair.lower().endswith(".json"):
        sys.exit(f"--pair: unsupported file type {args.pair!r} (use .json)")
    for flag, dest in (("--pair-classes", args.pair_classes), ("--pair-change", args.pair_change)):
        if dest is not None and not dest.lower().endswith(ROI_EXTENSIONS):
            sys.exit(f"{flag}: unsupported file type {dest!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    pair_kw = {}
    if want_pair:
        from . import pairs as lmpairs

        pair_kw = dict(roles={"insp-exp": ("inspiration", "expiration"), "exp-insp": ("expiration", "inspiration"),
                              "longitudinal": None}[args.pair_roles or "insp-exp"],
                       maps=("classes", "change"))
        if args.pair_thresholds is not None:
            pair_kw["fixed_threshold"], pair_kw["moving_threshold"] = args.pair_thresholds
        if args.pair_range is not None:
            pair_kw["hu_range"] = tuple(args.pair_range)
        try:
            lmpairs.check_arguments(**pair_kw)
        except ValueError as exc:
            sys.exit(f"--pair: {exc}")
    if args.inverse_deformation is not None and not args.inverse_deformation.lower().endswith((".npz", ".nii", ".nii.gz")):
        sys.exit(f"--inverse-deformation: unsupported file type {args.inverse_deformation!r} (use .npz, .nii or .nii.gz)")
    if args.labels_on_moving is not None and not args.labels_on_moving.lower().endswith(ROI_EXTENSIONS):
        sys.exit(f"--labels-on-moving: unsupported file type {args.labels_on_moving!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.deformation is not None and not args.deformation.lower().endswith((".npz", ".nii", ".nii.gz")):
        sys.exit(f"--deformation: unsupported file type {args.deformation!r} (use .npz, .nii or .nii.gz)")
    if args.jacobian is not None and not args.jacobian.lower().endswith(ROI_EXTENSIONS):
        sys.exit(f"--jacobian: unsupported file type {args.jacobian!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.registered is not None and not args.registered.lower().endswith(ROI_EXTENSIONS):
        sys.exit(f"--registered: unsupported file type {args.registered!r} (use .nii, .nii.gz, .mha, .mhd or .npy)")
    if args.registration is not None and not args.registration.lower().endswith(".json"):
        sys.exit(f"--registration: unsupported file type {args.registration!r} (use .json)")
    if want_register and not os.path.exists(args.register_moving):
        sys.exit(f"File not found: {args.register_moving}")
    resample_kw = dict(order=3 if args.resample_order is None else args.resample_order, label_mode=args.resample_label_mode or "linear")
    if args.resample_spacing is not None:  # (array axis order)
        resample_kw["spacing_out"] = args.resample_spacing[0] if len(args.resample_spacing) == 1 else tuple(args.resample_spacing[::-1])
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
    probs = stats = roi = meshes = texture = closed = clusters = filtered = vessels = resampled = registration = pair = None
    moving = volume_io.load_input_image(args.register_moving) if want_register else None
    if args.resample_like is not None:
        from . import resample as lmresample

        resample_kw["like"] = lmresample.Grid.of(volume_io.load_input_image(args.resample_like))
    mesh_kw = dict(per_label="{label}" in (args.mesh or ""), smooth=args.mesh_smooth or 0)
    if args.denoise is not None and args.probabilities is None:
        result, filtered = inferer.apply_denoised(image, **denoise_kw)
    elif args.probabilities is not None:
        result, probs = inferer.apply_probabilities(image)  # the labels are those of apply(image)
        if args.stats is not None and args.denoise is None:
            from . import stats as lmstats

            n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
            stats = lmstats.label_statistics(image, result, names=lmstats.label_names(inferer.modelname, n_labels), engine=inferer.engine,
                                             n_labels=n_labels)
    elif args.stats is not None:
        result, stats = inferer.apply_with_stats(image)
    elif args.texture is not None:
        result, texture = inferer.apply_with_texture(image, **texture_kw)
    elif args.roi is not None:
        result, roi = inferer.apply_roi(image, spacing_out=args.roi_spacing)
    elif args.mesh is not None:
        result, meshes = inferer.apply_mesh(image, **mesh_kw)
    elif args.closed is not None:
        result, closed = inferer.apply_closed(image, radius_mm=close_mm)
    elif args.clusters is not None:
        result, clusters = inferer.apply_with_clusters(image, **cluster_kw)
    elif want_tree:
        result, vessels = inferer.apply_with_vessel_tree(image, calibres_mm2=calibres, **vessel_kw)
    elif want_vessels:
        result, vessels = inferer.apply_with_vessels(image, **vessel_kw)
    elif want_resampled:
        result, resampled = inferer.apply_resampled(image, **resample_kw)
    elif want_pair and not want_inverse:
        result, registration, pair = inferer.apply_pair(image, moving, deformable=want_deform, transform=args.register_transform or "rigid", **pair_kw)
    elif want_deform:
        result, registration = inferer.apply_deformable(image, moving, transform=args.register_transform or "rigid", inverse=want_inverse)
    elif want_register:
        result, registration = inferer.apply_registered(image, moving, transform=args.register_transform or "rigid")
    else:
        result = inferer.apply(image)
    measured = image  # what --stats, --clusters, --texture and --roi measure: the input, or its --denoise filtered form
    if args.denoise is not None:
        from . import filters as lmfilters

        if filtered is None and np.any(result):  # beside --probabilities: from the labels it returned
            if denoise_kw["method"] == "median":
                filtered = lmfilters.median(image, denoise_kw["size"], labels=result, engine=inferer.engine)
            else:
                filtered = lmfilters.gaussian(image, denoise_kw["sigma_mm"], labels=result, engine=inferer.engine)
        elif filtered is None:  # no labelled voxel: nothing is filtered
            filtered = np.asarray(image.array) if denoise_kw["method"] == "median" else np.asarray(image.array, dtype=np.float32)
        measured = image.like(filtered)
        if args.stats is not None:
            from . import stats as lmstats

            n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
            stats = lmstats.label_statistics(measured, result, names=lmstats.label_names(inferer.modelname, n_labels),
                                             engine=inferer.engine, n_labels=n_labels)
    if want_vessels and vessels is None:  # beside the other products: from the labels they returned, on the image they measure
        from . import stats as lmstats

        n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
        vessel_names = lmstats.label_names(inferer.modelname, n_labels)
        if want_tree:
            vessels = lmskeleton.vessel_tree(measured, result, calibres_mm2=calibres, names=vessel_names, engine=inferer.engine, **vessel_kw)
        else:
            vessels = lmvessels.vessel_result(measured, result, names=vessel_names, engine=inferer.engine, **vessel_kw)
    laa = None
    if args.laa_map is not None:
        from . import filters as lmfilters

        laa = np.zeros(result.shape, np.float32)
        if np.any(result):
            laa = lmfilters.low_attenuation_map(image, result, threshold=cluster_kw["threshold"],
                                                sigma_mm=5.0 if args.laa_sigma is None else args.laa_sigma, engine=inferer.engine)
    if args.clusters is not None and clusters is None:  # beside the other products: from the labels they returned
        from . import components as lmcomp
        from . import stats as lmstats

        n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
        clusters = lmcomp.cluster_analysis(measured, result, names=lmstats.label_names(inferer.modelname, n_labels), engine=inferer.engine,
                                           **cluster_kw)
    cluster_ids = None
    if args.cluster_ids is not None:  # the whole lung's clusters, largest first
        from . import components as lmcomp

        cluster_ids = lmcomp.find_components(measured, result, hu_range=lmcomp.cluster_range(cluster_kw["threshold"]), per_label=False,
                                             connectivity=cluster_kw["connectivity"], order="size", engine=inferer.engine).ids
    if args.closed is not None and closed is None:  # beside the other products: from the labels they returned
        from . import morphology as lmmorph

        closed = lmmorph.close(image.like(result), close_mm, engine=inferer.engine) if np.any(result) else np.array(result, copy=True)
    if args.texture is not None and texture is None:  # beside --probabilities / --stats: from the labels they returned
        from . import stats as lmstats
        from . import texture as lmtexture

        n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
        texture = lmtexture.texture_features(measured, result, n_labels=n_labels, names=lmstats.label_names(inferer.modelname, n_labels),
                                             engine=inferer.engine, **texture_kw)
    if args.mesh is not None and meshes is None:  # beside the other products: from the labels they returned
        from . import mesh as lmmesh

        meshes = lmmesh.extract_surfaces(image.like(result), engine=inferer.engine, **mesh_kw)
    if args.roi is not None and roi is None:  # beside --probabilities / --stats: from the labels they returned
        from . import roi as lmroi

        roi = lmroi.extract_roi(measured, result, spacing_out=args.roi_spacing, engine=inferer.engine)
    if want_resampled and resampled is None:  # beside the other products: from the labels they returned, on the image they measure
        from . import resample as lmresample

        grid = resample_kw.get("like") or lmresample.Grid.isotropic(image, resample_kw.get("spacing_out", 1.0))
        order = resample_kw["order"]
        img = lmresample.resample_image(measured, grid, order=order, dtype=None if order == 0 else np.float32, engine=inferer.engine)
        lab = lmresample.resample_labels(image.like(result), grid, mode=resample_kw["label_mode"], engine=inferer.engine)
        resampled = lmresample.Resampled(img.array, lab.array, grid, order, resample_kw["label_mode"], True)
    if want_register and registration is None:  # beside the other products: from the labels they returned
        from . import morphology as lmmorph
        from . import registration as lmreg

        if not np.any(result):
            sys.exit("--register-moving: no voxel is labelled, nothing to register on")
        rim = lmmorph.dilate(image.like(result), 10.0, engine=inferer.engine)
        registration = lmreg.register(image, moving, args.register_transform or "rigid", labels=rim, engine=inferer.engine)
        if want_deform:
            from . import deformable as lmdef

            first = registration
            registration = lmdef.register_deformable(image, moving, initial=first, labels=rim, engine=inferer.engine)
            registration.affine_registration = first
        registration.image = registration.resample(moving, engine=inferer.engine).array
        if want_inverse:
            registration.labels_on_moving = registration.resample_to_moving(image.like(result), engine=inferer.engine).array
    if want_pair and pair is None:  # beside the other products: from the labels and the registration they returned
        from . import pairs as lmpairs
        from . import stats as lmstats

        n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
        pair = lmpairs.pair_analysis(image, moving, image.like(result), registration, n_labels=n_labels,
                                     names=lmstats.label_names(inferer.modelname, n_labels), engine=inferer.engine, **pair_kw)
    logger.info(f"Save result to: {args.output}")
    keep = None
    if keepmetadata:  # __main__.py:125-141 (only formats that store tags use them)
        keep = {k: v for k, v in image.meta.items() if k in DICOM_METADATA_TO_KEEP}
        keep.update({"0008|103e": "Created with lungmask", "0028|1050": "1", "0028|1051": "2"})
    volume_io.save_image(args.output, image.like(result), keep)
    if closed is not None:
        logger.info(f"Save closed mask to: {args.closed}")
        volume_io.save_image(args.closed, image.like(closed), keep)
    if args.metrics is not None:
        import json

        from . import metrics as lmmetrics
        from . import stats as lmstats

        n_labels = max(1, min(inferer.engine.n_classes(0), lmstats.MAX_LABELS))
        other = volume_io.load_input_image(args.compare_to)
        if args.compare_to.lower().endswith((".npy", ".npz")):  # a bare array: it lies on the input's grid
            other = image.like(np.asarray(other.array))
        agreement = lmmetrics.compare_labels(image.like(result), other, n_labels=n_labels,
                                             names=lmstats.label_names(inferer.modelname, n_labels), engine=inferer.engine,
                                             resample_b=args.compare_resample)
        logger.info(f"Save metrics to: {args.metrics}")
        with open(args.metrics, "w") as f:
            json.dump(agreement, f, indent=2)
    vessel_map = None if vessels is None else vessels.vesselness
    vessel_mask = None if vessels is None else vessels.mask.astype(np.uint8)
    for what, arr, dest in (("denoised volume", filtered, args.denoised), ("low-attenuation map", laa, args.laa_map),
                            ("vesselness map", vessel_map, args.vesselness), ("vessel mask", vessel_mask, args.vessel_mask),
                            ("vessel skeleton", vessels.skeleton if want_tree else None, args.vessel_skeleton),
                            ("vessel calibre classes", vessels.calibre if want_tree else None, args.vessel_calibre)):
        if dest is not None:
            logger.info(f"Save {what} to: {dest}")
            if dest.lower().endswith(".npy"):
                np.save(dest, arr)
            else:
                volume_io.save_image(dest, image.like(arr))
    if denoise_meta is not None:
        for product in (stats, clusters, texture, None if vessels is None else vessels.analysis, vessels.tree if want_tree else None):
            if product is not None:
                product["denoise"] = denoise_meta
    if args.vessels is not None:
        import json

        logger.info(f"Save vessel analysis to: {args.vessels}")
        with open(args.vessels, "w") as f:
            json.dump(vessels.analysis, f, indent=2)
    if args.vessel_tree is not None:
        import json

        logger.info(f"Save vessel tree to: {args.vessel_tree}")
        with open(args.vessel_tree, "w") as f:
            json.dump(vessels.tree, f, indent=2)
    if meshes is not None:
        for k, m in meshes.items():
            path = args.mesh.replace("{label}", str(k))
            logger.info(f"Save mesh to: {path}")
            m.save(path)
    if roi is not None:
        logger.info(f"Save ROI to: {args.roi}")
        if args.roi.lower().endswith(".npy"):
            np.save(args.roi, roi.image)
        else:
            volume_io.save_image(args.roi, roi.as_volume())
    if resampled is not None:
        for what, vol, dest in (("resampled volume", resampled.as_volume(), args.resampled),
                                ("resampled labels", resampled.labels_volume(), args.resampled_labels)):
            if dest is not None:
                logger.info(f"Save {what} to: {dest}")
                if dest.lower().endswith(".npy"):
                    np.save(dest, vol.array)
                else:
                    volume_io.save_image(dest, vol)
    if args.registered is not None:
        logger.info(f"Save registered image to: {args.registered}")
        if args.registered.lower().endswith(".npy"):
            np.save(args.registered, registration.image)
        else:
            volume_io.save_image(args.registered, image.like(registration.image))
    if args.deformation is not None:
        logger.info(f"Save displacement field to: {args.deformation}")
        registration.field.save(args.deformation)
    if args.jacobian is not None:
        logger.info(f"Save Jacobian determinant to: {args.jacobian}")
        det, _ = registration.jacobian(engine=inferer.engine)
        if args.jacobian.lower().endswith(".npy"):
            np.save(args.jacobian, det)
        else:
            volume_io.save_image(args.jacobian, image.like(det))
    if args.inverse_deformation is not None:
        logger.info(f"Save inverse displacement field to: {args.inverse_deformation}")
        registration.inverse_field.save(args.inverse_deformation)
    if args.labels_on_moving is not None:
        logger.info(f"Save labels on the moving grid to: {args.labels_on_moving}")
        if args.labels_on_moving.lower().endswith(".npy"):
            np.save(args.labels_on_moving, registration.labels_on_moving)
        else:
            volume_io.save_image(args.labels_on_moving, moving.like(registration.labels_on_moving))
    if pair is not None:
        for what, arr, dest in (("pair class map", pair.classes, args.pair_classes), ("pair density change map", pair.change, args.pair_change)):
            if dest is not None:
                logger.info(f"Save {what} to: {dest}")
                if dest.lower().endswith(".npy"):
                    np.save(dest, arr)
                else:
                    volume_io.save_image(dest, image.like(arr))
        if args.pair is not None:
            import json

            logger.info(f"Save paired analysis to: {args.pair}")
            with open(args.pair, "w") as f:
                json.dump(pair.analysis, f, indent=2)
    if args.registration is not None:
        import json

        logger.info(f"Save registration to: {args.registration}")
        with open(args.registration, "w") as f:
            json.dump(registration.meta(), f, indent=2)
    if clusters is not None:
        import json

        logger.info(f"Save cluster analysis to: {args.clusters}")
        with open(args.clusters, "w") as f:
            json.dump(clusters, f, indent=2)
    if cluster_ids is not None:
        logger.info(f"Save cluster ids to: {args.cluster_ids}")
        if args.cluster_ids.lower().endswith(".npy"):
            np.save(args.cluster_ids, cluster_ids)
        else:
            volume_io.save_image(args.cluster_ids, image.like(cluster_ids))
    if texture is not None:
        import json

        logger.info(f"Save texture features to: {args.texture}")
        with open(args.texture, "w") as f:
            json.dump(texture, f, indent=2)
    if stats is not None:
        import json

        logger.info(f"Save statistics to: {args.stats}")
        with open(args.stats, "w") as f:
            json.dump(stats, f, indent=2)
    if probs is not None:
        logger.info(f"Save probabilities to: {args.probabilities}")
        if args.probabilities.lower().endswith(".npy"):
            np.save(args.probabilities, probs)
        else:
            volume_io.write_nifti_channels(args.probabilities, image, probs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
