/* lungmask_hip.h -- C ABI of liblungmask_hip.so, the MI355X (gfx950) engine that
 * replaces the hot path of JoHof/lungmask: `LMInferer.apply()` ->
 * `LMInferer._inference()` (reference lungmask/mask.py:141-232) and everything
 * it calls in lungmask/resunet.py and lungmask/utils.py.
 *
 * The reference has no FFI seam (it is pure Python over torch/scipy/skimage);
 * the entry points below are what a ctypes binding inside the reference's
 * `mask.py` / `utils.py` would call -- one per reference call site, cited on
 * each declaration.  INTEGRATION.md shows that binding.
 *
 * Conventions
 *   - plain C: pointers + sizes only; no torch / numpy types.
 *   - every function returns 0 on success or a negative lm_status; the message
 *     is available from lm_last_error() (thread-local).
 *   - "dev" pointers are HBM addresses (hipMalloc / torch.cuda tensors /
 *     lm_dev_alloc); "host" pointers are ordinary memory.
 *   - an lm_engine owns one device, one HIP stream and its workspaces; it is not
 *     thread-safe, distinct engines are independent.
 *   - volumes are C-contiguous [n][h][w]; labels are uint8.
 *   - alignment of caller pointers: a device pointer needs the alignment of its ELEMENT type and no more (1 byte for u8
 *     labels, 2 for int16 / float16, 4 for float32 / int32, 8 for float64 / int64).  Views into a larger allocation -- one
 *     class map of a [C][n][h][w] stack, a slab of a volume, a slice of a torch tensor -- are therefore valid arguments of
 *     every entry point.  Kernels with a wide path (16-byte loads and stores, word-wise label reads) choose it per call
 *     from the pointer's low bits and the row length and fall back to element-wise access otherwise; the network reads
 *     its input and writes labels and log-probabilities element by element.  The result never depends on the placement:
 *     bit for bit the same at any base (tests/test_gpu_state.py).  Host pointers need the alignment of their C type.
 */
#ifndef LUNGMASK_HIP_H
#define LUNGMASK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lm_engine lm_engine;

typedef enum lm_status {
    LM_OK = 0,
    LM_ERR_INVALID = -1,  /* bad argument / shape / state            */
    LM_ERR_DEVICE = -2,   /* HIP runtime error (message has details) */
    LM_ERR_NOMODEL = -3,  /* model slot empty                        */
    LM_ERR_ALLOC = -4
} lm_status;

/* dtype codes for input volumes (numpy mode of mask.py:153-155 accepts any dtype); LM_F16 (IEEE binary16): output of the
 * probability maps only (lm_uncrop_probs_dev, lm_apply_probs_dev) */
enum { LM_I16 = 0, LM_I32 = 1, LM_F32 = 2, LM_F64 = 3, LM_U8 = 4, LM_U16 = 5, LM_I64 = 6, LM_F16 = 7 };

/* One named tensor of a torch state_dict (fp32, C-contiguous, host memory). */
typedef struct lm_tensor {
    const char* name; /* e.g. "down_path.0.block.0.weight" */
    const float* data;
    int64_t numel;
} lm_tensor;

/* ---- lifetime ---------------------------------------------------------------- */
const char* lm_last_error(void);
const char* lm_version(void);
/* 1 if the library was built for the GPU (always, for the shipped library). */
int lm_is_gpu_build(void);
/* mask.py:118-134 (device selection) -> explicit device ordinal. */
int lm_engine_create(lm_engine** out, int device_id);
void lm_engine_destroy(lm_engine* e);
int lm_engine_sync(lm_engine* e);

/* The HIP stream (hipStream_t, as void*) every stage call of this engine enqueues on.  A host that owns other GPU work or
 * collectives (lungmask_amd/pipeline.py: torch.distributed over RCCL) orders them against the engine's kernels by enqueuing on
 * / waiting for this stream instead of synchronising the device.  NULL for a NULL engine. */
void* lm_engine_stream(lm_engine* e);

/* ---- one rank per engine: RCCL communicator behind the C ABI --------------------------------------
 * The reference has no multi-GPU form; the slice-sharded pipeline (lungmask_amd/pipeline.py) needs exactly one
 * collective -- an equal-size all-gather of device buffers (label shards, slab-protocol planes/tables, the result) -- and with
 * these entry points it needs nothing else from the host's GPU stack.  RCCL is bound at run time (dlopen; torch's copy when
 * one is already mapped); a world of one initialised WITHOUT an id involves no library at all (its all-gather is a copy), with
 * an id it is a real RCCL communicator of one rank.
 *   rank 0: lm_dist_unique_id(id);  -> hand the 128 bytes to every rank by any side channel (a TCP store, a file, MPI)
 *   every rank: lm_dist_init(e, rank, world, id);   ...   lm_dist_all_gather(e, send, recv, bytes);   ...   lm_dist_destroy(e);
 * lm_dist_all_gather: recv_dev holds world * bytes, rank r's contribution at r * bytes (send_dev may be that very slot: in
 * place).  It is ENQUEUED on the engine's stream (lm_engine_stream): ordered after the engine's earlier kernels and before its
 * later ones, the host does not wait. */
#define LM_DIST_ID_BYTES 128
int lm_dist_unique_id(uint8_t* id_out /* [LM_DIST_ID_BYTES] */);
int lm_dist_init(lm_engine* e, int rank, int world, const uint8_t* id /* [LM_DIST_ID_BYTES]; NULL allowed when world == 1 */);
int lm_dist_rank(lm_engine* e);  /* < 0 without a communicator */
int lm_dist_world(lm_engine* e); /* < 0 without a communicator */
int lm_dist_all_gather(lm_engine* e, const void* send_dev, void* recv_dev, size_t bytes);
int lm_dist_destroy(lm_engine* e);

/* ---- device memory helpers (so a binding needs no other GPU runtime) ---------- */
int lm_dev_alloc(lm_engine* e, void** dev_ptr, size_t bytes);
int lm_dev_free(lm_engine* e, void* dev_ptr);
int lm_copy_h2d(lm_engine* e, void* dev_dst, const void* host_src, size_t bytes);
int lm_copy_d2h(lm_engine* e, void* host_dst, const void* dev_src, size_t bytes);
/* Page-locked host memory for volumes / label arrays that cross the boundary (lm_apply_host): the device copies straight into and
 * out of it at link speed, and a result block that is used again has no page faults to take.  The block belongs to the caller --
 * the engine keeps no record of it and lm_engine_destroy does not free it; lm_host_free accepts e == NULL. */
int lm_host_alloc(lm_engine* e, void** host_ptr, size_t bytes);
int lm_host_free(lm_engine* e, void* host_ptr);

/* ---- model (mask.py:38-68 get_model) ------------------------------------------ */
/* Loads a U-Net state_dict into `slot` (0..3).  n_classes is taken from
 * "last.bias" exactly as mask.py:56 does; the always-present-but-unused
 * residual_* tensors and num_batches_tracked are accepted and ignored. */
int lm_model_load(lm_engine* e, int slot, const lm_tensor* tensors, int n_tensors);
int lm_model_classes(lm_engine* e, int slot);

/* Arithmetic of the convolutions: 1 (default) = split-f16 3-product on v_mfma_f32_32x32x16_f16
 * (values carried as hi/lo f16 pairs, fp32 accumulate; ~2^-22 relative, i.e. fp32-class:
 * measured max |log-prob error| vs the reference <= 1.7e-4); 0 = exact fp32 matrix ops
 * (v_mfma_f32_32x32x2_f32, 16x lower peak). */
int lm_set_precision(lm_engine* e, int mode);
/* The arithmetic the NEXT forward of `slot` will use: 1 split-f16, 0 exact fp32.  The split form stores activations as
 * f16 pairs; its kernels watch the range (|v| >= 2^15 or non-finite), and a model that ever trips the guard is re-run --
 * in the same call -- and pinned to the exact-fp32 kernels (the reference computes in fp32, resunet.py:58-70, and has no
 * such range limit).  On the split-f16 kernels lm_forward_dev / lm_forward_batches_dev / lm_apply_* therefore return only after
 * the forward has finished (the flag is read back).  On the exact-fp32 kernels -- lm_set_precision(e, 0), or a model the range
 * guard or the accuracy guard has pinned -- there is no flag to read: lm_forward_dev and lm_forward_batches_dev only ENQUEUE
 * (both lanes joined into the engine's stream), and so do lm_apply_dev / lm_apply_probs_dev / lm_pipe_apply without volume
 * post-processing and fill model.  Their results are ordered on the engine's stream like those of every other enqueue-only entry
 * point; the host waits with lm_engine_sync, a blocking copy or lm_pipe_wait. */
int lm_model_precision(lm_engine* e, int slot);
/* Accuracy guard.  lm_model_load on a split-f16 engine (and lm_set_precision(e, 1) for models loaded before it) runs TWO deterministic
 * probe slices (256 x 256: a phantom-like image and uniform noise, both in the network's [0, 1] input range) through the split-f16 and the exact-fp32 kernels of the
 * model and pins it to the exact-fp32 kernels -- with a notice on stderr -- when max |delta log-prob| exceeds the limit (environment
 * LM_ACC_GUARD, default 5e-4: half of the 1e-3 of the reference's fp32 result the engine is held to; "0" disables the probe).  A
 * checkpoint with a logit range or weight tails beyond what the split arithmetic resolves therefore cannot silently sit outside the
 * tolerance.  Between the two there are middle tiers: a model above the limit is probed again with the 3x3 convs split along K so that
 * no fp32 accumulator chain runs over more than 4608, then 2304, then 1152 products (the chain's roundings are where the split
 * arithmetic's error comes from; parts are work items of their own, added in a fixed order; +1 % / +4 % / +12 % forward time instead
 * of the exact kernels' 4x) and runs on the first form that is within the limit (lm_model_precision still says 1: split-f16;
 * lm_model_chain_limit says which).
 * *err_out = max |delta log-prob| of the probe of the form the model runs on (< 0: no probe was run -- guard off, or the f16 range
 * guard tripped on the probe and pinned the model first); returns 0 fast split-f16 form, 2 a split-K form, 1 pinned to the
 * exact-fp32 kernels by the probe, < 0 on error.  LM_H3_KSPLIT_K=<products> puts every model on that split-K form (A/B and test hook). */
int lm_model_probe_error(lm_engine* e, int slot, float* err_out);
/* products per accumulator chain of the model's 3x3 convs: 0 = not split (the fast form), else the limit the accuracy guard chose. */
int lm_model_chain_limit(lm_engine* e, int slot);

/* ---- network forward (mask.py:178-186: model(mbt) + torch.max(pred,1)[1]) ------ */
/* x_dev: f32 [b][h][w] (h, w multiples of 16).  labels_dev: u8 [b][h][w] or NULL.
 * logp_dev: f32 [b][C][h][w] log-softmax exactly like UNet.forward's return
 * (resunet.py:70), or NULL. */
int lm_forward_dev(lm_engine* e, int slot, const float* x_dev, int b, int h, int w,
                   uint8_t* labels_dev, float* logp_dev);

/* ---- pre-processing (utils.py:32-111 preprocess / simple_bodymask / crop_and_resize,
 *      mask.py:166-168 clip + (x+1024)/1624) -------------------------------------- */
/* vol_dev: [n][h][w] of `dtype` (LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64).  Outputs (all dev):
 *   bbox_dev   int32 [n][4]  body bounding box (r0,c0,r1,c1), utils.py:102-106
 *   x_f32_dev  f32 [n][oh][ow] normalised network input        (or NULL)
 *   x_i16_dev  i16 [n][oh][ow] == utils.preprocess()[0]        (or NULL; integer volumes only)
 *   bmask_dev  u8  [n][h][w]   == utils.simple_bodymask(slice) (or NULL; test seam) */
int lm_preprocess_dev(lm_engine* e, const void* vol_dev, int dtype, int n, int h, int w, int oh, int ow,
                      int32_t* bbox_dev, float* x_f32_dev, int16_t* x_i16_dev, uint8_t* bmask_dev);

/* ---- mask un-crop (utils.py:114-129 reshape_mask, mask.py:196-202) --------------- */
/* mask_dev u8 [n][mh][mw], bbox_dev int32 [n][4] -> out_dev u8 [n][h][w]. */
int lm_reshape_mask_dev(lm_engine* e, const uint8_t* mask_dev, const int32_t* bbox_dev, int n, int mh, int mw,
                        int h, int w, uint8_t* out_dev);

/* ---- probability maps un-cropped to the input volume (not in the reference: its LMInferer returns labels only) ------------------
 * The raw network probabilities, resampled back into each slice's body box -- reshape_mask's recipe (utils.py:114-129) with linear
 * instead of nearest-neighbour interpolation.  For slice z, class c, bbox[z] = (r0, c0, r1, c1):
 *     p = exp(logp[z][c])                                           f32 [mh][mw], logp = the forward's log-softmax
 *     out[c][z][r0:r1, c0:c1] = scipy.ndimage.zoom(p, ((r1-r0)/mh, (c1-c0)/mw), order=1)   fp64 arithmetic, one rounding to f32
 *     out[c][z][elsewhere]     = c == 0 ? 1 : 0                     reshape_mask's zero fill = label 0 = background
 * Where ndimage.zoom's coordinate lands beyond the last source row / column (the rounding of o * (in-1)/(out-1) for some box sizes;
 * scipy then returns its cval 0 in every class, and reshape_mask label 0) the fill is written as well.  The maps therefore sum to
 * one everywhere (linear interpolation is a convex combination).  LM_F16 output is (half)(float)v, round to nearest even.
 * logp_dev f32 [n][C][mh][mw] (1 <= mw <= 256), bbox_dev int32 [n][4] -> out_dev [C][n][h][w] of out_dtype (LM_F32 or LM_F16):
 * class-major, each class map a contiguous volume shaped like the input.  Test seam and building block. */
int lm_uncrop_probs_dev(lm_engine* e, const float* logp_dev, const int32_t* bbox_dev, int n, int C, int mh, int mw,
                        int h, int w, int out_dtype, void* out_dev);

/* ---- orientation (mask.py:156-164/* ---- orientation (mask.py:156-164 sitk.DICOMOrient(image, "LPS") and its undo at :204-208) ---- */
/* Axis permutation / flip as an index transform: out[i0][i1][i2] = in[base + i0*s0 + i1*s1 + i2*s2]
 * (strides and base in ELEMENTS of elem_size = 1|2|4|8 bytes; strides may be negative; in/out must not
 * overlap).  The host side derives (s, base) from the image direction cosines (lungmask_amd/volume_io.py). */
int lm_reorient_dev(lm_engine* e, const void* in_dev, void* out_dev, int elem_size, int n0, int n1, int n2,
                    int64_t s0, int64_t s1, int64_t s2, int64_t base);

/* ---- volume post-processing (utils.py:272-358 postprocessing incl. :361-404 bbox_3D /
 *      keep_largest_connected_component and the hole filler of :344-352) -------------- */
/* lab_dev u8 [n][h][w], processed IN PLACE.  spare: label values that are merged into
 * neighbours and dropped (fusion), may be NULL; skip_below: utils.py default 3. */
int lm_postprocess_dev(lm_engine* e, uint8_t* lab_dev, int n, int h, int w, const int* spare, int n_spare,
                       int skip_below);
/* ---- the two helpers of postprocessing as seams of their own (utils.py:361-387 bbox_3D, :390-404
 *      keep_largest_connected_component; the reference's tests call bbox_3D directly, tests/test_utils.py:58-63) ---- */
/* mask_dev u8 [n][h][w] (non-zero = set).  bbox_out (HOST, 6 ints) = [zmin, zmax, ymin, ymax, xmin, xmax]: first / last set index
 * per axis, grown by `margin`, clipped to the volume, maxima exclusive (utils.py:376-383).  A mask without a set voxel has no
 * box -- the reference raises IndexError at utils.py:377 -- and all six come back as -1.  Returns after the result is known. */
int lm_bbox3d_dev(lm_engine* e, const uint8_t* mask_dev, int n, int h, int w, int margin, int32_t bbox_out[6]);
/* mask_dev u8 [n][h][w], IN PLACE -> 1 on the voxels of the largest region of skimage.measure.label(mask) (full connectivity:
 * 26 neighbours, 8 when n == 1; voxels of different non-zero values are different regions), 0 elsewhere.  Equal areas: the
 * region whose first voxel (raster order) comes last -- what `np.argsort(resizes)[-1]` of utils.py:402 yields while numpy's sort
 * is its stable insertion sort (<= 16 regions); beyond that the reference itself leaves the tie to numpy's quicksort.
 * *area_out (HOST, may be NULL) = that region's voxel count; 0 = no region at all (the reference raises IndexError at
 * utils.py:402), mask unchanged. */
int lm_keep_largest_dev(lm_engine* e, uint8_t* mask_dev, int n, int h, int w, int64_t* area_out);

/* ---- per-label volume and density statistics (not in the reference: what users compute from a lung / lobe mask) -------------------
 * lab u8 [n][h][w] and vol [n][h][w] of `dtype` (LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64: what apply takes).
 *   HU value of a voxel: integer volumes hu = v; float volumes hu = rint(v) (round half to even), saturated to the int32 range.
 *     NaN is counted in `nonfinite` and left out of every density figure; +-inf saturate like any other value.
 *   Histogram: clip(hu, -1024, 3071) goes into a 4096-bin histogram with 1-HU bins (bin = clipped + 1024), one per label;
 *     clipped_low / clipped_high count the values that were clipped.  Mean, std, percentiles and "below" fractions all use the
 *     clipped values, so every one of them follows from the histogram.  hu_min / hu_max use the unclipped hu (0 when the label
 *     has no finite voxel).
 *   Accumulators of labels 1 .. n_labels-1: voxels, nonfinite, clipped_low, clipped_high, hu_min, hu_max, index_sum = (sum z,
 *     sum y, sum x), bbox = zmin, zmax, ymin, ymax, xmin, xmax with the maxima exclusive (bbox_3D with margin 0; all six -1 when
 *     the label has no voxel).  Label 0 (background) gets `voxels` only (the other fields 0, bbox -1).
 *   *other_out = the number of voxels whose label is >= n_labels.
 * stats_host [n_labels]; hist_host [n_labels][4096] int64 or NULL (row 0 stays 0).  1 <= n_labels <= 16; n * h * w < 2^31
 * (u32 bins per workgroup, 32-bit voxel indices).  Runs on the engine's stream and returns once the result is on the host. */
typedef struct lm_label_stats {
    int64_t voxels, nonfinite, clipped_low, clipped_high, hu_min, hu_max, index_sum[3];
    int32_t bbox[6];
} lm_label_stats;
int lm_label_stats_dev(lm_engine* e, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h, int w, int n_labels,
                       lm_label_stats* stats_host, int64_t* hist_host, int64_t* other_out);

/* ---- per-label texture matrices (not in the reference: the GLCM and GLRLM a radiomics tool derives its texture features from) ------
 * lab u8 [n][h][w] and vol [n][h][w] of `dtype` (LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64), as for lm_label_stats_dev.  The device
 * produces integer matrices only; every feature follows from them on the host (lungmask_amd/texture.py).
 *   HU value of a voxel: exactly lm_label_stats_dev's -- integer volumes hu = v; float volumes hu = rint(v) (round half to even),
 *     saturated to the int32 range; NaN is counted in `nonfinite` and left out.
 *   Re-segmentation and discretisation (params lo, hi, bin_width; all arithmetic in int64): a voxel of label k is VALID when it is
 *     finite and lo <= hu <= hi.  A voxel outside that range is excluded, not clipped (IBSI re-segmentation), and counted in `below`
 *     or `above`.  The grey level of a valid voxel is g = (hu - lo) / bin_width (integer division, 0-based);
 *     Ng = (hi - lo) / bin_width + 1 levels, 1 <= Ng <= 64, bin_width >= 1, lo <= hi.
 *   Directions: the 13 offsets (dz, dy, dx) of {-1, 0, 1}^3, in the array's axis order, whose first non-zero component is +1, in
 *     ascending lexicographic order: 0 (0,0,1)  1 (0,1,-1)  2 (0,1,0)  3 (0,1,1)  4 (1,-1,-1)  5 (1,-1,0)  6 (1,-1,1)  7 (1,0,-1)
 *     8 (1,0,0)  9 (1,0,1)  10 (1,1,-1)  11 (1,1,0)  12 (1,1,1).  Neighbours are taken in index space: the spacing is never seen
 *     (resample an anisotropic volume first, lm_roi_dev).
 *   GLCM: glcm[k][d][i][j] = the number of voxels p such that p and q = p + distance * dir_d both lie inside the volume, both are
 *     valid voxels of label k, g(p) = i and g(q) = j.  Ordered pairs, not symmetrised (the host uses P + P^T).  1 <= distance <= 8.
 *   GLRLM (always adjacent voxels): a run of label k along direction d is a maximal set of consecutive voxels p, p + dir, p + 2 dir,
 *     ... that are all valid, all of label k and all of one grey level -- the voxel before the first and the voxel after the last are
 *     outside the volume, not valid, of another label or of another level.  glrlm[k][d][i][min(r, nr) - 1] counts the runs of level i
 *     and length r: the last of the caller's nr columns (1 <= nr <= 8192) absorbs every longer run, and counts[k].longest_run, the
 *     longest run of label k over all directions (0: none), tells whether it did.
 *   counts[k] for k in 1 .. n_labels-1: voxels, valid, nonfinite, below, above (voxels = the sum of the other four), longest_run.
 *   Label 0 and labels >= n_labels take no part: row 0 of counts and of both matrices is zero.
 * params, counts_host [n_labels] and glcm_host [n_labels][13][Ng][Ng] int64 are required; glrlm_host [n_labels][13][Ng][nr] int64 or
 * NULL (longest_run is still reported).  1 <= n_labels <= 16; every dimension <= 4096 and n * h * w < 2^31.  Anything else returns
 * LM_ERR_INVALID with a message before the device is touched.  All counting is integer: the result does not depend on the schedule.
 * Runs on the engine's stream and returns once the result is on the host. */
typedef struct lm_texture_params {
    int32_t lo, hi, bin_width, distance, nr;
} lm_texture_params;
typedef struct lm_texture_counts {
    int64_t voxels, valid, nonfinite, below, above, longest_run;
} lm_texture_counts;
int lm_texture_dev(lm_engine* e, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h, int w, int n_labels,
                   const lm_texture_params* params, lm_texture_counts* counts_host, int64_t* glcm_host, int64_t* glrlm_host);

/* ---- label agreement metrics (not in the reference: Dice, Hausdorff and surface distances between two label volumes) ---------------
 * lm_edt_dev: the exact squared Euclidean distance transform.  feat u8 [n][h][w], spacing[3] doubles in the array's axis order
 * (z, y, x; NULL = 1, 1, 1) -> d2 f32 [n][h][w] = the squared distance of every voxel to the nearest voxel with feat != 0, DEFINED
 * in float32 (fl = one rounding to float32, no fused multiply-add):
 *     w_i          = (float)(spacing_i * spacing_i)                                 the product in double
 *     g1[z][y][x]  = min over x' with feat[z][y][x'] != 0 of w_x * (float)((x-x')^2)   +inf for a row without such a voxel
 *     g2[z][y][x]  = min over y' of fl(g1[z][y'][x] + fl(w_y * (float)((y-y')^2)))
 *     d2[z][y][x]  = min over z' of fl(g2[z'][y][x] + fl(w_z * (float)((z-z')^2)))
 * Float rounding is monotone, so this equals the minimum over all feature voxels of fl(fl(fl(w_x dx^2) + fl(w_y dy^2)) + fl(w_z
 * dz^2)): the value does not depend on the algorithm, and stays within 3e-7 relative of the float64 transform.  A volume without a
 * feature gives +inf everywhere.  Every dimension <= 4096 (dx^2 exact in float32) and n * h * w < 2^31, refused before anything is
 * read.  Works in place in d2_out_dev (no workspace); enqueued on the engine's stream.
 *
 * lm_label_agreement_dev: a, b u8 [n][h][w].  out_rows (HOST) [n_labels]: row k in 1 .. n_labels-1 compares A = (a == k) with
 * B = (b == k); row 0 ("lung") compares (a >= 1) with (b >= 1), whatever the label values.
 *   voxels_a, voxels_b, intersection: |A|, |B|, |A and B|.  bbox: box of A or B, zmin, zmax, ymin, ymax, xmin, xmax with exclusive
 *     maxima (bbox_3D with margin 0; all -1 when both are empty).
 *   Surface voxel of A: a voxel of A with at least one of its 6 face neighbours not in A or outside the volume (== A ^
 *     binary_erosion(A, generate_binary_structure(3, 1)) with border_value 0).  surface_a, surface_b count them.
 *   a -> b: the values of lm_edt_dev(features = surface of B, spacing) at the surface voxels of A; b -> a the other way round.  The
 *     transforms run inside bbox, which holds every surface voxel of both, so the values are those of the whole volume.
 *     max_d2_ab / max_d2_ba: the largest value (exact).  sum_d_ab / sum_d_ba: the sum of sqrt((double)d2), in a fixed order.
 *     order_ab / order_ba / order_pooled [q][0 .. 1]: for percentiles[q], the order statistics of the a -> b list, the b -> a list
 *     and the two lists together at ranks floor and ceil of percentiles[q] / 100 * (count - 1) (numpy's method="linear" neighbours).
 *     When either surface is empty no distance exists: max_d2 and the order statistics are -1, the sums 0.
 *   other_a, other_b (row 0 only): voxels of a / b with a label >= n_labels (they count for row 0 and for no other row).
 * 1 <= n_labels <= 16; at most 8 percentiles in [0, 100]; spacing as above; limits as lm_edt_dev.  Everything but the two sums is
 * independent of the schedule.  Workspace (grow-only, kept by the engine): two u8 surface volumes of the input's size and two
 * float32 volumes of the size of row 0's box; the distance lists are never materialised.  Returns once the result is on the host. */
int lm_edt_dev(lm_engine* e, const uint8_t* feat_dev, int n, int h, int w, const double* spacing, float* d2_out_dev);
typedef struct lm_label_agreement {
    int64_t voxels_a, voxels_b, intersection, surface_a, surface_b, other_a, other_b;
    double sum_d_ab, sum_d_ba;
    float max_d2_ab, max_d2_ba;
    float order_ab[8][2], order_ba[8][2], order_pooled[8][2];
    int32_t bbox[6];
} lm_label_agreement;
int lm_label_agreement_dev(lm_engine* e, const uint8_t* a_dev, const uint8_t* b_dev, int n, int h, int w, int n_labels,
                           const double* spacing, const double* percentiles, int n_percentiles, lm_label_agreement* out_rows);

/* ---- lung ROI: the masked, cropped, resampled volume (not in the reference: what callers cut out of the CT with the mask) -----------
 * vol [n][h][w] of `dtype` (LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64) and lab u8 [n][h][w] -> out_image [N_0][N_1][N_2] of
 * p->out_dtype and out_labels u8 [N_0][N_1][N_2].  The HOST fixes the grid (p->bbox, p->out_dims, p->step); the device never
 * derives it, so both sides agree by construction.  DEFINITION, with s_i the source spacing and t_i the output spacing of axis i
 * (array axis order z, y, x), all arithmetic in float64 without fused multiply-add:
 *   1. Box.  bbox_3D with margin 0 of the voxels with keep[lab] != 0 (lm_roi_plan_dev; no such voxel: LM_ERR_INVALID, "no kept
 *      voxel"), grown per axis by m_i = ceil(margin_mm / s_i) voxels (margin_mm voxels without a spacing) and clipped to the volume:
 *      bbox = zmin, zmax, ymin, ymax, xmin, xmax with exclusive maxima, extents e_i.  (The margins are the caller's: lungmask_amd/roi.py.)
 *   2. Grid.  step_i = t_i / s_i;  N_i = floor((e_i - 1) / step_i) + 1;  output index o samples the source coordinate
 *      c_i(o) = min((double)o * step_i, (double)(e_i - 1)), relative to the box start.  lm_roi_dev refuses out_dims that differ.
 *   3. Intensity.  Trilinear: i0 = floor(c), f = c - i0, i1 = min(i0 + 1, e - 1); lerp(a, b, f) = a * (1 - f) + b * f, applied
 *      along x, then y, then z, on the source values converted to double.  One rounding at the very end (7.).
 *   4. Labels.  Nearest neighbour: j_i = min((int)floor(c_i + 0.5), e_i - 1); out_labels[o] = lab[box + j], the raw value.
 *   5. Inside.  dilate_mm == 0: keep[out_labels[o]] != 0.  dilate_mm > 0: d2[box + j] <= (float)(dilate_mm * dilate_mm), d2 =
 *      lm_edt_dev's float32 squared distance (p->spacing) to the voxels with keep[lab] != 0.  Every feature lies inside the box, so
 *      the transform runs on the box only: its values there are those of the whole volume.
 *   6. Mask and window.  With LM_ROI_MASK_OUTSIDE a voxel that is not inside takes p->fill.  Then, with LM_ROI_WINDOW (hi > lo):
 *      v = (v < lo ? lo : v > hi ? hi : v), followed by (v - lo) / (hi - lo).
 *   7. Output.  LM_F32: (float)v.  LM_F16: (half)(float)v, i.e. the float32 result's astype(float16), bit for bit.  LM_I16:
 *      rint(v), half to even, saturated to [-32768, 32767]; integer volumes without a window only (refused otherwise).
 *   NaN and inf of float volumes follow from the formulas (inf * 0 = NaN in a lerp; NaN passes the window's comparisons unchanged);
 *   which NaN comes out (sign, payload) is not defined.
 *   With every step equal to 1 the formulas return the source value of a finite input (a pure crop; -0.0 comes out as +0.0).
 * Limits are lm_edt_dev's: n, h, w <= 4096 and n * h * w < 2^31, also for the output's voxel count; refused before anything is read.
 * Workspace (grow-only, kept by the engine, with dilate_mm > 0 only): one u8 and one float32 volume of the box's size.  Enqueued on
 * the engine's stream; p is read before the call returns.
 *
 * lm_roi_plan_dev: bbox_out (HOST) = the margin-0 box of step 1 (lm_bbox3d_dev's kernel; for a keep table other than "every label
 * >= 1" on the u8 volume keep[lab]).  Returns once the box is known. */
#define LM_ROI_MASK_OUTSIDE 1u
#define LM_ROI_WINDOW 2u
typedef struct lm_roi_params {
    int32_t bbox[6];     /* zmin, zmax, ymin, ymax, xmin, xmax in source indices, maxima exclusive */
    int32_t out_dims[3]; /* N_0, N_1, N_2 */
    double step[3];      /* source voxels per output voxel */
    uint8_t keep[256];   /* keep[label] != 0: the label belongs to the ROI */
    double dilate_mm;    /* >= 0 */
    double spacing[3];   /* source spacing (array axis order), the metric of dilate_mm; 1, 1, 1 = voxels */
    double fill;
    double window_lo, window_hi;
    uint32_t flags;      /* LM_ROI_MASK_OUTSIDE | LM_ROI_WINDOW */
    int32_t out_dtype;   /* LM_F32, LM_F16 or LM_I16 */
} lm_roi_params;
int lm_roi_plan_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], int32_t bbox_out[6]);
int lm_roi_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev, int n, int h, int w, const lm_roi_params* p,
               void* out_image_dev, uint8_t* out_labels_dev);

/* ---- resampling onto any grid (not in the reference: what callers leave the device for SimpleITK.Resample for) ----------------------
 * src [n][h][w] of `dtype` (LM_I16, LM_I32, LM_I64, LM_F32, LM_F64, or LM_U8 for labels) -> out [N_0][N_1][N_2] of p->out_dtype, the
 * source sampled at an affine map of the output index.  The HOST fixes the map (p->A, p->b; lungmask_amd/resample.py: index_map); the
 * device never derives it.  DEFINITION, array axis order z, y, x, e_i the source extents, all arithmetic in float64 without fused
 * multiply-add and in the order written:
 *   1. Coordinate.  For the output index o:  c_i = ((A[3i] * o_0 + A[3i+1] * o_1) + A[3i+2] * o_2) + b_i.
 *   2. Domain.  t_i = floor(c_i + 0.5); the voxel is INSIDE iff 0 <= t_i < e_i on all three axes (ITK's buffer test: c_i in
 *      [-0.5, e_i - 0.5); a NaN coordinate is outside), and j_i = (int)t_i.  An outside voxel takes p->fill, converted as in 7.
 *      (LM_RS_NEAREST: to the source's dtype -- integers rint, half to even, saturated; LM_U8 outputs take (uint8_t)fill, and fill
 *      must lie in [0, 255]).  For the interpolating modes the coordinate is then clamped: c_i = min(max(c_i, 0), e_i - 1).
 *   3. LM_RS_NEAREST.  out[o] = src[j], the raw value; out_dtype must equal dtype.
 *   4. LM_RS_LINEAR.  lm_roi_dev's trilinear (3. there) on the clamped coordinate: i0 = floor(c), f = c - i0, i1 = min(i0 + 1, e - 1),
 *      lerp(a, b, f) = a * (1 - f) + b * f along x, then y, then z, on the source values converted to double.
 *   5. LM_RS_CUBIC.  Cubic B-spline interpolation with mirror boundaries (the edge sample not repeated: period P = 2e - 2, index
 *      m(k) = k mod P, and P - that where it is >= e; e = 1: always 0).
 *      Prefilter (lm_spline_prefilter_dev), per axis x, then y, then z, on the volume converted to double, along every line s[0 .. e-1]
 *      of the axis; an axis of extent 1 is skipped.  With z = sqrt(3.0) - 2.0:
 *        cp[0] = sum over k = 0 .. 36 of zk * s[m(k)], accumulated from 0.0 in ascending k, zk = 1.0 first and zk = zk * z after each term
 *        cp[i] = s[i] + z * cp[i-1]                                   (i = 1 .. e-1)
 *        c[e-1] = (z / (z * z - 1.0)) * (cp[e-1] + z * cp[e-2])
 *        c[i]  = z * (c[i+1] - cp[i])                                 (i = e-2 .. 0)
 *        the line becomes 6.0 * c[i].
 *      Sample, on the clamped coordinate: i0 = floor(c), f = c - i0, g = 1.0 - f; taps m(i0 - 1), m(i0), m(i0 + 1), m(i0 + 2) with the
 *      weights  w0 = ((g * g) * g) / 6.0,  w1 = 2.0 / 3.0 - ((f * f) * (2.0 - f)) / 2.0,  w2 = 2.0 / 3.0 - ((g * g) * (1.0 + f)) / 2.0,
 *      w3 = ((f * f) * f) / 6.0.  vx = 0.0, then vx = vx + wx_k * coef in tap order along x; vy = 0.0, vy = vy + wy_k * vx_k along y; the
 *      same along z.  The overshoot of the spline is not clamped.
 *   6. LM_RS_LABEL_LINEAR (LM_U8 in and out).  The per-label trilinear indicator and an argmax, without a map per label: the eight
 *      corners (i0 or i1 per axis, taps of 4.) in z-major order (z0 y0 x0, z0 y0 x1, z0 y1 x0, ...), each with the weight
 *      (wz * wy) * wx, w = 1 - f for i0 and f for i1.  The weights are summed per distinct label value in corner order; the result is
 *      the label with the largest sum, the smaller label value on a tie.  On a map that translates by whole voxels it equals nearest.
 *   7. Output of 4. and 5.: lm_roi_dev's three rules.  LM_F32: (float)v.  LM_F16: the float32 result's astype(float16).  LM_I16:
 *      rint(v), half to even, saturated; integer sources only (refused otherwise).
 *   NaN and inf of float sources follow from the formulas; which NaN comes out is not defined.
 * Limits: every dimension <= 4096 and fewer than 2^31 voxels, for the source and for the output; refused before anything is read.
 * Workspace (grow-only, kept by the engine, LM_RS_CUBIC only): one float64 volume of the source's size.  Enqueued on the engine's
 * stream; p is read before the call returns.
 *
 * lm_spline_prefilter_dev: coef_out_dev [n][h][w] float64 = the prefilter of 5. alone (no workspace). */
enum { LM_RS_NEAREST = 0, LM_RS_LINEAR = 1, LM_RS_CUBIC = 2, LM_RS_LABEL_LINEAR = 3 };
typedef struct lm_resample_params {
    int32_t out_dims[3]; /* N_0, N_1, N_2 */
    int32_t mode;        /* LM_RS_* */
    double A[9];         /* row-major: source index = A * output index + b */
    double b[3];
    double fill;
    int32_t out_dtype;   /* LM_F32, LM_F16 or LM_I16; the source's dtype for LM_RS_NEAREST; LM_U8 for LM_RS_LABEL_LINEAR */
} lm_resample_params;
int lm_spline_prefilter_dev(lm_engine* e, const void* vol_dev, int dtype, int n, int h, int w, double* coef_out_dev);
int lm_resample_dev(lm_engine* e, const void* src_dev, int dtype, int n, int h, int w, const lm_resample_params* p, void* out_dev);

/* ---- joint histogram of two volumes under an affine map (not in the reference: the cost function of a mutual-information registration) ----
 * fixed [fn][fh][fw] of fdtype and moving [mn][mh][mw] of mdtype (each LM_U8, LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64) -> hist_out
 * int64 [bins][bins] (row: the fixed bin) and counts_out int64 [4].  Neither volume moves and no resampled volume is written.  The HOST
 * fixes the map (lungmask_amd/resample.py: index_map(moving_grid, fixed_grid, transform)).  DEFINITION, array axis order z, y, x, e_i
 * the MOVING extents, all floating-point arithmetic in float64 without fused multiply-add and in the order written, Q = 65536:
 *   1. Lattice.  The sampled fixed voxels are o_i = start_i + k * step_i, k >= 0, o_i < (fixed extent)_i.  With fixed_lab_dev (u8, the
 *      fixed volume's shape) only the voxels with keep[label] != 0 are sampled.  counts[0] = the number of sampled voxels.
 *   2. Fixed value.  The HU rule of lm_label_stats_dev: integers as they are (int64 saturated to int32), floats rint (half to even)
 *      saturated to int32.  A NaN: the sample counts in counts[3] and contributes nothing.
 *      i = (clamp(hu, f_lo, f_lo + bins * f_width - 1) - f_lo) / f_width.
 *   3. Coordinate and domain.  1. and 2. of lm_resample_dev with the fixed index as o and the moving volume as the source: c_i, the
 *      buffer test on t_i = floor(c_i + 0.5) (a NaN coordinate is outside), j_i = (int)t_i.  An outside sample counts in counts[2] and
 *      contributes nothing.  The coordinate is then clamped to [0, e_i - 1].
 *   4. LM_JH_LINEAR.  v = the trilinear value of lm_resample_dev (4. there) of the moving values converted to double.  A NaN v: the
 *      sample counts in counts[3] and contributes nothing.  u = min(max((v - m_lo) / m_width, 0.0), bins - 1.0), k0 = floor(u),
 *      k1 = min(k0 + 1, bins - 1), g = u - k0, q1 = (int64)floor(g * Q + 0.5), q0 = Q - q1;  hist[i][k0] += q0, hist[i][k1] += q1.
 *      The bin centres of the moving axis sit at m_lo + k * m_width: integer data with width 1 lands in exactly one bin.
 *   5. LM_JH_NEAREST.  The moving value is src[j], the raw voxel of the domain test, through the HU rule (NaN as in 2.) and binned as
 *      in 2. with m_lo and m_width;  hist[i][k] += Q.  The form for two label volumes: LM_U8, lo = 0, width = 1.
 *   6. counts[1] = the number of samples that contributed: sum(hist) == Q * counts[1], counts[0] == counts[1] + counts[2] + counts[3].
 * Limits: every dimension in 1 .. 4096 and fewer than 2^31 voxels per volume (a bin stays below 2^47), 2 <= bins <= 64, widths >= 1,
 * step_i >= 1, start_i >= 0; refused before anything is read.  Both outputs are fully written: the caller zeroes nothing.
 * Workspace (grow-only, kept by the engine): at most 1024 * (bins^2 + 4) int64.  Enqueued on the engine's stream; p is read before the
 * call returns. */
enum { LM_JH_LINEAR = 0, LM_JH_NEAREST = 1 };
typedef struct lm_joint_hist_params {
    double A[9], b[3];         /* row-major: moving index = A * fixed index + b */
    int32_t start[3], step[3]; /* the sampled fixed indices */
    int32_t bins;              /* 2 .. 64, the same on both axes */
    int32_t mode;              /* LM_JH_* */
    int32_t f_lo, f_width;     /* fixed axis: lowest HU and HU per bin (>= 1) */
    int32_t m_lo, m_width;     /* moving axis */
    uint8_t keep[256];         /* with labels: the label values that are sampled */
} lm_joint_hist_params;
int lm_joint_hist_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* fixed_lab_dev,
                      const void* moving_dev, int mdtype, int mn, int mh, int mw, const lm_joint_hist_params* p, int64_t* hist_out_dev,
                      int64_t* counts_out_dev);

/* ---- deformable registration: warping through a displacement field, a demons step, the Jacobian determinant (not in the reference:
 *      what callers leave the device for elastix or ANTs for) --------------------------------------------------------------------------
 * A DISPLACEMENT FIELD is float32 [3][n][h][w] on the FIXED (output) grid; component i is the displacement along the grid's array axis
 * i (z, y, x), in millimetres with a spacing and in voxels without.  The device gets field_scale[i] = 1 / spacing_i (1.0 without a
 * spacing; float64, fixed by the host) and never sees a spacing.  COORDINATE RULE, all in float64 without fused multiply-add and in the
 * order written, o the output (fixed) index, u_i[o] the field:
 *     p_i = (double)o_i + (double)u_i[o] * field_scale[i]                       (p_i = (double)o_i with a NULL field)
 *     c_i = ((A[3i] * p_0 + A[3i+1] * p_1) + A[3i+2] * p_2) + b_i
 * with A, b the map of lm_resample_dev (resample.py: index_map(moving grid, fixed grid, affine)).  A field of zeros gives p = o
 * exactly, so every call below then equals its counterpart without a field bit for bit.  From c on -- the inside test on
 * t_i = floor(c_i + 0.5), the clamp to [0, e_i - 1], the taps -- everything is lm_resample_dev's 2. to 7.; a NaN coordinate, and so a
 * NaN in the field, is outside.
 *
 * lm_warp_dev: src [n][h][w] of `dtype`, field_dev float32 [3][N_0][N_1][N_2] or NULL -> out [N_0][N_1][N_2] of p->out_dtype.
 * DEFINITION: lm_resample_dev with the coordinate rule above in place of its 1.; modes, fills and output dtypes are lm_resample_dev's.
 * For LM_RS_CUBIC the caller passes the float64 coefficient volume of lm_spline_prefilter_dev as src (dtype must be LM_F64: anything
 * else is refused, a source that was not prefiltered cannot be told apart and gives a smoothed image), so the call needs no
 * workspace; out_dtype LM_F32, LM_F16 or LM_I16 (the caller knows whether the coefficients came from integers).  field_scale must be
 * finite.  out_dev must be neither src_dev nor field_dev.
 *
 * lm_demons_step_dev: ONE additive demons iteration with Thirion's force from the fixed image's gradient, without a warped volume.
 * fixed [fn][fh][fw] of fdtype and moving [mn][mh][mw] of mdtype (each LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64), optionally
 * fixed_lab_dev u8 [fn][fh][fw], the current field u_dev float32 [3][fn][fh][fw] -> out_dev float32 [3][fn][fh][fw] (NOT u_dev:
 * in-place is refused) and counts_out_dev int64 [5].  DEFINITION, per fixed voxel o, F the fixed volume converted to double:
 *   1. Selection.  Selected iff fixed_lab_dev is NULL or keep[label] != 0.  Not selected: out_j = u_j.  Selected: counts[0]++.
 *   2. Fixed value.  f = F[o].  A NaN: counts[3]++ and out_j = u_j.
 *   3. Coordinate.  The rule above with e_i the MOVING extents.  Outside: counts[2]++ and out_j = u_j.
 *   4. Moving value.  m = the trilinear value of lm_resample_dev (4. there) on the clamped coordinate.  A NaN: as in 2.
 *   5. Gradient.  g_j = (F[o + e_j] - F[o - e_j]) * grad_scale[j], the neighbour indices CLAMPED to the volume (the host passes
 *      grad_scale[j] = field_scale[j] / 2: millimetre^-1 central differences).  At a border the clamped difference spans one voxel and
 *      is divided by two: HALF of the one-sided slope there -- a damped force in the outermost layer, not special-cased.  An axis of
 *      extent 1 gives g_j = 0.0.  A NaN g_j: as in 2.
 *   6. d = f - m;  den = ((g_0 * g_0 + g_1 * g_1) + g_2 * g_2) + (d * d) * inv_k2.
 *      step_j = den < den_min ? 0.0 : (d * g_j) / den;   out_j = (float)((double)u_j + step_j).
 *   7. counts[1]++ and counts[4] += (int64)floor(min(d * d, 16777216.0) * 16.0 + 0.5), min(x, c) = x < c ? x : c (a NaN d * d, from
 *      inf - inf, takes the cap; its out_j is a NaN).
 *   counts[0] == counts[1] + counts[2] + counts[3] always, and counts[4] / (16 * counts[1]) is the mean squared difference BEFORE the
 *   step as an exact integer ratio: the stopping rule compares such ratios in integers.  All sums are integer sums (a term is at most
 *   2^28, a volume has fewer than 2^31 voxels): no result depends on the schedule.  out_dev is fully written, counts_out_dev is zeroed
 *   by the call.
 *
 * lm_jacobian_dev: field [3][n][h][w] -> det_out float32 [n][h][w] = det(I + G), G_ij = d(u_i * field_scale[i]) / d o_j, the Jacobian
 * of o -> o + u * field_scale in INDEX space.  With p_mm = D S (o + S^-1 u_mm) + origin (D the direction matrix, S the spacings) the
 * millimetre-space Jacobian is D S (I + G) S^-1 D^-1: a similarity transform of I + G, so the determinants are equal -- for ANY
 * invertible D, an orthonormal one included.  DEFINITION, float64 in the order written:
 *   Interior of axis j:       G_ij = (((double)u_i[o + e_j] - (double)u_i[o - e_j]) * field_scale[i]) * 0.5
 *   o_j == 0 (no lower):      G_ij = ((double)u_i[o + e_j] - (double)u_i[o]) * field_scale[i]
 *   o_j == e_j - 1:           G_ij = ((double)u_i[o] - (double)u_i[o - e_j]) * field_scale[i]
 *   (one-sided at the border, special-cased so that a linear field has an exact Jacobian there too); an axis of extent 1: G_ij = 0.0.
 *   a = I + G;  det = (a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20)) + a02 * (a10 * a21 - a11 * a20);
 *   det_out[o] = (float)det.  counts_out_dev (int64 [2], may be NULL; zeroed by the call): [0] the voxels with det <= 0.0 (folded),
 *   [1] those with a NaN det, both on the float64 value.
 * Limits of all three: every dimension in 1 .. 4096 and fewer than 2^31 voxels per volume; refused before anything is read.  No
 * workspace.  Enqueued on the engine's stream; the parameters are read before the call returns. */
typedef struct lm_demons_params {
    double A[9], b[3];      /* row-major: moving index = A * p + b */
    double field_scale[3];  /* 1 / spacing_i of the fixed grid, array axis order; 1.0 without a spacing */
    double grad_scale[3];   /* field_scale[i] / 2 */
    double inv_k2;          /* the weight of d^2 in the denominator, mm^-2 (>= 0) */
    double den_min;         /* below this denominator the step is 0 (>= 0) */
    uint8_t keep[256];      /* with labels: the label values that are selected */
} lm_demons_params;
int lm_warp_dev(lm_engine* e, const void* src_dev, int dtype, int n, int h, int w, const float* field_dev /* or NULL */,
                const lm_resample_params* p, const double field_scale[3], void* out_dev);
int lm_demons_step_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* fixed_lab_dev /* or NULL */,
                       const void* moving_dev, int mdtype, int mn, int mh, int mw, const float* u_dev, const lm_demons_params* p,
                       float* out_dev, int64_t* counts_out_dev);
int lm_jacobian_dev(lm_engine* e, const float* field_dev, int n, int h, int w, const double field_scale[3], float* det_out_dev,
                    int64_t* counts_out_dev /* or NULL */);

/* ---- local-correlation metric of the deformable registration (not in the reference: the metric for two scans whose intensities are
 *      related by a LOCAL affine map, an inspiration / expiration pair: within a window  m ~ air + (f - air) * J) ----------------------
 * Both entries take the fixed level volume f float32 [n][h][w] and m float32 [n][h][w], the moving volume ALREADY WARPED onto the same
 * grid (lm_warp_dev, LM_RS_LINEAR, with a NaN fill: a voxel that samples outside the moving volume is a NaN).  A voxel is VALID iff
 * f and m are both finite.  All arithmetic in float64 without fused multiply-add and in the order written.
 *
 * lm_local_moments_dev: -> out_dev float64 [6][n][h][w], the sums over the window of the VALID voxels of  1, f, m, f*f, m*m, f*m
 * (channels 0 .. 5; every product of two float32 values formed in float64, which is exact).  The window of voxel o is the box
 * o_i - radius[i] .. o_i + radius[i] clipped to the volume: nothing exists outside it.  radius[i] in 0 .. 8 (array axis order z, y, x).
 * DEFINITION: three separable passes, x, then y, then z.  The x pass forms the channels: for every voxel
 *     acc = 0.0;  for k = -radius[2] .. radius[2] ascending, x + k inside the row and that voxel valid:  acc = acc + term(x + k)
 * with term = 1.0, (double)f, (double)m, (double)f * (double)f, (double)m * (double)m, (double)f * (double)m.  The y and the z pass,
 * per channel, on the previous pass's values:  acc = 0.0;  for k = -r .. r ascending, in range:  acc = acc + in[i + k].  These are
 * DIRECT sums, not a sliding update: a sliding sum depends on the order of its updates and would not be reproducible bit for bit.
 * A y or z axis with radius 0 is the identity (the pass is skipped: its one-term sum 0.0 + v is v, no value being -0.0 after the x
 * pass); the x pass with radius 0 gives the terms of the voxel itself, zeros for a voxel that is not valid.
 * out_dev must not overlap f_dev or m_dev.  Workspace (grow-only, kept by the engine, only with radius[0] > 0 or radius[1] > 0): one
 * float64 array of the output's size, 48 bytes per voxel.
 *
 * lm_lcc_step_dev: ONE additive demons iteration on the residual of the window's affine intensity fit, with the ACTIVE force: the
 * gradient of the warped moving volume scaled by the fit's gain (it vanishes where the moving image is locally flat: a flat window
 * carries no information).  f, m, moments_dev (S_1, S_f, S_m, S_ff, S_mm, S_fm = the six channels of lm_local_moments_dev), optionally
 * fixed_lab_dev u8 [n][h][w], the current field u_dev float32 [3][n][h][w] -> out_dev float32 [3][n][h][w] (NOT u_dev) and
 * counts_out_dev int64 [6].  A, b, field_scale and moving_dims serve the outside test only: nothing is gathered.
 * DEFINITION, per fixed voxel o:
 *   1. Selection.  lm_demons_step_dev's: selected iff fixed_lab_dev is NULL or keep[label] != 0.  Not selected: out_j = u_j.
 *      Selected: counts[0]++.
 *   2. Coordinate.  The COORDINATE RULE of lm_warp_dev with u as the field and moving_dims as the extents.  Outside: counts[2]++ and
 *      out_j = u_j.
 *   3. f[o] or m[o] not finite, or N = S_1[o] < 2 (not N >= 2.0): counts[3]++ and out_j = u_j.
 *   4. mu_f = S_f / N;  mu_m = S_m / N;
 *      c_fm = S_fm - (S_f * S_m) / N;  c_mm = S_mm - (S_m * S_m) / N;  c_ff = S_ff - (S_f * S_f) / N.
 *   5. Gain.  a = c_fm / (c_mm + var_eps * N), then a = a < 0.0 ? 0.0 : (a > a_max ? a_max : a): an anti-correlated window gives no
 *      force, and var_eps (intensity^2) keeps the gain of a nearly flat window small.
 *   6. d = ((double)f - mu_f) - a * ((double)m - mu_m).
 *   7. Gradient.  g_j = a * (((double)m[o + e_j] - (double)m[o - e_j]) * grad_scale[j]), the neighbour indices CLAMPED to the volume
 *      as in lm_demons_step_dev's 5. -- the same difference, taken on m; an axis of extent 1 gives g_j = 0.0.
 *   8. den = ((g_0 * g_0 + g_1 * g_1) + g_2 * g_2) + (d * d) * inv_k2;  step_j = den < den_min ? 0.0 : (d * g_j) / den.
 *      A NaN among a, den and step_j (a NaN neighbour of m, a window without variance and var_eps = 0): as in 3.
 *   9. out_j = (float)((double)u_j + step_j);  counts[1]++;
 *      counts[4] += (int64)floor(min(d * d, 16777216.0) * 16.0 + 0.5);
 *      counts[5] += (int64)floor(rho2 * 1048576.0 + 0.5),  rho2 = (c_mm * c_ff > 0.0) ? min(max((c_fm * c_fm) / (c_mm * c_ff), 0.0), 1.0)
 *      : 0.0, the squared local correlation coefficient.
 *   counts[0] == counts[1] + counts[2] + counts[3] always.  counts[4] / (16 * counts[1]) is the mean squared residual and counts[5] /
 *   (2^20 * counts[1]) the mean squared local correlation BEFORE the step, as exact integer ratios.  All sums are integer sums.
 *   A step is at most 1 / (2 * sqrt(inv_k2)) long, as in lm_demons_step_dev: |d| |g| <= (|g|^2 + d^2 inv_k2) / (2 sqrt(inv_k2)).
 *   out_dev is fully written, counts_out_dev is zeroed by the call.  out_dev must overlap none of the inputs.
 * Limits of both: every dimension (moving_dims included) in 1 .. 4096 and fewer than 2^31 voxels; radius[i] in 0 .. 8; A, b,
 * field_scale, grad_scale finite; inv_k2, den_min, var_eps finite and >= 0; a_max finite and > 0.  Refused with LM_ERR_INVALID and a
 * message before anything is read.  Enqueued on the engine's stream; the parameters are read before the call returns. */
#define LM_LCC_MAX_RADIUS 8
typedef struct lm_lcc_params {
    double A[9], b[3];       /* row-major: moving index = A * p + b (the outside test) */
    double field_scale[3];   /* 1 / spacing_i of the fixed grid, array axis order; 1.0 without a spacing */
    double grad_scale[3];    /* field_scale[i] / 2 */
    double inv_k2;           /* the weight of d^2 in the denominator (>= 0) */
    double den_min;          /* below this denominator the step is 0 (>= 0) */
    double var_eps;          /* added to the window's variance of m per voxel, intensity^2 (>= 0) */
    double a_max;            /* the largest gain (> 0) */
    int32_t moving_dims[3];  /* the extents of the moving volume that m was warped from */
    uint8_t keep[256];       /* with labels: the label values that are selected */
} lm_lcc_params;
int lm_local_moments_dev(lm_engine* e, const float* f_dev, const float* m_dev, int n, int h, int w, const int32_t radius[3],
                         double* out_dev);
int lm_lcc_step_dev(lm_engine* e, const float* f_dev, const float* m_dev, const double* moments_dev, const uint8_t* fixed_lab_dev /* or NULL */,
                    int n, int h, int w, const float* u_dev, const lm_lcc_params* p, float* out_dev, int64_t* counts_out_dev);

/* ---- displacement fields as operands: a field sampled through another field, rotated, scaled and added (not in the reference: the one
 *      device operation under the inversion, the composition, the transport onto another grid and the difference of two fields) --------
 * lm_field_combine_dev: src float32 [3][n][h][w], and on the OUTPUT grid [N_0][N_1][N_2] (N voxels) the optional float32 [3][N] fields
 * add_dev, coord_dev and ref_dev -> out_dev float32 [3][N] and counts_out_dev int64 [4] (may be NULL).  DEFINITION, per output voxel
 * o, all in float64 without fused multiply-add and in the order written:
 *   1. Coordinate.  The COORDINATE RULE above with coord_dev as the field: p_i = (double)o_i + (double)coord_i[o] * field_scale[i]
 *      (p = o for NULL), c_i = ((A[3i] * p_0 + A[3i+1] * p_1) + A[3i+2] * p_2) + b_i, and lm_resample_dev's inside test on
 *      t_i = floor(c_i + 0.5) against n, h, w.  An OUTSIDE voxel counts in counts[0] and is STILL SAMPLED, at the clamped coordinate:
 *      a field is extended by its edge values, not by a fill.  (A NaN coordinate is outside and clamps to index 0.)
 *   2. Sample.  s_k = the trilinear value of lm_resample_dev (4. there) of component k of src at the clamped c, k = 0, 1, 2; the
 *      three components share one set of taps.
 *   3. Rotate.  t_j = (R[3j] * s_0 + R[3j+1] * s_1) + R[3j+2] * s_2.
 *   4. Combine.  v_j = beta * t_j, or with add_dev v_j = alpha * (double)add_j[o] + beta * t_j;  out_j = (float)v_j.
 *   5. Counts.  d_j = (double)out_j - (double)ref_j[o] (ref is 0.0 for NULL);  d2 = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2.  A NaN d2
 *      counts in counts[1] and contributes nothing else.  Otherwise q = (int64)floor(min(d2, 256.0) * 4194304.0 + 0.5),
 *      min(x, c) = x < c ? x : c;  counts[2] += q and counts[3] = max(counts[3], q).  q <= 2^30, so the sum stays below 2^61; all sums
 *      are integer sums and the maximum is an integer maximum: nothing depends on the schedule.  The resolution is 2^-22 squared
 *      units, 2^-11 units of the field; a difference longer than 16 units takes the cap.  The call zeroes counts_out_dev.
 *   NaN and inf follow from the formulas.
 * The uses (lungmask_amd/deformable.py):             add    coord  src  ref   alpha, beta   A, b, R
 *   inversion step w' = -u o (Id + w)                NULL   w      u    w     -, -1         identity
 *   composition u1 + R u2 o (T1)                     u1     u1     u2   NULL  1, 1          from the geometry
 *   transport of w onto another grid                 zeros  zeros  w    NULL  1, 1          from the geometry
 *   difference v - u                                 v      NULL   u    NULL  1, -1         identity
 * add_dev, coord_dev, src_dev and ref_dev may alias one another (all are read only); out_dev equal to any of them is refused.
 * Limits: every dimension of both grids in 1 .. 4096 and fewer than 2^31 voxels per grid; field_scale, A, b, R, alpha and beta
 * finite; refused before anything is read.  No workspace.  Enqueued on the engine's stream; p is read before the call returns. */
typedef struct lm_field_combine_params {
    int32_t out_dims[3];    /* N_0, N_1, N_2: the output grid */
    double A[9], b[3];      /* row-major: index in src's grid = A * p + b */
    double field_scale[3];  /* 1 / spacing_i of the OUTPUT grid (for coord_dev), array axis order; 1.0 without a spacing */
    double R[9];            /* row-major, applied to the sampled vector */
    double alpha, beta;
} lm_field_combine_params;
int lm_field_combine_dev(lm_engine* e, const float* add_dev /* [3][N] or NULL */, const float* coord_dev /* [3][N] or NULL */,
                         const float* src_dev, int n, int h, int w /* [3][n][h][w] */, const float* ref_dev /* [3][N] or NULL */,
                         const lm_field_combine_params* p, float* out_dev /* [3][N] */, int64_t* counts_out_dev /* [4] or NULL */);

/* ---- paired-CT analysis: parametric response map, mass-corrected density change, Jacobian per label (not in the reference: what the
 *      registration stack is for -- two CTs of one patient compared voxel by voxel without leaving the device) -------------------------
 * lm_pair_map_dev: fixed [fn][fh][fw] of fdtype, its labels lab u8 [fn][fh][fw], moving [mn][mh][mw] of mdtype (each dtype LM_I16,
 * LM_I32, LM_I64, LM_F32 or LM_F64), field_dev float32 [3][N] on the fixed grid or NULL (N = fn * fh * fw) -> class_out u8 [N],
 * change_out float32 [N], jac_out float32 [N] (each may be NULL) and table_out int64 [n_labels][LM_PAIR_COLS].  DEFINITION, per fixed
 * voxel o with L = lab[o]; all arithmetic float64 without fused multiply-add in the order written; min(x, c) = x < c ? x : c,
 * max(x, c) = x > c ? x : c; every sum is an integer sum, so nothing depends on the schedule:
 *   1. Selection.  Selected iff keep[L] != 0 and L < n_labels.  Not selected: class 0, change 0.0f, jac 0.0f.  Selected: T[L][0]++.
 *   2. f = (double)F[o].  A NaN: T[L][3]++ and the outputs of a voxel that is not selected.
 *   3. Coordinate.  The COORDINATE RULE of lm_warp_dev with the moving extents.  Outside: T[L][2]++, outputs as not selected.
 *   4. m = lm_resample_dev's trilinear value (4. there) on the clamped coordinate.  A NaN: as in 2.
 *   5. J = jac_scale * det, det = lm_jacobian_dev's float64 determinant at o (one-sided at the borders, 0.0 for an axis of extent 1),
 *      det = 1.0 with a NULL field.  A NaN J: as in 2.  J <= 0.0 (folded): T[L][4]++, class 0, change 0.0f, jac (float)J.
 *   6. mc = J * (m - air) + air;  change = mc - f.  A NaN change (inf - inf): as in 2.  Otherwise the voxel is VALID: T[L][1]++,
 *      jac = (float)J, change_out = (float)change,
 *        T[L][5] += (int64)floor(min(J, 64.0) * 1048576.0 + 0.5)
 *        T[L][6] += (int64)floor(max(min(change, 65536.0), -65536.0) * 16.0 + 0.5)        (signed)
 *        T[L][7] += (int64)floor(min(change * change, 16777216.0) * 16.0 + 0.5)
 *   7. Class.  Unless lo <= f <= hi and lo <= m <= hi: T[L][8]++ and class 0.  Otherwise code = 1 + (f < fixed_thr) +
 *      2 * (m < moving_thr), class = code and T[L][8 + code]++ (columns 9 .. 12).
 *   Columns: 0 selected, 1 valid, 2 outside, 3 non-finite, 4 folded, 5 sum of J in 2^-20, 6 sum of change in 1/16 HU, 7 sum of change^2
 *   in 1/16 HU^2, 8 valid but not classified, 9 .. 12 codes 1 .. 4.  Always T[.][0] == T[.][1] + T[.][2] + T[.][3] + T[.][4] and
 *   T[.][1] == T[.][8] + ... + T[.][12].  A term of column 5 is at most 2^26, of column 6 at most 2^20 in magnitude, of column 7 at most
 *   2^28, and a volume has fewer than 2^31 voxels: no sum overflows.  mc is the moving density carried onto the fixed voxel with its
 *   mass kept (the "sponge model": tissue inflated by J is 1 / J as dense; HU - air is proportional to density).
 * The call zeroes the table; every non-NULL output is fully written; an output that overlaps an input or another output is refused.
 * Limits as for lm_warp_dev (every dimension of both volumes in 1 .. 4096, fewer than 2^31 voxels per volume); n_labels in 1 .. 16; A,
 * b, field_scale, air, both thresholds, lo and hi finite; jac_scale finite and > 0; lo <= hi; refused before anything is read.  No
 * workspace.  Enqueued on the engine's stream; p is read before the call returns. */
#define LM_PAIR_COLS 13
typedef struct lm_pair_params {
    double A[9], b[3];        /* moving index = A * p + b  (index_map(moving grid, fixed grid, affine)) */
    double field_scale[3];    /* 1 / spacing_i of the fixed grid; 1.0 without a spacing */
    double jac_scale;         /* |det| of the affine's matrix under the field (1.0 without one); finite, > 0 */
    double air;               /* HU of zero density, -1000.0 */
    double fixed_thr, moving_thr;   /* "low" is value < threshold */
    double lo, hi;            /* a voxel is classified iff lo <= f <= hi and lo <= m <= hi */
    int32_t n_labels;         /* 1 .. 16 rows of the table */
    uint8_t keep[256];
} lm_pair_params;
int lm_pair_map_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* lab_dev,
                    const void* moving_dev, int mdtype, int mn, int mh, int mw, const float* field_dev /* [3][N] or NULL */,
                    const lm_pair_params* p, uint8_t* class_out_dev /* [N] or NULL */, float* change_out_dev /* [N] or NULL */,
                    float* jac_out_dev /* [N] or NULL */, int64_t* table_out_dev /* [n_labels][LM_PAIR_COLS] */);

/* ---- surface mesh of a label selection (not in the reference: what callers run marching cubes on the finished mask for) ------------
 * lab u8 [n][h][w] -> verts_out float32 [V][3] and quads_out int32 [Q][4]: SURFACE NETS of the binary selection.  DEFINITION:
 *   Selection.  A voxel is selected when keep[label] != 0 (the 256-entry table of lm_roi_plan_dev).  Voxels outside the volume count
 *      as unselected, so a selection that touches the border still closes.
 *   Cells.  Voxel centres sit at the integer indices (z, y, x).  There are (n + 1)(h + 1)(w + 1) cells: cell (k, j, i), k in
 *      [-1, n - 1] and likewise j and i, has the 8 corner voxels (k + a, j + b, i + c), a, b, c in {0, 1}.  A cell is active when its
 *      corners are not all equal.
 *   Vertices.  One per active cell, numbered in raster order of (k, j, i).  With cnt (1..12) the number of the cell's 12 edges whose
 *      two ends differ and S2[d] the integer sum over those edges of (offset of end 0 + offset of end 1) along axis d (twice the
 *      midpoint's offset), the vertex in array index coordinates is
 *          p[d] = fl32(fl32(base[d]) + fl32(fl32(S2[d]) / fl32(2 * cnt))),  base = (k, j, i),
 *      written as (z, y, x).
 *   Faces.  One quad for every pair of axis neighbours v, v + e_a whose selection differs (either may lie in the one-voxel border
 *      outside the volume).  It joins the four cells that contain that grid edge.  Its first corner is the cell with the smallest
 *      raster index of the four; the others follow round the edge in the direction that makes the right-hand normal
 *      (p1 - p0) x (p2 - p0), with the components taken in (z, y, x) order, point from the selected to the unselected voxel.  Quads
 *      are ordered by the raster index of the lower voxel v in the padded grid, then by axis z, y, x.  Triangles, where wanted, are
 *      corners (0, 1, 2) and (0, 2, 3) of each quad; the host derives them.
 *   Smoothing.  `smooth` Taubin iterations (0: none): one Jacobi pass with factor `lambda`, then one with factor `mu` (customary:
 *      0.5 and -0.53), both reading the previous positions.  The neighbours of the vertex of cell c are the vertices of the cells
 *      c - e_z, c + e_z, c - e_y, c + e_y, c - e_x, c + e_x, in that order; a neighbour counts only when the four voxels of the shared
 *      cell face are not all equal (every active cell has at least two).  Per component, float32 without fused multiply-add:
 *      m = (((0 + v_1) + v_2) + ...) over the counting neighbours in order, avg = m / (float)count, p' = p + f * (avg - p).
 *      Uniform weights in index space commute with an affine map to millimetres, so the device never sees a spacing.
 *   Properties.  The mesh is closed (every directed quad side has its reverse).  It can be non-manifold where two selected voxels
 *      meet only across an edge or a corner.  Naive surface nets shrink features one voxel wide: a single voxel becomes a cube of
 *      side 1/3.
 * Limits are lm_roi_plan_dev's (n, h, w <= 4096, n * h * w < 2^31; refused before anything is read), and V, Q < 2^31.  No selected
 * voxel: LM_ERR_INVALID, "no kept voxel", as lm_roi_plan_dev.
 *
 * lm_mesh_plan_dev: bbox_out (HOST) = the margin-0 box of the selection (lm_roi_plan_dev's), *n_vertices = V, *n_quads = Q.  Runs the
 * counting pass on the box grown by one cell and returns once the counts are known.
 * lm_mesh_dev: writes V vertices and Q quads.  n_vertices_cap < V or n_quads_cap < Q: LM_ERR_INVALID ("capacity"), nothing is written;
 * it never writes past a capacity.  Called right after lm_mesh_plan_dev with the same lab_dev, dimensions and keep table it reuses that
 * plan (once; the labels must not change in between); otherwise it plans itself.  Workspace (grow-only, kept by the engine): 4 bytes
 * per cell of the box grown by one cell, 16 bytes per workgroup of the two passes, and with smooth > 0 17 bytes per vertex.  Enqueued on
 * the engine's stream. */
int lm_mesh_plan_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], int32_t bbox_out[6],
                     int64_t* n_vertices, int64_t* n_quads);
int lm_mesh_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], int smooth, float lambda, float mu,
                float* verts_out_dev, int64_t n_vertices_cap, int32_t* quads_out_dev, int64_t n_quads_cap);

/* ---- label morphology (not in the reference: what callers run scipy.ndimage on the finished mask for) -----------------------------
 * lm_nearest_label_dev: lab u8 [n][h][w] -> d2_out f32 [n][h][w] (may be NULL) and near_out u8 [n][h][w]: the squared distance to the
 * nearest feature and WHICH label that feature carries.  DEFINITION.  A voxel is a feature when keep[lab] != 0.  The weights are
 * lm_edt_dev's, w_i = (float)(spacing_i * spacing_i), and so are the three passes, carried out on pairs (d, k) that are ordered
 * lexicographically: the smaller float32 d first, then the smaller label k.
 *     g1[z][y][x] = lexmin over the features x' of the row of (w_x * (float)((x-x')^2), lab[z][y][x'])     (+inf, 0) for a row without one
 *     g2[z][y][x] = lexmin over y' of (fl(g1.d[z][y'][x] + fl(w_y * (float)((y-y')^2))), g1.k[z][y'][x])
 *     g3[z][y][x] = lexmin over z' of (fl(g2.d[z'][y][x] + fl(w_z * (float)((z-z')^2))), g2.k[z'][y][x])
 *     d2_out = g3.d, near_out = g3.k.
 * Every candidate with d = +inf carries k = 0, so a volume without a feature gives +inf and 0 everywhere.  d2_out equals lm_edt_dev
 * on the u8 volume keep[lab] bit for bit (the second key never changes the minimum of the first).  near_out is defined BY THE
 * RECURSION, not as "the smallest label among all global minimisers": the two can differ where float rounding turns a strict
 * inequality of one pass into a tie in the next.  The value does not depend on the schedule.  Limits are lm_edt_dev's (every dimension
 * <= 4096, n * h * w < 2^31; refused before anything is read).  Both outputs are worked on in place; without d2_out_dev the distances
 * live in the engine's workspace.  near_out_dev must not be lab_dev.  Enqueued on the engine's stream.
 *
 * lm_morph_dev: lab u8 [n][h][w] -> out u8 [n][h][w] (out_dev may be lab_dev).  DEFINITIONS, with S = {keep[lab] != 0},
 * r2 = (float)(radius_mm * radius_mm) (the product in double), d(v, X) = lm_edt_dev's float32 squared distance (p->spacing) of voxel v
 * to the voxel set X:
 *     D(X) = {v : d(v, X) <= r2}                                   dilation by the ball of radius_mm
 *     E(X) = {v in X : d(v, volume \ X) > r2}                      erosion; the complement is taken INSIDE the volume
 * Outside the volume there are no voxels: dilation finds nothing selected there and erosion no background, so the volume's border does
 * not erode.  On the volume's voxel set D and E are adjoint (the float32 distance expression is symmetric in its two voxels), hence
 * closing is extensive and idempotent, opening anti-extensive and idempotent, exactly.
 *     LM_MORPH_DILATE  a voxel of D(S) \ S with into[lab] != 0 takes near (lm_nearest_label_dev of S); every other voxel is unchanged.
 *     LM_MORPH_ERODE   a voxel of S \ E(S) becomes 0.
 *     LM_MORPH_OPEN    a voxel of S \ D(E(S)) becomes 0.
 *     LM_MORPH_CLOSE   a voxel of E(D(S)) \ S with into[lab] != 0 takes near, the nearest label OF S: the closing acts on the selection
 *                      as a whole and new voxels go to the nearest lung or lobe.
 * 0 <= radius_mm < 1e15 (r2 stays finite in float32; the bound of lm_roi_dev's dilate_mm and of every spacing), or +inf for
 * LM_MORPH_DILATE only (propagation: every `into` voxel takes the nearest kept label); anything else is LM_ERR_INVALID.  radius_mm == 0
 * is the identity.  changed_host (HOST): voxels added, voxels removed.  No selected voxel: LM_ERR_INVALID, "no kept voxel", as
 * lm_roi_plan_dev.  The transforms run inside the box of S (lm_roi_plan_dev's kernel) grown per axis by ceil(radius_mm / s_i) + 1
 * voxels and clipped to the volume, which is exact.  Limits are lm_edt_dev's.  Workspace (grow-only, kept by the
 * engine): per voxel of that box one float32 and one u8, and for dilate and close a second u8.  Returns once changed_host is known. */
enum { LM_MORPH_DILATE = 0, LM_MORPH_ERODE = 1, LM_MORPH_OPEN = 2, LM_MORPH_CLOSE = 3 };
typedef struct lm_morph_params {
    int32_t op;
    double radius_mm;
    double spacing[3];   /* array axis order; 1, 1, 1 = voxels */
    uint8_t keep[256];   /* the selection S */
    uint8_t into[256];   /* labels a grown voxel may overwrite (customary: 0 only) */
} lm_morph_params;
int lm_nearest_label_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], const double* spacing,
                         float* d2_out_dev, uint8_t* near_out_dev);
int lm_morph_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const lm_morph_params* p, uint8_t* out_dev,
                 int64_t changed_host[2]);

/* ---- connected components of a selection inside the labels (not in the reference: what callers run scipy.ndimage.label for) ------
 * lm_components_dev: lab u8 [n][h][w] and, optionally, vol [n][h][w] of `dtype` (LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64; vol_dev
 * NULL: no image, dtype ignored) -> ids_out int32 [n][h][w].  DEFINITIONS (all integer).
 *   HU value of a voxel: exactly lm_label_stats_dev's -- integer volumes hu = v (LM_I64: saturated to the int32 range); float volumes
 *     hu = rint(v) (round half to even), saturated to the int32 range, +-inf included; NaN is NONFINITE.
 *   Selection: voxel v is selected iff keep[lab[v]] != 0 and (no image is given, or v is not nonfinite and (!has_lo || lo <= hu) and
 *     (!has_hi || hu <= hi)).  has_lo && has_hi && lo > hi is LM_ERR_INVALID.
 *   Key: key(v) = lab[v] with per_label != 0 (a component never crosses a label border), otherwise 1.  keep[0] != 0 with per_label is
 *     LM_ERR_INVALID (the key of a selected voxel must not be 0).
 *   Connectivity: two selected voxels are connected when their keys are equal and they are 6-adjacent (connectivity 6: they share a
 *     face, scipy.ndimage.label's default structure) or 26-adjacent (connectivity 26: their indices differ by at most 1 on every axis).
 *     Nothing exists outside the volume.  Any other connectivity is LM_ERR_INVALID.
 *   ids: 0 where v is not selected, otherwise 1 .. T, the components numbered by the raster (C-order) index of their first voxel;
 *     for a binary selection this is scipy.ndimage.label's numbering with the matching structure.  *total_out = T.
 *   counts_host [3][256] int64 (HOST), from the selection pass: [0][k] voxels with lab == k, [1][k] those of them that are nonfinite
 *     (0 without an image), [2][k] those that are selected.
 * Every dimension <= 4096 and n * h * w < 2^31.  The inputs are not written.  Workspace
 * (grow-only, kept by the engine): one u8 and two int32 per voxel.  Runs the selection, the engine's union-find labelling and its
 * dense raster-order numbering on the engine's stream, and returns once T and the counts are on the host.
 *
 * lm_component_table_dev: one row per component of ANY int32 id volume (ids <= 0: no component) over lab and, optionally, vol.  Row
 * i - 1 of table_host (HOST, `cap` rows) describes id i, for 1 <= i <= min(T, cap), where T = *total_out = the largest id present
 * (0: none); ids beyond cap are ignored and rows beyond min(T, cap) are not written.  The device tables are sized by cap.
 *   voxels; first = the raster index of its first voxel; label = lab[first] (the label of the FIRST voxel: with per_label ids every
 *   voxel of the component carries it); bbox = zmin, zmax, ymin, ymax, xmin, xmax with exclusive maxima (lm_label_stats_dev's
 *   convention); index_sum = (sum z, sum y, sum x); hu_sum, hu_min, hu_max over its voxels that are not nonfinite (ids from
 *   lm_components_dev with the same image have no other; all three 0 without an image or without such a voxel); faces[a] for a = z,
 *   y, x = the number of (voxel, side) pairs, over the component's voxels and the two sides along axis a, whose neighbouring voxel
 *   lies outside the volume or has another id -- the voxel faces normal to that axis that bound the component.
 *   An id that no voxel carries (possible only for foreign ids) gives a row of zeros with bbox -1 and first -1.
 * Integer arithmetic throughout: the result does not depend on the schedule.  0 <= cap < 2^31; limits as above.  Returns once the
 * rows are on the host.  lm_component_table_launch reports the launch geometry of its main kernel for nvox voxels: the number of
 * workgroups and the length of the contiguous voxel range each of them walks (a large component costs one set of global atomics per
 * workgroup it touches, a small one one set in all).
 *
 * lm_relabel_dev: out[v] = lut[ids[v]] for nvox voxels (int32 everywhere, all on the device; out_dev may be ids_dev).  An id that is
 * negative or >= lut_len is never looked up: the voxel is written as 0, a device flag is raised and the call returns LM_ERR_INVALID
 * ("id outside the table") once the pass has finished.  Returns once the flag is on the host. */
typedef struct lm_components_params {
    uint8_t keep[256];
    int32_t lo, hi;          /* inclusive HU bounds, used when has_lo / has_hi != 0 */
    int32_t has_lo, has_hi;
    int32_t per_label;
    int32_t connectivity;    /* 6 or 26 */
} lm_components_params;
typedef struct lm_component {
    int64_t voxels;
    int64_t index_sum[3];
    int64_t hu_sum;
    int64_t faces[3];
    int32_t bbox[6];
    int32_t hu_min, hu_max;
    int32_t label;
    int32_t first;
} lm_component;
int lm_components_dev(lm_engine* e, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h, int w,
                      const lm_components_params* p, int32_t* ids_out_dev, int64_t* total_out, int64_t counts_host[3][256]);
int lm_component_table_dev(lm_engine* e, const int32_t* ids_dev, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h,
                           int w, lm_component* table_host, int64_t cap, int64_t* total_out);
int lm_component_table_launch(int64_t nvox, int64_t* workgroups, int64_t* voxels_per_workgroup);
int lm_relabel_dev(lm_engine* e, const int32_t* ids_dev, const int32_t* lut_dev, int64_t lut_len, int64_t nvox, int32_t* out_dev);

/* ---- lung-aware image filters (not in the reference: what callers run scipy.ndimage.median_filter / gaussian_filter for) ----------
 * lm_filter_dev: vol [n][h][w] of `dtype` and, optionally, lab u8 [n][h][w] -> out [n][h][w].  out_dev must not be vol_dev.
 * DEFINITIONS.
 *   Selection.  With LM_FILTER_MASKED a voxel is selected iff keep[lab] != 0.  Without the flag every voxel is selected and lab_dev
 *     may be NULL (keep, fill and LM_FILTER_FILL_OUTSIDE are then ignored).  Masked without a selected voxel: LM_ERR_INVALID, "no kept
 *     voxel", as lm_roi_plan_dev.
 *   LM_FILTER_MEDIAN.  size[i] in {1, 3, 5} per array axis; dtype LM_I16, LM_I32 or LM_F32, out of the same dtype (anything else is
 *     LM_ERR_INVALID).  Order: ascending value, -0.0 before +0.0; NaN never takes part.
 *       Unmasked: the window is size[0] x size[1] x size[2] around the voxel, indices clamped to the volume (scipy's mode="nearest").
 *         out = the element of rank (cnt - 1) / 2 (integer division, rank 0 = the smallest) of the window's non-NaN values, cnt their
 *         number; cnt == 0 gives NaN (0x7fc00000).
 *       Masked: nothing exists outside the volume.  The window of a selected voxel holds the selected, non-NaN voxels of it, and the
 *         same rank rule applies (an even cnt gives the lower median).  A NaN centre is selected but contributes nothing.  A voxel
 *         that is not selected keeps its source value, or takes (dtype)fill with LM_FILTER_FILL_OUTSIDE (for the integer dtypes fill
 *         must be an integer of the dtype's range: LM_ERR_INVALID otherwise).
 *     The result is one of the input values, bit for bit: integer results are exact.
 *   LM_FILTER_SEPARABLE.  dtype LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64, read as (float)v; out is float32.  radius[i] <= 32;
 *     taps[i][k], k = 0 .. 2 radius[i], is the tap at offset k - radius[i] along array axis i.  Three passes, along x (axis 2), then y,
 *     then z, each writing a float32 volume; a pass of radius r with taps w computes at index i of its line
 *         acc = 0.0f;  for k = -r .. r ascending:  acc = fl32(acc + fl32(in[j(i + k)] * w[k]))        (no fused multiply-add)
 *     A pass with r == 0 and w[0] == 1 is skipped (exact).
 *       Unmasked: j clamps to the line.
 *       Masked (normalised convolution): nothing exists outside the volume -- those terms are left out.  The passes run on
 *         num = selected ? (float)v : 0 and on den = selected ? 1 : 0 with the same taps; a selected voxel gets fl32(num / den), a
 *         correctly rounded division; a voxel that is not selected gets (float)v, or fill with LM_FILTER_FILL_OUTSIDE.  Every tap
 *         must be >= 0 and every centre tap > 0 (LM_ERR_INVALID otherwise), which keeps den > 0 where it is used unless the
 *         product of the centre taps underflows.
 *     LM_FILTER_INDICATOR replaces the source value, wherever it is read, by (nonfinite ? 0 : ind_lo <= hu && hu <= ind_hi ? 1 : 0)
 *     with hu and nonfinite lm_label_stats_dev's HU value of the voxel (integers as they are, LM_I64 saturated; floats rint half to
 *     even, saturated to int32; NaN nonfinite).  INT32_MIN / INT32_MAX make a bound open.
 *     Which NaN comes out of NaN or inf input (sign, payload) is not defined; where it comes out is.
 * Limits are lm_edt_dev's (every dimension <= 4096, n * h * w < 2^31; refused before anything is read).  Workspace (grow-only, kept by
 * the engine): unmasked separable one float32 volume (two or three passes); masked separable two float32 per voxel of the box of the
 * selection grown by the radii (four with three passes) -- the passes run inside that box, which is exact; the
 * median none.  Everything is enqueued on the engine's stream; the masked forms first wait for lm_roi_plan_dev's box.  p is read
 * before the call returns. */
enum { LM_FILTER_MEDIAN = 0, LM_FILTER_SEPARABLE = 1 };
#define LM_FILTER_MASKED 1u
#define LM_FILTER_INDICATOR 2u
#define LM_FILTER_FILL_OUTSIDE 4u
typedef struct lm_filter_params {
    int32_t kind;
    int32_t size[3];      /* median window per array axis: 1, 3 or 5 */
    int32_t radius[3];    /* separable: tap radius per array axis, 0 .. 32 */
    float taps[3][65];    /* separable: taps[i][k] = the tap at offset k - radius[i] */
    uint8_t keep[256];    /* keep[label] != 0: the label is selected */
    uint32_t flags;       /* LM_FILTER_MASKED | LM_FILTER_INDICATOR | LM_FILTER_FILL_OUTSIDE */
    int32_t ind_lo, ind_hi;
    float fill;
} lm_filter_params;
int lm_filter_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev /* NULL: unmasked */, int n, int h, int w,
                  const lm_filter_params* p, void* out_dev);

/* ---- Hessian, eigenvalues and vesselness (not in the reference: the multi-scale Frangi filter callers run on the host) -------------
 * lm_hessian_dev: vol [n][h][w] of `dtype` and, optionally, lab u8 [n][h][w], ONE scale (p->n_scales == 1) -> comp_out float32
 *   [6][n][h][w], the normalised components in the order xx, yy, zz, xy, xz, yz (x = array axis 2, y = axis 1, z = axis 0), and,
 *   when eig_out_dev is not NULL, float32 [3][n][h][w] = l1, l2, l3.
 * lm_vesselness_dev: the same inputs, 1 .. 8 scales -> v_out float32 [n][h][w] and, when not NULL, scale_out u8 [n][h][w].
 * lm_vessel_counts_dev: V, scale, lab -> counts (HOST) int64 [n_labels][9]: counts[l][s] = the voxels with lab == l, scale == s and
 *   V >= threshold, for l in 1 .. n_labels - 1 (row 0 stays 0; labels >= n_labels and scale values > 8 take no part).
 * DEFINITIONS.  Everything is float32, every operation rounded on its own (no fused multiply-add), and only + - * / sqrt (all
 * correctly rounded), rint and bit operations are used: device, emulator and a numpy restatement agree bit for bit.
 *   Selection.  With LM_VESSEL_MASKED a voxel is selected iff keep[lab] != 0; without it every voxel is (lab_dev may be NULL).  Only
 *     selected voxels are analysed; every other voxel of every output is 0.  At a selected voxel the result equals the unmasked
 *     result bit for bit (nothing is confined: the taps see the whole volume).  Masked without a selected voxel: LM_ERR_INVALID,
 *     "no kept voxel", as lm_roi_plan_dev.
 *   Derivatives.  scales[s].taps[i][o][k], k = 0 .. 2 radius[i], is the tap of derivative order o (0, 1, 2) at offset k - radius[i]
 *     along array axis i (radius <= 32).  The component with orders (oz, oy, ox) is LM_FILTER_SEPARABLE's unmasked result with the
 *     taps (taps[0][oz], taps[1][oy], taps[2][ox]), bit for bit: three passes x, y, z, each
 *         acc = 0.0f;  for k = -r .. r ascending:  acc = fl32(acc + fl32(in[clamp(i + k)] * w[k])),
 *     a pass with r == 0 and w[0] == 1 being the identity.  Hxx: (0, 0, 2), Hyy: (0, 2, 0), Hzz: (2, 0, 0), Hxy: (0, 1, 1),
 *     Hxz: (1, 0, 1), Hyz: (1, 1, 0).
 *   Scale normalisation.  h_ab = fl32(nrm[ab] * H_ab), nrm in the components' order; the caller passes nrm_ab = (float)(sigma_a *
 *     sigma_b) with the sigmas in voxels of their axes (= sigma_mm^2 times the derivative per mm, whatever the spacing).  With
 *     LM_VESSEL_DARK H_ab is negated first (dark tubes on a bright background).
 *   Eigenvalues.  A = [[hxx hxy hxz] [hxy hyy hyz] [hxz hyz hzz]] (index 0 = x).  Cyclic Jacobi, 4 sweeps over the pairs (p, q) =
 *     (0, 1), (0, 2), (1, 2); a pair with a_pq == 0 is skipped; otherwise, r being the third index,
 *         theta = (a_qq - a_pp) / (2 a_pq);  t = sgn(theta) / (|theta| + sqrt(theta theta + 1)), sgn = -1 for theta < 0, else +1;
 *         c = 1 / sqrt(t t + 1);  s = t c;  tau = s / (1 + c);  h = t a_pq;  a_pp -= h;  a_qq += h;  a_pq = 0;
 *         a_rp' = a_rp - s (a_rq + tau a_rp);  a_rq' = a_rq + s (a_rp - tau a_rq)        (both from the old a_rp, a_rq).
 *     (l1, l2, l3) = the diagonal (a_00, a_11, a_22) after three compare-exchange steps on the positions (1, 2), (2, 3), (1, 2), each
 *     exchanging when |first| > |second|: ascending |lambda|, stable.  On 400 000 float32 matrices (degenerate, diagonal, zero and
 *     1e4-scaled families included) the recipe stayed within 3.83 x 2^-24 x ||A||_F of float64 eigenvalues.
 *   vexp(x), x <= 0.  0 for x < -87; NaN for NaN; otherwise k = rint(fl(x * 1.44269504f)) (half to even),
 *     r = fl(fl(x - fl(k * 0.693359375f)) - fl(k * -2.12194440e-4f)), p = 1.9875691500e-4f, then p = fl(fl(p * r) + c) for c =
 *     1.3981999507e-3f, 8.3334519073e-3f, 4.1665795894e-2f, 1.6666665459e-1f, 5.0000001201e-1f, y = fl(fl(fl(p * fl(r * r)) + r) + 1),
 *     vexp = y * 2^k (exact: the result is a normal number).  Within 1 ulp of exp on [-87, 0], exactly 1 at 0, never above 1.
 *   Vesselness (Frangi, bright tubes).  V = 0 unless l2 < 0 and l3 < 0 and fl(l2 * l3) > 0 (so NaN gives 0).  Otherwise, with a_i =
 *     fl(l_i * l_i): Ra2 = a2 / a3, Rb2 = a1 / fl(l2 * l3), S2 = fl(fl(a1 + a2) + a3) and
 *         V = fl(fl((1 - vexp(-fl(Ra2 * ka))) * vexp(-fl(Rb2 * kb))) * (1 - vexp(-fl(S2 * kc)))),
 *     ka, kb, kc = (float)(1 / (2 alpha^2)), (float)(1 / (2 beta^2)), (float)(1 / (2 c^2)) from the caller (>= 0 and finite).
 *   Multi-scale.  The scales run in the caller's order; V starts at 0 and a strictly greater value replaces the held one (a NaN
 *     never does); scale = the 1-based index of the scale whose value is held, 0 where V == 0.
 * dtype LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64, read as (float)v.  Limits are lm_edt_dev's.  The inputs are not written; the outputs
 * must not overlap them.  Workspace (grow-only, kept by the engine): nine float32 volumes of the box of the selection grown by the
 * largest radii (of the volume without labels) -- the passes run inside that box, which is exact.  Everything is
 * enqueued on the engine's stream; the masked forms first wait for lm_roi_plan_dev's box, and lm_vessel_counts_dev returns once the
 * counts are on the host.  p is read before the call returns. */
#define LM_VESSEL_MASKED 1u
#define LM_VESSEL_DARK 2u
#define LM_VESSEL_MAX_SCALES 8
typedef struct lm_vessel_scale {
    int32_t radius[3];     /* tap radius per array axis, 0 .. 32 */
    float taps[3][3][65];  /* taps[axis][order][k] = the tap of that derivative order at offset k - radius[axis] */
    float nrm[6];          /* xx, yy, zz, xy, xz, yz */
} lm_vessel_scale;
typedef struct lm_vessel_params {
    uint8_t keep[256];     /* keep[label] != 0: the label is selected */
    uint32_t flags;        /* LM_VESSEL_MASKED | LM_VESSEL_DARK */
    float ka, kb, kc;      /* lm_vesselness_dev only */
    int32_t n_scales;      /* 1 .. 8; lm_hessian_dev: 1 */
    lm_vessel_scale scales[LM_VESSEL_MAX_SCALES];
} lm_vessel_params;
int lm_hessian_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev /* NULL: unmasked */, int n, int h, int w,
                   const lm_vessel_params* p, float* comp_out_dev, float* eig_out_dev /* or NULL */);
int lm_vesselness_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev /* NULL: unmasked */, int n, int h, int w,
                      const lm_vessel_params* p, float* v_out_dev, uint8_t* scale_out_dev /* or NULL */);
int lm_vessel_counts_dev(lm_engine* e, const float* v_dev, const uint8_t* scale_dev, const uint8_t* lab_dev, int n, int h, int w,
                         int n_labels, float threshold, int64_t* counts_host);

/* ---- skeleton, calibre classes (not in the reference: the centreline and the distance transform callers compute on the host) --------
 * lm_skeleton_dev: sel u8 [n][h][w] and a keep table -> out u8 [n][h][w], the topology-preserving curve skeleton of
 * S = {v : keep[sel[v]] != 0}, coded by the number of skeleton neighbours.  DEFINITIONS, all in integers:
 *   Connectivity.  Object voxels are 26-connected, background voxels 6-connected.  Nothing outside the volume is object: outside the
 *     volume is background.  N6 / N18 / N26(v) are the voxels that differ from v by at most 1 in every coordinate and in at most 1 /
 *     2 / 3 coordinates, v itself excluded.
 *   Simple point.  v in S is simple iff (a) the object voxels of N26(v) form exactly one 26-connected set, and (b) among the
 *     6-connected sets that the background voxels of N18(v) form within N18(v), exactly one contains a voxel of N6(v).
 *   End point.  v has at most one object voxel in N26(v).  End points (isolated voxels included) are never deleted.
 *   Pass.  48 sub-steps (d, f): the direction d in the order -z, +z, -y, +y, -x, +x, and within a direction the subfield f = 0 .. 7,
 *     f(v) = ((z & 1) << 2) | ((y & 1) << 1) | (x & 1) from the voxel's index IN THE VOLUME.  Sub-step (d, f) takes the voxels of S in
 *     subfield f whose neighbour in direction d is background and deletes, simultaneously, those that are not end points and are
 *     simple with respect to S at the start of the sub-step.
 *   Passes repeat until a whole pass deletes nothing; what is left is K.  Two voxels of one subfield are never 26-adjacent, so the
 *     simultaneous deletion equals a sequential one, and every deletion of a simple point keeps the number of 26-components, of
 *     cavities and of tunnels: K has the topology of S exactly.  The result does not depend on the schedule.
 *   out[v] = 0 outside K and 1 + |N26(v) and K| on K: 1 isolated, 2 end, 3 curve voxel, >= 4 junction voxel.
 *   info_host (HOST) = |S|, |K|, the number of passes (the last, empty one included), 0.
 * out_dev may be sel_dev.  No selected voxel: LM_ERR_INVALID, "no kept voxel", as lm_roi_plan_dev.  Limits are lm_edt_dev's.  The
 * thinning runs in the box of S (lm_roi_plan_dev's kernel) with a border of one background voxel, which is exact: everything outside
 * the box is background either way.  One launch per sub-step, one counter read back per pass; more than |S| + 1 passes cannot happen
 * (every pass but the last deletes a voxel) and would be LM_ERR_DEVICE, "internal".  Workspace (grow-only, kept by the engine): one u8
 * per voxel of that bordered box.  Returns once info_host is known.
 *
 * lm_skeleton_points_dev: skel u8 [n][h][w] (lm_skeleton_dev's out) -> the list of its non-zero voxels in ascending raster order:
 * index_out int32 [cap] (the raster index (z * h + y) * w + x), code_out u8 [cap] (skel there) and, when d2_dev (float32 [n][h][w]) is
 * given, d2_out float32 [cap] (d2_dev there; d2_out_dev is then required, otherwise ignored).  *total_out (HOST) = the number of
 * non-zero voxels; only the first min(total, cap) entries are written, cap >= 0.  Returns once total_out is known.
 *
 * lm_calibre_dev: skel (lm_skeleton_dev's out), sel + keep (the mask M = {keep[sel] != 0}), optionally lab u8, spacing and n_edges
 * (1 .. 7) edges in mm, strictly ascending, > 0 and < 1e15 (anything else: LM_ERR_INVALID) ->
 *   d2        = lm_edt_dev(feature = voxel of the volume not in M, spacing): +inf everywhere when M is the whole volume.
 *   cls[v]    = 1 + #{j : d2[v] >= (float)(edges_mm[j] * edges_mm[j])} (the square in double) where skel[v] != 0 and v in M, else 0.
 *   class_out = lm_nearest_label_dev(cls, keep = every value >= 1, spacing)'s near_out on the voxels of M, its own tie rule; 0
 *               elsewhere (and on M where cls is 0 everywhere).
 *   counts_host (HOST) int64 [n_labels][9]: counts[k][c] = the voxels of M with lab == k and class_out == c, k in 1 .. n_labels - 1
 *               (row 0 stays 0; labels >= n_labels take no part); lab_dev == NULL: every voxel of M counts in row 1.
 *   d2_out_dev (float32 [n][h][w], or NULL) receives d2.
 * Everything but the comparisons on d2 is integer: the result does not depend on the schedule.  2 <= n_labels <= 16.  class_out_dev
 * must not be skel_dev, sel_dev or lab_dev.  Limits are lm_edt_dev's.  Workspace (grow-only, kept by the engine): two u8 volumes and
 * up to two float32 volumes of the input's size.  Returns once counts_host is known.
 *
 * lm_vessel_mask_dev: V float32 [n][h][w] and lab u8 [n][h][w] -> out u8 [n][h][w] = 1 where lab != 0 and V >= threshold (a NaN never
 * is), else 0: the vessel mask of lm_vesselness_dev's map inside (eroded) labels, on the device.  out_dev may be lab_dev.  Limits are
 * lm_edt_dev's.  Enqueued on the engine's stream. */
#define LM_CALIBRE_MAX_EDGES 7
#define LM_CALIBRE_COLUMNS 9
int lm_skeleton_dev(lm_engine* e, const uint8_t* sel_dev, int n, int h, int w, const uint8_t keep[256], uint8_t* out_dev /* may be sel_dev */,
                    int64_t info_host[4]);
int lm_skeleton_points_dev(lm_engine* e, const uint8_t* skel_dev, const float* d2_dev /* or NULL */, int n, int h, int w, int64_t cap,
                           int32_t* index_out_dev, uint8_t* code_out_dev, float* d2_out_dev, int64_t* total_out);
int lm_calibre_dev(lm_engine* e, const uint8_t* skel_dev, const uint8_t* sel_dev, const uint8_t keep[256], const uint8_t* lab_dev /* or NULL */,
                   int n, int h, int w, const double* spacing, const double* edges_mm, int n_edges, int n_labels, uint8_t* class_out_dev,
                   float* d2_out_dev /* or NULL */, int64_t* counts_host);
int lm_vessel_mask_dev(lm_engine* e, const float* v_dev, const uint8_t* lab_dev, int n, int h, int w, float threshold, uint8_t* out_dev);

/* ---- seeded minimax flood, airway mask (not in the reference, which leaves the trachea and the bronchi out of its labels) ----------
 * lm_seed_cost_dev: vol [n][h][w] of `dtype` and 1 .. 64 seeds (HOST int64 raster indices (z * h + y) * w + x) -> cost_out int16
 * [n][h][w], the smallest threshold at which each voxel connects to a seed.  DEFINITIONS, all in integers:
 *   Value.  hu = the statistics' HU value of the voxel (integers as they are; floats rint, half to even, saturated to int32; int64
 *     saturated to int32; NaN flagged), x = max(hu, -1024).
 *   Passable.  A voxel is passable iff it is not NaN and hu <= cap_hu, -1023 <= cap_hu <= 3071.  Nothing exists outside the volume.
 *   Cost.  cost[v] = the minimum, over the 6-connected paths of passable voxels from any seed to v, of the maximum x on the path, both
 *     ends included; 32767 where no such path exists (an impassable voxel; an impassable seed contributes nothing).  A duplicate seed
 *     counts once in the result and twice in info[2].
 *   curve_host (HOST) int64 [cap_hu + 1025]: curve[k] = the number of voxels with cost == -1024 + k.  The region a threshold T grows
 *     from the seeds is {cost <= T}, and its size the cumulative curve.
 *   info_host (HOST) = rounds run, voxels reached (the sum of the curve), passable seeds, converged (0 / 1).
 * The cost is the unique fixed point of c[v] = max(x[v], min(c[v], min over the six neighbours u of c[u])) from c = x at the seeds and
 * 32767 elsewhere; every intermediate value is the cost of a real path, so relaxations may run in any order and read neighbours in any
 * state: the result does not depend on the schedule.  The volume is cut into bricks of 8 x 8 x 32 voxels; a round relaxes every
 * brick of its work-list to its local fixed point in LDS and lists the face neighbours of the faces on which a voxel fell for the
 * next round; the host launches a round, reads back one counter and stops on zero.  After round j + 1 every voxel
 * with an optimal path that crosses brick faces j times is final, and a simple path crosses fewer faces than the volume has voxels:
 * a run with max_rounds >= n * h * w + 1 always converges.  When max_rounds is spent before the fixed point: LM_ERR_INVALID, "max_rounds",
 * info_host = rounds, 0, passable seeds, 0, and cost_out_dev is unspecified.  A seed outside the volume: LM_ERR_INVALID.  dtype
 * LM_I16, LM_I32, LM_I64, LM_F32 or LM_F64.  Limits are lm_edt_dev's.  The input is not written; cost_out_dev must not be vol_dev.
 * Workspace (grow-only, kept by the engine): one int16 volume of the input's size and 12 bytes per brick.  Returns once curve_host
 * and info_host are known.  lm_seed_cost_bricks: the number of bricks of a volume and the brick's extents (z, y, x).
 *
 * lm_airway_mask_dev: cost int16 [n][h][w] (lm_seed_cost_dev's), optionally lab u8 [n][h][w] -> mask_out u8 [n][h][w] = 1 where
 * cost <= threshold, else 0 (-32768 <= threshold <= 32766: an unreached voxel never enters), and counts_host (HOST) int64 [256]:
 * counts[L] = the mask voxels with lab == L, all of them in entry 0 when lab_dev is NULL.  mask_out_dev must not be an input.  Limits
 * are lm_edt_dev's.  Returns once counts_host is known. */
#define LM_SEED_MAX 64
int lm_seed_cost_dev(lm_engine* e, const void* vol_dev, int dtype, int n, int h, int w, const int64_t* seeds, int n_seeds, int cap_hu,
                     int64_t max_rounds, int16_t* cost_out_dev, int64_t* curve_host, int64_t info_host[4]);
int lm_seed_cost_bricks(int n, int h, int w, int64_t* bricks_out, int32_t brick_out[3]);
int lm_airway_mask_dev(lm_engine* e, const int16_t* cost_dev, const uint8_t* lab_dev /* or NULL */, int n, int h, int w, int threshold,
                       uint8_t* mask_out_dev, int64_t counts_host[256]);

/* ---- test seam: engine workspaces --------------------------------------------------------------------------------------------
 * The engine keeps grow-only workspaces between calls; no entry point may depend on what an earlier call left in them.
 * lm_debug_fill_workspaces waits for the engine's streams, sets every scratch workspace the engine currently owns (device and pinned
 * host, the whole capacity) to `byte` (0 .. 255), waits again and reports the bytes written in *bytes_filled (0: nothing allocated
 * yet).  Exempt, because their contents ARE state between calls: the resident volumes of lm_pipe_* (between lm_pipe_upload and
 * lm_pipe_download), and the slab state of lm_slab_* -- while an exchange is open (lm_slab_begin without the last lm_slab_step) the
 * call returns LM_ERR_INVALID and touches nothing.  A pending plan of lm_mesh_plan_dev is dropped (the next lm_mesh_dev plans itself).
 * Model weights are untouched.  Every result after the call must equal, bit for bit, what a new engine returns. */
int lm_debug_fill_workspaces(lm_engine* e, int byte, int64_t* bytes_filled);

/* What the last lm_postprocess_dev saw: info[0]=regions, [1]=boundary voxels shipped to the
 * host, [2]=regions processed by the merge loop, [3]=regions merged, [4]=host replay in us. */
/* ---- the same post-processing with the volume's slices spread over `world` ranks (multi-GPU pipeline) ----
 * Every rank holds a contiguous slab lab_slab_dev u8 [n][h][w] = slices [z0, z0+n) of a volume of n_total slices and
 * runs the voxel passes on its slab only; the slabs are tied together by six small exchanges (four with LM_SLAB_GRAPH=1, the region-graph form of the second labelling) the CALLER performs
 * (torch.distributed all_gather over RCCL; csrc/slab_engine.hip describes each).  Protocol, identical on every rank:
 *     lm_slab_begin(...);
 *     do { len = lm_slab_pending(e);                       // int32 words this rank contributes
 *          all-gather len -> lens[world];  stride = max(lens);
 *          lm_slab_emit(e, mine_dev);                       // device buffer of >= len words
 *          all-gather mine_dev (padded to stride) -> gathered_dev [world][stride];
 *     } while (lm_slab_step(e, gathered_dev, stride, lens) == 0);   // 1 = finished: the slab holds the result
 * Requires n >= 1 on every rank.  Result == lm_postprocess_dev on the gathered volume, bit for bit. */
int lm_slab_begin(lm_engine* e, uint8_t* lab_slab_dev, int n, int h, int w, int rank, int world, int z0, int n_total,
                  const int* spare, int n_spare, int skip_below);
int64_t lm_slab_pending(lm_engine* e);
/* 1 when the pending length is the same on every rank by construction (the face-plane exchanges): the caller may skip
 * the all-gather of the lengths for this round. */
int lm_slab_pending_uniform(lm_engine* e);
int lm_slab_emit(lm_engine* e, int32_t* dst_dev);
int lm_slab_step(lm_engine* e, const int32_t* gathered_dev, int64_t stride, const int64_t* lens);

int lm_postprocess_info(lm_engine* e, int64_t info[5]);

/* ---- label fusion (mask.py:228-230): res_l <- fuse(res_l, res_r); returns the spare label -- */
int lm_fuse_dev(lm_engine* e, uint8_t* res_l_dev, const uint8_t* res_r_dev, size_t nvox, int* spare_out);
/* The two halves of lm_fuse_dev for a volume whose slices are spread over several ranks (lungmask_amd/pipeline.py): `spare =
 * res_l.max() + 1` (mask.py:228) is a maximum over the WHOLE volume, so every rank reports the maximum of its slab
 * (lm_label_max_dev), the caller combines them (one small all-gather) and every rank fuses its slab with the agreed value
 * (lm_fuse_spare_dev == mask.py:229-230). */
int lm_label_max_dev(lm_engine* e, const uint8_t* lab_dev, size_t nvox, int* max_out);
int lm_fuse_spare_dev(lm_engine* e, uint8_t* res_l_dev, const uint8_t* res_r_dev, size_t nvox, int spare);

/* ---- the whole hot path: LMInferer.apply on a numpy volume (mask.py:212-232) ---------- */
/* slot: model; fill_slot: fill model for the fused LTRCLobes_R231 mode or -1.
 * vol: [n][h][w] of `dtype` (LM_I16/LM_I32/LM_I64/LM_F32/LM_F64); out: u8 [n][h][w].
 * batch_size, volume_postprocessing: the LMInferer constructor arguments (mask.py:72-82).
 * _dev: both buffers already in HBM, nothing leaves the device.  _host: does the H2D / D2H. */
int lm_apply_dev(lm_engine* e, int slot, int fill_slot, const void* vol_dev, int dtype, int n, int h, int w,
                 int batch_size, int volume_postprocessing, uint8_t* out_dev);
int lm_apply_host(lm_engine* e, int slot, int fill_slot, const void* vol_host, int dtype, int n, int h, int w,
                  int batch_size, int volume_postprocessing, uint8_t* out_host);
/* lm_apply_dev of ONE model that also writes its probability maps (lm_uncrop_probs_dev's semantics) to probs_out_dev [C][n][h][w]
 * of prob_dtype (LM_F32 or LM_F16).  labels_out_dev u8 [n][h][w] (may be NULL) receives exactly what lm_apply_dev returns,
 * post-processing included.  Volume post-processing changes labels only, never probabilities: argmax of the maps may differ from
 * the labels where post-processing removed or filled a region, and where nearest-neighbour and linear resampling disagree.
 * There is no fill model: probabilities of the fused mode are not defined (the reference fuses labels, mask.py:223-232).
 * Each batch's log-softmax is un-cropped on its forward lane's stream right behind the batch (2 x batch x C x 256^2 floats of
 * workspace); when the f16 range guard re-runs the volume on the exact-fp32 kernels, the maps are regenerated by that run. */
int lm_apply_probs_dev(lm_engine* e, int slot, const void* vol_dev, int dtype, int n, int h, int w, int batch_size,
                       int volume_postprocessing, uint8_t* labels_out_dev, int prob_dtype, void* probs_out_dev);

/* lm_apply_host with flags.  LM_APPLY_OUT_SCRATCH: the previous contents of out_host are of no value to the caller (a result
 * array the binding allocated itself, mask.py:210) -- the engine may write it before the call is known to succeed: a helper thread
 * fills it with zeros while the network runs, and only the slab of slices x image rows that carries a label is copied back (one
 * strided device-to-host copy).  Without the flag (== lm_apply_host) out_host is only written by the final copy of a successful
 * call.  The labels are the same either way. */
#define LM_APPLY_OUT_SCRATCH 1u
int lm_apply_host_ex(lm_engine* e, int slot, int fill_slot, const void* vol_host, int dtype, int n, int h, int w,
                     int batch_size, int volume_postprocessing, uint8_t* out_host, unsigned flags);

/* ---- volumes QUEUED through one engine ("multi-volume queueing"; the reference's apply is one blocking call
 *      per volume, mask.py:212-232) -------------------------------------------------------------------------------------------
 * lm_apply_host crosses the host boundary inside the call: copy-in before the first kernel, copy-back behind the last.  With a
 * stream of volumes both can run BESIDE the hot path of the neighbouring volumes.  The engine holds two resident input buffers and
 * two result buffers (k = 0, 1); volume i uses k = i % 2:
 *     lm_pipe_upload(e, k, vol_host, bytes)      copy-in on a stream of its own (returns when a pageable source has been staged:
 *                                                call it from a thread of its own, ahead of the volume's turn);
 *     lm_pipe_apply(e, k, slot, ...)             == lm_apply_dev on buffer k: waits ON THE DEVICE for the copy-in of k and for the
 *                                                copy-back of the volume that used result buffer k before (two volumes earlier);
 *     lm_pipe_download(e, k, out_host, bytes)    enqueues the copy-back on a third stream behind the hot path, returns at once;
 *     lm_pipe_wait(e, k)                         blocks until that copy-back has arrived;
 *     lm_pipe_query(e, k)                        1: that copy-back has arrived (or none is enqueued), 0: not yet; never blocks.
 * Every dependency between the four streams is on the DEVICE: the copy into input buffer k waits for the hot path of the volume
 * that read it last, the hot path for its copy-in and for the copy-back out of result buffer k, the copy-back for its hot path.
 * What the caller still owes:
 *   - lm_pipe_upload(k) of volume i + 2 is CALLED only after lm_pipe_apply(k) of volume i has returned (the engine learns of that
 *     hot path only then -- its return says nothing about the device, which may not have started);
 *   - vol_host: a PAGEABLE source is staged inside lm_pipe_upload and is the caller's again when the call returns; a PAGE-LOCKED
 *     source (lm_host_alloc, a registered range) is read by the copy itself, which may run long after the call has returned (it
 *     waits for the buffer's last reader): it stays unchanged and alive until the copy-in has run, e.g. until lm_pipe_wait or a
 *     positive lm_pipe_query of that volume's copy-back;
 *   - out_host stays alive until lm_pipe_wait.
 * Threads: lm_pipe_upload may run on another thread than lm_pipe_apply / lm_pipe_download / lm_pipe_wait (it shares nothing with
 * them but the order above).  lm_pipe_query(k) may be called from any further thread at any time, except concurrently with
 * lm_pipe_download of the SAME k: it reads only that buffer's copy-back event and its validity flag.
 * lungmask_amd.LMInferer.apply_async is the binding.  Labels == lm_apply_host. */
int lm_pipe_upload(lm_engine* e, int k, const void* vol_host, size_t bytes);
int lm_pipe_apply(lm_engine* e, int k, int slot, int fill_slot, int dtype, int n, int h, int w, int batch_size, int volume_postprocessing);
int lm_pipe_download(lm_engine* e, int k, uint8_t* out_host, size_t bytes);
int lm_pipe_wait(lm_engine* e, int k);
int lm_pipe_query(lm_engine* e, int k);

/* The batch loop of mask.py:173-187 in one call: n slices in batches of batch_size.  With two forward
 * lanes (default; lm_set_streams(e, 1) disables) consecutive batches alternate between two HIP streams and
 * workspaces so that one batch's kernel tails are filled by the next batch's work; results are identical. */
int lm_forward_batches_dev(lm_engine* e, int slot, const float* x_dev, int n, int h, int w, int batch_size,
                           uint8_t* labels_dev);
int lm_set_streams(lm_engine* e, int n);
/* Producer/consumer fusions of the split-f16 forward (default 11 = bits 0 and 3; A/B and test hook).
 * bit 0: down_path.0's first conv (Cin = 1, resunet.py:93-95) computed inside the loader of its second conv -- the stand-alone
 *        kernel's operation order: bit-identical results;
 * bit 1: reserved (the decoder's bilinear x2, resunet.py:131-133, inside the loader of the block's first conv: ruled out by
 *        measurement, DESIGN.md 3.6 -- setting it changes nothing);
 * bit 2: split-K of the 16 x 16 / 32 x 32 decoder 1x1 convs (parts added in a fixed order: deterministic, last bits differ from
 *        the single chain); measured slower than the single chain, hence off by default;
 * bit 3: the head (last 1x1 conv + log-softmax + argmax, resunet.py:69-70, mask.py:184-186) inside the last conv's epilogue, on the
 *        conv's fp32 results instead of the stored 22-bit hi/lo tensor: log-probabilities differ in the last bits, labels on
 *        near-tie pixels only. */
int lm_set_fusion(lm_engine* e, int mask);

/* Per-kernel timing of the launches since the last reset (HIP events on the launching stream).
 * lm_profile_enable(e, on): 0 off; 1 every kernel; 2 every kernel, one entry per conv layer shape;
 * 3 the dominant kernel (conv3x3) only -- a third of the events, for timed regions (the events of mode 1 cost ~1 %).
 * lm_profile_read returns the number of distinct kernel kinds and fills up to `cap` entries. */
typedef struct lm_kernel_stat {
    char name[48];
    int64_t launches;
    double total_ms;
    double flops; /* algorithmic FLOPs of those launches (0 for non-GEMM kernels) */
    double bytes; /* algorithmic HBM bytes of those launches */
} lm_kernel_stat;
int lm_profile_enable(lm_engine* e, int on);
int lm_profile_reset(lm_engine* e);
int lm_profile_read(lm_engine* e, lm_kernel_stat* out, int cap);
/* Timeline of the launches since the last reset (lm_profile_enable(e, 4): per-layer names + start/end of every launch in
 * milliseconds since the first recorded launch, with the forward lane it ran on): what runs beside what when two lanes are on. */
typedef struct lm_launch_span {
    char name[48];
    int lane;
    double start_ms, end_ms;
} lm_launch_span;
int lm_profile_timeline(lm_engine* e, lm_launch_span* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* LUNGMASK_HIP_H */
