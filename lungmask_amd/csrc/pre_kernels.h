// Parameter blocks / launchers of the pre-processing kernels (pre_kernels.hip).
#pragma once
#include "../../include/lungmask_hip.h"
#include "lm_platform.h"

namespace lm {

struct BodyMaskParams {
    const void* vol;  // [N][H][W] of `dtype`
    int dtype;        // LM_I16 / LM_I32 / LM_I64
    int N, H, W;
    int* bbox;       // [N][4] = (r0, c0, r1, c1) half-open, utils.py:102-106
    uint8_t* bmask;  // optional [N][H][W] full-resolution body mask (test seam), else nullptr
};

struct ResampleParams {
    const void* vol;
    int dtype;
    int N, H, W;
    const int* bbox;
    int OH, OW;        // 256 x 256 (mask.py:166)
    int16_t* out_i16;  // optional [N][OH][OW]: utils.preprocess output
    float* out_f32;    // optional [N][OH][OW]: normalised network input (mask.py:167-168,178-181)
};

struct ReshapeParams {
    const uint8_t* mask;  // [N][MH][MW]
    const int* bbox;      // [N][4]
    uint8_t* out;         // [N][H][W]
    int N, MH, MW, H, W;
};

// Probability maps un-cropped to the input volume (the soft counterpart of reshape_mask, utils.py:114-129): for slice z and class c
//   p = expf(logp[z][c])  (f32 [MH][MW]),  out[c][z0 + z][bbox] = ndimage.zoom(p, (box rows, box cols) / (MH, MW), order=1)
//   (fp64 coordinates, weights and accumulation in scipy's order, one rounding to f32),  out[c][z0 + z][elsewhere] = (c == 0)
// i.e. reshape_mask's zero fill = label 0 = background.  Where ndimage.zoom's coordinate lands beyond the last source row / column
// (the rounding of (in - 1) / (out - 1) * o for some box sizes: scipy returns cval 0 in EVERY class there, and reshape_mask label
// 0) the fill is written too, so that the maps sum to one everywhere.  f16 output = (half)(float)v, round to nearest even.
struct UncropParams {
    const float* logp;  // [b][C][MH][MW] log-softmax of slices z0 .. z0 + b - 1
    const int* bbox;    // [b][4] = (r0, c0, r1, c1) of those slices
    void* out;          // [C][n_total][H][W] of out_dtype
    int out_dtype;      // LM_F32 / LM_F16
    int b, C, MH, MW, H, W;
    int n_total, z0;
};

// Axis permutation / flip of a volume (sitk.DICOMOrient at mask.py:156-164,204-208 as an index transform):
// out[i0][i1][i2] = in[base + i0*s0 + i1*s1 + i2*s2], element strides (may be negative).
struct ReorientParams {
    const void* in;
    void* out;
    int elem;  // bytes per element: 1, 2, 4 or 8
    int n0, n1, n2;
    long long s0, s1, s2, base;
};

hipError_t launch_reorient(const ReorientParams& p, hipStream_t stream);
hipError_t launch_bodymask_bbox(const BodyMaskParams& p, hipStream_t stream);
hipError_t launch_resample_norm(const ResampleParams& p, hipStream_t stream);
hipError_t launch_reshape_mask(const ReshapeParams& p, hipStream_t stream);
hipError_t launch_uncrop_probs(const UncropParams& p, hipStream_t stream);
// Extent of the non-zero labels of vol [N][H][W] along the two slow axes: ext[4] = {z0, z1, y0, y1} half-open (z0 >= z1: the
// volume is all zero).  lm_apply_host copies only that slab back to a zero-filled result array (a lung mask is mostly background).
hipError_t launch_label_extent(const uint8_t* vol, int N, int H, int W, int* ext_dev, hipStream_t stream);

}  // namespace lm
