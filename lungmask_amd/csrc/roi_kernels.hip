// Lung ROI (lm_roi_plan_dev, lm_roi_dev; include/lungmask_hip.h): the box of the kept labels, and the masked, cropped, trilinearly
// resampled volume with its nearest-neighbour labels on the same grid.
//
// roi_resample_kernel.  A gather: output voxel o reads 2 x 2 x 2 source voxels around o * step.  A workgroup (256 threads) owns a
// tile of kRows output rows x kTileX output columns of one output slice; a wave takes one row at a time and a lane kVec consecutive
// columns, so that a wave's store is one contiguous run (16 bytes per lane of float32, 8 of float16 / int16, 4 of labels) and each of
// its four tap rows one nearly contiguous source segment of kTileX * step voxels.  What does not depend on x is computed once per
// workgroup: the z taps are uniform, the y taps of the tile's rows sit in LDS (uncrop_probs_kernel's row map); the x taps are
// computed once per lane and kept in registers over the rows.  Consecutive output rows share source rows (step < 2) and the two z
// planes are shared with the next slice's tile: those re-reads come from L2.  The labels are read first; a voxel that the mask blanks
// (most of a lung box is not lung) skips its eight intensity loads.  All arithmetic is the header's, float64 without contraction;
// lerp and the output conversion are lm_resample_dev's (sample_common.h).
//
// With dilate_mm > 0 the inside test reads lm_edt_dev's squared distance to the kept voxels: roi_keepmask_kernel writes keep[lab]
// of the box as a u8 volume, edt() transforms it (every feature lies in the box, so the box's values are the whole volume's).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kRT = 256, kVec = 4, kRows = 16, kTileX = 64 * kVec;

// out[z][y][x] = keep[lab[z0 + z][y0 + y][x0 + x]] != 0 for the box (z0, y0, x0) + (e0, e1, e2) of a volume with rows of W and slices
// of H rows
__global__ __launch_bounds__(kRT) void roi_keepmask_kernel(const uint8_t* __restrict__ lab, int H, int W, int z0, int y0, int x0, int e0,
                                                          int e1, int e2, LabelTable kb, uint8_t* __restrict__ out) {
    __shared__ uint8_t keep[256];
    stage_table(kb, keep, threadIdx.x);
    __syncthreads();
    const int rows = e0 * e1;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int z = row / e1, y = row - z * e1;
        const uint8_t* src = lab + ((size_t)(z0 + z) * H + (y0 + y)) * W + x0;
        uint8_t* dst = out + (size_t)row * e2;
        for (int x = threadIdx.x; x < e2; x += kRT) dst[x] = keep[src[x]];
    }
}

struct RoiParams {
    const void* vol;
    const uint8_t* lab;
    const float* d2;  // [e0][e1][e2] squared distance to the kept voxels, or NULL: the inside test is keep[label]
    int H, W;         // rows per slice / voxels per row of the source volume
    int z0, y0, x0, e0, e1, e2;  // the box
    int N0, N1, N2;              // the output grid
    double s0, s1, s2;           // steps
    LabelTable kb;
    float thr;  // (float)(dilate_mm^2)
    double fill, lo, hi;
    int mask_outside, window;
    int vec;  // N2 % kVec == 0 and both outputs aligned for the vector stores
    int tx, ty;  // tiles along x and y
    void* out;
    uint8_t* out_lab;
};

// the taps of output index o along an axis of extent e: c = min(o * step, e - 1).  Not sample_common.h's taps2: the coordinate comes
// from o * step, has no lower clamp, and the nearest index j is part of the result.
__device__ __forceinline__ void roi_taps(int o, double step, int e, int& i0, int& i1, double& f, int& j) {
    const double last = (double)(e - 1);
    double c = (double)o * step;
    c = c < last ? c : last;
    const double fl = floor(c);
    i0 = (int)fl;
    f = c - fl;
    i1 = i0 + 1 < e - 1 ? i0 + 1 : e - 1;
    const int jn = (int)floor(c + 0.5);
    j = jn < e - 1 ? jn : e - 1;
}

template <class T, class OUT>
__global__ __launch_bounds__(kRT) void roi_resample_kernel(RoiParams p) {
    __shared__ uint8_t keep[256];
    __shared__ double yf[kRows];
    __shared__ int yi0[kRows], yi1[kRows], yj[kRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned tile = blockIdx.x;
    const unsigned per_slice = (unsigned)p.tx * (unsigned)p.ty;
    const int z = (int)(tile / per_slice);
    const unsigned rem = tile - (unsigned)z * per_slice;
    const int ytile = (int)(rem / (unsigned)p.tx), xtile = (int)(rem - (unsigned)ytile * (unsigned)p.tx);
    const int yb = ytile * kRows, rows = min(kRows, p.N1 - yb);
    stage_table(p.kb, keep, tid);
    if (tid < rows) {
        int a, b, j;
        double f;
        roi_taps(yb + tid, p.s1, p.e1, a, b, f, j);
        yi0[tid] = a;
        yi1[tid] = b;
        yf[tid] = f;
        yj[tid] = j;
    }
    int zi0, zi1, zj;
    double fz;
    roi_taps(z, p.s0, p.e0, zi0, zi1, fz, zj);  // (uniform)
    const int xg = xtile * kTileX + lane * kVec;
    int xi0[kVec], xi1[kVec], xj[kVec];
    double fx[kVec];
    bool valid[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        valid[k] = xg + k < p.N2;
        roi_taps(valid[k] ? xg + k : 0, p.s2, p.e2, xi0[k], xi1[k], fx[k], xj[k]);
    }
    __syncthreads();
    if (!valid[0]) return;  // (no barrier below)
    const T* __restrict__ vol = static_cast<const T*>(p.vol);
    const size_t plane = (size_t)p.H * p.W;
    const size_t zoff0 = (size_t)(p.z0 + zi0) * plane, zoff1 = (size_t)(p.z0 + zi1) * plane;
    for (int r = wave; r < rows; r += kRT / 64) {
        const int y = yb + r, j1 = yj[r];
        const uint8_t* __restrict__ lrow = p.lab + ((size_t)(p.z0 + zj) * p.H + (p.y0 + j1)) * p.W + p.x0;
        const float* __restrict__ drow = p.d2 ? p.d2 + ((size_t)zj * p.e1 + j1) * p.e2 : nullptr;
        uint8_t l[kVec];
        bool need[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            l[k] = valid[k] ? lrow[xj[k]] : (uint8_t)0;
            bool inside = true;
            if (p.mask_outside) inside = drow ? (valid[k] && drow[xj[k]] <= p.thr) : keep[l[k]] != 0;
            need[k] = valid[k] && inside;
        }
        const size_t ro0 = (size_t)(p.y0 + yi0[r]) * p.W + p.x0, ro1 = (size_t)(p.y0 + yi1[r]) * p.W + p.x0;
        const T* __restrict__ r00 = vol + zoff0 + ro0;
        const T* __restrict__ r01 = vol + zoff0 + ro1;
        const T* __restrict__ r10 = vol + zoff1 + ro0;
        const T* __restrict__ r11 = vol + zoff1 + ro1;
        const double fy = yf[r];
        OUT o[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            double v = p.fill;
            if (need[k]) {
                const int a = xi0[k], b = xi1[k];
                const double v00 = lerp((double)r00[a], (double)r00[b], fx[k]);
                const double v01 = lerp((double)r01[a], (double)r01[b], fx[k]);
                const double v10 = lerp((double)r10[a], (double)r10[b], fx[k]);
                const double v11 = lerp((double)r11[a], (double)r11[b], fx[k]);
                v = lerp(lerp(v00, v01, fy), lerp(v10, v11, fy), fz);
            }
            if (p.window) {
                v = v < p.lo ? p.lo : (v > p.hi ? p.hi : v);
                v = (v - p.lo) / (p.hi - p.lo);
            }
            o[k] = sample_out<OUT>(v);
        }
        const size_t oo = ((size_t)z * p.N1 + y) * p.N2 + xg;
        OUT* dst = static_cast<OUT*>(p.out) + oo;
        uint8_t* ldst = p.out_lab + oo;
        if (p.vec) {  // (N2 % kVec == 0: the whole group is valid)
            if constexpr (sizeof(OUT) == 4) {
                uint4 q;
                __builtin_memcpy(&q, o, 16);
                *reinterpret_cast<uint4*>(dst) = q;
            } else {
                uint2 q;
                q.x = (unsigned)(uint16_t)o[0] | ((unsigned)(uint16_t)o[1] << 16);
                q.y = (unsigned)(uint16_t)o[2] | ((unsigned)(uint16_t)o[3] << 16);
                *reinterpret_cast<uint2*>(dst) = q;
            }
            *reinterpret_cast<unsigned*>(ldst) = (unsigned)l[0] | ((unsigned)l[1] << 8) | ((unsigned)l[2] << 16) | ((unsigned)l[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < kVec; ++k)
                if (valid[k]) {
                    dst[k] = o[k];
                    ldst[k] = l[k];
                }
        }
    }
}

template <class T, class OUT>
hipError_t launch_roi(const RoiParams& p, unsigned tiles, hipStream_t s) {
    LM_LAUNCH((roi_resample_kernel<T, OUT>), dim3(tiles), dim3(kRT), 0, s, p);
    return hipGetLastError();
}

template <class OUT>
hipError_t launch_roi_dtype(const RoiParams& p, int dtype, unsigned tiles, hipStream_t s) {
    switch (dtype) {
        case LM_I16: return launch_roi<int16_t, OUT>(p, tiles, s);
        case LM_I32: return launch_roi<int32_t, OUT>(p, tiles, s);
        case LM_I64: return launch_roi<int64_t, OUT>(p, tiles, s);
        case LM_F32: return launch_roi<float, OUT>(p, tiles, s);
        default: return launch_roi<double, OUT>(p, tiles, s);
    }
}

int keepmask(lm_engine* e, const uint8_t* lab, int H, int W, const int box[6], const LabelTable& kb, uint8_t* out) {
    const int e0 = box[1] - box[0], e1 = box[3] - box[2], e2 = box[5] - box[4];
    ProfScope ps(e, "roi_keepmask", (double)e0 * e1 * e2 * 2.0);
    LM_LAUNCH(roi_keepmask_kernel, dim3((unsigned)std::min(e0 * e1, 1 << 16)), dim3(kRT), 0, e->stream, lab, H, W, box[0], box[2], box[4], e0, e1,
              e2, kb, out);
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace

int roi_plan(lm_engine* e, const uint8_t* lab, int n, int h, int w, const uint8_t keep[256], int32_t bbox[6], const char* entry) {
    for (int k = 0; k < 6; ++k) bbox[k] = -1;
    bool all = keep[0] == 0;
    for (int l = 1; l < 256 && all; ++l) all = keep[l] != 0;
    if (n > 0) {
        if (all) {  // keep[lab] != 0 is lab != 0: bbox_3D as it stands
            LM_TRY(bbox3d(e, lab, n, h, w, 0, bbox));
        } else {
            LM_TRY(e->roi.feat.reserve((size_t)n * h * w));
            const int whole[6] = {0, n, 0, h, 0, w};
            LM_TRY(keepmask(e, lab, h, w, whole, label_table(keep), e->roi.feat.as<uint8_t>()));
            LM_TRY(bbox3d(e, e->roi.feat.as<uint8_t>(), n, h, w, 0, bbox));
        }
    }
    if (bbox[1] < 0) {
        set_error("%s: no kept voxel (the labels hold none of the values of the keep table)", entry);
        return LM_ERR_INVALID;
    }
    return LM_OK;
}

int roi(lm_engine* e, const void* vol, int dtype, const uint8_t* lab, int n, int h, int w, const lm_roi_params& q, void* out_image,
        uint8_t* out_labels) {
    (void)n;
    RoiParams p;
    std::memset(&p, 0, sizeof p);
    p.vol = vol;
    p.lab = lab;
    p.H = h;
    p.W = w;
    p.z0 = q.bbox[0], p.y0 = q.bbox[2], p.x0 = q.bbox[4];
    p.e0 = q.bbox[1] - q.bbox[0], p.e1 = q.bbox[3] - q.bbox[2], p.e2 = q.bbox[5] - q.bbox[4];
    p.N0 = q.out_dims[0], p.N1 = q.out_dims[1], p.N2 = q.out_dims[2];
    p.s0 = q.step[0], p.s1 = q.step[1], p.s2 = q.step[2];
    p.kb = label_table(q.keep);
    p.fill = q.fill;
    p.lo = q.window_lo, p.hi = q.window_hi;
    p.mask_outside = (q.flags & LM_ROI_MASK_OUTSIDE) ? 1 : 0;
    p.window = (q.flags & LM_ROI_WINDOW) ? 1 : 0;
    p.out = out_image;
    p.out_lab = out_labels;
    const size_t box_vox = (size_t)p.e0 * p.e1 * p.e2;
    if (q.dilate_mm > 0.0 && p.mask_outside) {
        RoiWorkspace& ws = e->roi;
        LM_TRY(ws.feat.reserve(box_vox));
        LM_TRY(ws.d2.reserve(box_vox * sizeof(float)));
        LM_TRY(keepmask(e, lab, h, w, q.bbox, p.kb, ws.feat.as<uint8_t>()));
        LM_TRY(edt(e, ws.feat.as<uint8_t>(), p.e0, p.e1, p.e2, q.spacing, ws.d2.as<float>()));
        p.d2 = ws.d2.as<float>();
        p.thr = (float)(q.dilate_mm * q.dilate_mm);
    }
    const int osz = q.out_dtype == LM_F32 ? 4 : 2;
    p.vec = p.N2 % kVec == 0 && (reinterpret_cast<uintptr_t>(out_image) & (size_t)(kVec * osz - 1)) == 0 &&
            (reinterpret_cast<uintptr_t>(out_labels) & (size_t)(kVec - 1)) == 0;
    p.tx = (p.N2 + kTileX - 1) / kTileX;
    p.ty = (p.N1 + kRows - 1) / kRows;
    const unsigned long long tiles = (unsigned long long)p.tx * p.ty * p.N0;  // (< 2^31: one tile holds at least one output voxel)
    const int esz = dtype_bytes(dtype);
    const double nout = (double)p.N0 * p.N1 * p.N2;
    ProfScope ps(e, "roi_resample", (double)box_vox * (esz + 1.0) + nout * (osz + 1.0));
    hipError_t err;
    if (q.out_dtype == LM_F32) err = launch_roi_dtype<float>(p, dtype, (unsigned)tiles, e->stream);
    else if (q.out_dtype == LM_F16) err = launch_roi_dtype<uint16_t>(p, dtype, (unsigned)tiles, e->stream);
    else if (dtype == LM_I16) err = launch_roi<int16_t, int16_t>(p, (unsigned)tiles, e->stream);
    else if (dtype == LM_I32) err = launch_roi<int32_t, int16_t>(p, (unsigned)tiles, e->stream);
    else err = launch_roi<int64_t, int16_t>(p, (unsigned)tiles, e->stream);
    LM_K(err);
    return LM_OK;
}

}  // namespace lm
