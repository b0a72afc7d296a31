// Resampling onto any grid (lm_spline_prefilter_dev, lm_resample_dev; include/lungmask_hip.h): the source sampled at an affine map of
// the output index -- nearest, trilinear, cubic B-spline, and the label-linear argmax.  All arithmetic is the header's, float64
// without contraction.  Everything here is bandwidth-bound.
//
// The gathers are sample_common.h's (gather_nearest_kernel, gather_linear_kernel, gather_cubic_kernel, gather_label_linear_kernel),
// instantiated here with RsMap: the coordinate is the affine map of the output index.  With a map near an axis permutation the taps
// of neighbouring outputs overlap and come from L2: the cubic gather reads 64 float64 coefficients per voxel, a 4 x 4 x 4 block that
// it shares with its neighbours.
//
// The prefilter works in place in the float64 coefficient volume (rs_convert_kernel fills it), one axis after the other.
//   y and z (rs_prefilter_lines_kernel): a lane owns one line and steps along the axis; consecutive lanes sit on consecutive x, so
//   every step of a wave is one contiguous 512-byte run.
//   x (rs_prefilter_x_kernel): a line runs along the fastest axis, so one lane per line would stride by w.  A workgroup of one wave
//   takes a band of kXT = 64 consecutive lines and moves tiles of 64 lines x kXT = 64 columns through LDS: a tile row is loaded and
//   stored by the whole wave (512 contiguous bytes), then lane l runs the recursion along row l of the tile.  Rows are padded by one
//   float64 (kXT + 1 = 65 per row), so the lanes' column reads fall on different banks.  LDS: 64 * 65 * 8 = 33280 bytes.  The causal
//   sweep walks the tiles in ascending order and carries cp in a register; the 37-term start sum reads columns 0 .. 36 at the most,
//   which all lie in tile 0.  The anticausal sweep reads cp back in descending tile order and carries c; its start value needs the
//   last two cp of the line, which the causal sweep leaves in registers.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kRS = 256;       // threads of a convert / line-pass workgroup
constexpr int kXT = 64;        // x pass: lines per band and columns per tile
constexpr int kXP = kXT + 1;   // padded tile row
constexpr int kStart = 37;     // terms of the causal start sum: |z|^37 < 2^-70

struct RsMap {
    double A[9], b[3];
    int e0, e1, e2;  // source extents
    int N1, N2;      // output rows per slice, voxels per row
    unsigned total;  // output voxels
    __device__ __forceinline__ bool coord(unsigned o, double c[3], int j[3]) const {
        unsigned o0, o1, o2;
        index_split(o, (unsigned)N1, (unsigned)N2, o0, o1, o2);
        return affine_coord(A, b, (double)o0, (double)o1, (double)o2, e0, e1, e2, c, j);
    }
};

template <class T>
__global__ __launch_bounds__(kRS) void rs_convert_kernel(const T* __restrict__ src, unsigned total, double* __restrict__ out) {
    const unsigned v = blockIdx.x * (unsigned)kRS + threadIdx.x;
    if (v < total) out[v] = (double)src[v];
}

// The prefilter along an axis that is not the fastest, in place.  `cols` contiguous columns (consecutive lanes), lines of L
// elements `stride` apart, n_outer groups of them `outer` apart (y pass: cols = w, stride = w, one group per slice; z pass:
// cols = h * w, stride = h * w, one group).
__global__ __launch_bounds__(kRS) void rs_prefilter_lines_kernel(double* __restrict__ coef, int L, size_t stride, unsigned cols, size_t outer,
                                                               unsigned n_lines, double z) {
    const unsigned line = blockIdx.x * (unsigned)kRS + threadIdx.x;
    if (line >= n_lines) return;
    const unsigned g = line / cols;
    double* __restrict__ s = coef + (size_t)g * outer + (size_t)(line - g * cols);
    double cp = 0.0, zk = 1.0;
    for (int k = 0; k < kStart; ++k) {
        cp = cp + zk * s[(size_t)mirror(k, L) * stride];
        zk = zk * z;
    }
    double prev = cp;
    s[0] = cp;
    for (int i = 1; i < L; ++i) {
        prev = cp;
        cp = s[(size_t)i * stride] + z * cp;
        s[(size_t)i * stride] = cp;
    }
    double c = (z / (z * z - 1.0)) * (cp + z * prev);  // (prev = cp[L - 2]: L >= 2)
    s[(size_t)(L - 1) * stride] = 6.0 * c;
    for (int i = L - 2; i >= 0; --i) {
        c = z * (c - s[(size_t)i * stride]);
        s[(size_t)i * stride] = 6.0 * c;
    }
}

// The prefilter along x, in place: one wave per band of kXT lines of W elements (see the head of the file).
__global__ __launch_bounds__(kXT) void rs_prefilter_x_kernel(double* __restrict__ coef, int W, unsigned n_lines, double z) {
    __shared__ double tile[kXT * kXP];  // 33280 bytes
    const int lane = threadIdx.x;
    const unsigned line0 = blockIdx.x * (unsigned)kXT;
    const int rows = (int)min((unsigned)kXT, n_lines - line0);
    double* __restrict__ band = coef + (size_t)line0 * W;
    const int tiles = (W + kXT - 1) / kXT;
    const bool mine = lane < rows;
    double* __restrict__ my = tile + lane * kXP;
    double cp = 0.0, prev = 0.0;
    for (int t = 0; t < tiles; ++t) {
        const int x0 = t * kXT, cw = min(kXT, W - x0);
        if (lane < cw)
            for (int r = 0; r < rows; ++r) tile[r * kXP + lane] = band[(size_t)r * W + x0 + lane];
        __syncthreads();
        if (mine) {
            int j = 0;
            if (t == 0) {
                double zk = 1.0;
                for (int k = 0; k < kStart; ++k) {
                    cp = cp + zk * my[mirror(k, W)];
                    zk = zk * z;
                }
                prev = cp;
                my[0] = cp;
                j = 1;
            }
            for (; j < cw; ++j) {
                prev = cp;
                cp = my[j] + z * cp;
                my[j] = cp;
            }
        }
        __syncthreads();
        if (lane < cw)
            for (int r = 0; r < rows; ++r) band[(size_t)r * W + x0 + lane] = tile[r * kXP + lane];
        __syncthreads();
    }
    double c = (z / (z * z - 1.0)) * (cp + z * prev);  // (prev = cp[W - 2]: W >= 2)
    for (int t = tiles - 1; t >= 0; --t) {
        const int x0 = t * kXT, cw = min(kXT, W - x0);
        if (lane < cw)
            for (int r = 0; r < rows; ++r) tile[r * kXP + lane] = band[(size_t)r * W + x0 + lane];
        __syncthreads();
        if (mine) {
            int j = cw - 1;
            if (t == tiles - 1) {
                my[j] = 6.0 * c;
                --j;
            }
            for (; j >= 0; --j) {
                c = z * (c - my[j]);
                my[j] = 6.0 * c;
            }
        }
        __syncthreads();
        if (lane < cw)
            for (int r = 0; r < rows; ++r) band[(size_t)r * W + x0 + lane] = tile[r * kXP + lane];
        __syncthreads();
    }
}

inline unsigned blocks_for(unsigned total) { return (total + (unsigned)kRS - 1u) / (unsigned)kRS; }

template <class T>
hipError_t launch_convert(const void* src, unsigned total, double* out, hipStream_t s) {
    LM_LAUNCH((rs_convert_kernel<T>), dim3(blocks_for(total)), dim3(kRS), 0, s, static_cast<const T*>(src), total, out);
    return hipGetLastError();
}

}  // namespace

int spline_prefilter(lm_engine* e, const void* vol, int dtype, int n, int h, int w, double* coef) {
    const unsigned total = (unsigned)((size_t)n * h * w);
    const double nbytes = (double)total * 8.0;
    const double z = std::sqrt(3.0) - 2.0;
    {
        ProfScope ps(e, "rs_convert", (double)total * dtype_bytes(dtype) + nbytes);
        hipError_t err;
        switch (dtype) {
            case LM_I16: err = launch_convert<int16_t>(vol, total, coef, e->stream); break;
            case LM_I32: err = launch_convert<int32_t>(vol, total, coef, e->stream); break;
            case LM_I64: err = launch_convert<int64_t>(vol, total, coef, e->stream); break;
            case LM_F32: err = launch_convert<float>(vol, total, coef, e->stream); break;
            default: err = launch_convert<double>(vol, total, coef, e->stream);
        }
        LM_K(err);
    }
    if (w > 1) {  // every pass reads and writes the volume twice (cp, then c)
        ProfScope ps(e, "rs_prefilter_x", 4.0 * nbytes);
        const unsigned lines = (unsigned)n * (unsigned)h;
        LM_LAUNCH(rs_prefilter_x_kernel, dim3((lines + kXT - 1) / kXT), dim3(kXT), 0, e->stream, coef, w, lines, z);
        LM_K(hipGetLastError());
    }
    if (h > 1) {
        ProfScope ps(e, "rs_prefilter_y", 4.0 * nbytes);
        const unsigned lines = (unsigned)n * (unsigned)w;
        LM_LAUNCH(rs_prefilter_lines_kernel, dim3(blocks_for(lines)), dim3(kRS), 0, e->stream, coef, h, (size_t)w, (unsigned)w, (size_t)h * w, lines, z);
        LM_K(hipGetLastError());
    }
    if (n > 1) {
        ProfScope ps(e, "rs_prefilter_z", 4.0 * nbytes);
        const unsigned lines = (unsigned)h * (unsigned)w;
        LM_LAUNCH(rs_prefilter_lines_kernel, dim3(blocks_for(lines)), dim3(kRS), 0, e->stream, coef, n, (size_t)h * w, lines, (size_t)0, lines, z);
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

int resample(lm_engine* e, const void* src, int dtype, int n, int h, int w, const lm_resample_params& p, void* out) {
    RsMap m;
    for (int i = 0; i < 9; ++i) m.A[i] = p.A[i];
    for (int i = 0; i < 3; ++i) m.b[i] = p.b[i];
    m.e0 = n, m.e1 = h, m.e2 = w;
    m.N1 = p.out_dims[1], m.N2 = p.out_dims[2];
    m.total = (unsigned)((size_t)p.out_dims[0] * p.out_dims[1] * p.out_dims[2]);
    if (p.mode == LM_RS_CUBIC) {  // the cubic gather reads the coefficients
        LM_TRY(e->resample.coef.reserve((size_t)n * h * w * sizeof(double)));
        LM_TRY(spline_prefilter(e, src, dtype, n, h, w, e->resample.coef.as<double>()));
        src = e->resample.coef.as<double>();
    }
    return launch_gather(e, m, "rs_", src, dtype, n, h, w, p, 0.0, out);
}

}  // namespace lm
