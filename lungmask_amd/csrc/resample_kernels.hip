// Resampling onto any grid (lm_spline_prefilter_dev, lm_resample_dev; include/lungmask_hip.h): the source sampled at an affine map of
// the output index -- nearest, trilinear, cubic B-spline, and the label-linear argmax.  All arithmetic is the header's, float64
// without contraction.  Everything here is bandwidth-bound.
//
// The gathers (rs_nearest_kernel, rs_linear_kernel, rs_cubic_kernel, rs_label_linear_kernel): one thread per output voxel, x fastest,
// so that a wave's store is one contiguous run.  With a map near an axis permutation the taps of neighbouring outputs overlap and
// come from L2: the cubic gather reads 64 float64 coefficients per voxel, a 4 x 4 x 4 block that it shares with its neighbours.
// The tap indices and weights of the three axes are kept in fully unrolled registers (no scratch).
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
#include <cstring>
#include <type_traits>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kRS = 256;       // threads of a gather / line-pass workgroup
constexpr int kXT = 64;        // x pass: lines per band and columns per tile
constexpr int kXP = kXT + 1;   // padded tile row
constexpr int kStart = 37;     // terms of the causal start sum: |z|^37 < 2^-70

struct RsMap {
    double A[9], b[3];
    int e0, e1, e2;  // source extents
    int N1, N2;      // output rows per slice, voxels per row
    unsigned total;  // output voxels
};

template <class OUT>
__device__ __forceinline__ OUT rs_out(double v);
template <>
__device__ __forceinline__ float rs_out<float>(double v) { return (float)v; }
template <>
__device__ __forceinline__ uint16_t rs_out<uint16_t>(double v) {  // (half)(float)v, round to nearest even both times
#ifdef LM_EMU_BUILD
    return lm_f2h((float)v);
#else
    return __builtin_bit_cast(uint16_t, lm_f2h((float)v));
#endif
}
template <>
__device__ __forceinline__ int16_t rs_out<int16_t>(double v) {  // rint (half to even), saturated
    const double r = rint(v);
    return r >= 32767.0 ? (int16_t)32767 : (r <= -32768.0 ? (int16_t)-32768 : (int16_t)(int)r);
}

// Steps 1 and 2 of the definition for output voxel `o`: the coordinate, the inside test and the nearest index.
__device__ __forceinline__ bool rs_coord(const RsMap& m, unsigned o, double c[3], int j[3]) {
    const unsigned row = o / (unsigned)m.N2;
    const double o2 = (double)(o - row * (unsigned)m.N2);
    const unsigned sl = row / (unsigned)m.N1;
    const double o1 = (double)(row - sl * (unsigned)m.N1), o0 = (double)sl;
    const int e[3] = {m.e0, m.e1, m.e2};
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = ((m.A[3 * i] * o0 + m.A[3 * i + 1] * o1) + m.A[3 * i + 2] * o2) + m.b[i];
        const double t = floor(c[i] + 0.5);
        const bool in = t >= 0.0 && t < (double)e[i];  // (false for a NaN)
        j[i] = in ? (int)t : 0;
        inside = inside && in;
    }
    return inside;
}

// the linear taps of the clamped coordinate along an axis of extent e
__device__ __forceinline__ void rs_taps2(double c, int e, int& i0, int& i1, double& f) {
    const double last = (double)(e - 1);
    c = c > 0.0 ? c : 0.0;
    c = c < last ? c : last;
    const double fl = floor(c);
    i0 = (int)fl;
    f = c - fl;
    i1 = i0 + 1 < e - 1 ? i0 + 1 : e - 1;
}

__device__ __forceinline__ double rs_lerp(double a, double b, double f) { return a * (1.0 - f) + b * f; }

// m(k) of the header for k >= -1: the mirror index with period 2e - 2
__device__ __forceinline__ int rs_mirror(int k, int e) {
    if (e == 1) return 0;
    const int P = 2 * e - 2;
    int m = k % P;
    m = m < 0 ? m + P : m;
    return m >= e ? P - m : m;
}

// the four cubic taps and weights of the clamped coordinate
__device__ __forceinline__ void rs_taps4(double c, int e, int idx[4], double w[4]) {
    const double last = (double)(e - 1);
    c = c > 0.0 ? c : 0.0;
    c = c < last ? c : last;
    const double fl = floor(c);
    const int i0 = (int)fl;
    const double f = c - fl, g = 1.0 - f;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = rs_mirror(i0 - 1 + k, e);
    w[0] = ((g * g) * g) / 6.0;
    w[1] = 2.0 / 3.0 - ((f * f) * (2.0 - f)) / 2.0;
    w[2] = 2.0 / 3.0 - ((g * g) * (1.0 + f)) / 2.0;
    w[3] = ((f * f) * f) / 6.0;
}

// U: an unsigned integer of the element's size -- the raw value goes through untouched; fill_bits: the fill in the source's dtype
template <class U>
__global__ __launch_bounds__(kRS) void rs_nearest_kernel(RsMap m, const U* __restrict__ src, U fill_bits, U* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kRS + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    const bool inside = rs_coord(m, o, c, j);
    out[o] = inside ? src[((size_t)j[0] * m.e1 + j[1]) * m.e2 + j[2]] : fill_bits;
}

template <class T, class OUT>
__global__ __launch_bounds__(kRS) void rs_linear_kernel(RsMap m, const T* __restrict__ src, double fill, OUT* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kRS + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    double v = fill;
    if (rs_coord(m, o, c, j)) {
        int z0, z1, y0, y1, x0, x1;
        double fz, fy, fx;
        rs_taps2(c[0], m.e0, z0, z1, fz);
        rs_taps2(c[1], m.e1, y0, y1, fy);
        rs_taps2(c[2], m.e2, x0, x1, fx);
        const T* __restrict__ r00 = src + ((size_t)z0 * m.e1 + y0) * m.e2;
        const T* __restrict__ r01 = src + ((size_t)z0 * m.e1 + y1) * m.e2;
        const T* __restrict__ r10 = src + ((size_t)z1 * m.e1 + y0) * m.e2;
        const T* __restrict__ r11 = src + ((size_t)z1 * m.e1 + y1) * m.e2;
        const double v00 = rs_lerp((double)r00[x0], (double)r00[x1], fx);
        const double v01 = rs_lerp((double)r01[x0], (double)r01[x1], fx);
        const double v10 = rs_lerp((double)r10[x0], (double)r10[x1], fx);
        const double v11 = rs_lerp((double)r11[x0], (double)r11[x1], fx);
        v = rs_lerp(rs_lerp(v00, v01, fy), rs_lerp(v10, v11, fy), fz);
    }
    out[o] = rs_out<OUT>(v);
}

template <class OUT>
__global__ __launch_bounds__(kRS) void rs_cubic_kernel(RsMap m, const double* __restrict__ coef, double fill, OUT* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kRS + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    double v = fill;
    if (rs_coord(m, o, c, j)) {
        int iz[4], iy[4], ix[4];
        double wz[4], wy[4], wx[4];
        rs_taps4(c[0], m.e0, iz, wz);
        rs_taps4(c[1], m.e1, iy, wy);
        rs_taps4(c[2], m.e2, ix, wx);
        double vz = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double vy = 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double* __restrict__ row = coef + ((size_t)iz[a] * m.e1 + iy[b]) * m.e2;
                double vx = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) vx = vx + wx[k] * row[ix[k]];
                vy = vy + wy[b] * vx;
            }
            vz = vz + wz[a] * vy;
        }
        v = vz;
    }
    out[o] = rs_out<OUT>(v);
}

__global__ __launch_bounds__(kRS) void rs_label_linear_kernel(RsMap m, const uint8_t* __restrict__ src, uint8_t fill, uint8_t* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kRS + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    uint8_t res = fill;
    if (rs_coord(m, o, c, j)) {
        int z0, z1, y0, y1, x0, x1;
        double fz, fy, fx;
        rs_taps2(c[0], m.e0, z0, z1, fz);
        rs_taps2(c[1], m.e1, y0, y1, fy);
        rs_taps2(c[2], m.e2, x0, x1, fx);
        const double wz[2] = {1.0 - fz, fz}, wy[2] = {1.0 - fy, fy}, wx[2] = {1.0 - fx, fx};
        const int zi[2] = {z0, z1}, yi[2] = {y0, y1}, xi[2] = {x0, x1};
        int lab[8];
        double wgt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {  // z-major corner order
            const int a = k >> 2, b = (k >> 1) & 1, d = k & 1;
            lab[k] = src[((size_t)zi[a] * m.e1 + yi[b]) * m.e2 + xi[d]];
            wgt[k] = (wz[a] * wy[b]) * wx[d];
        }
        int best = 256;
        double best_sum = -1.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s = lab[q] == lab[k] ? s + wgt[q] : s;  // the label's sum, in corner order
            const bool better = s > best_sum || (s == best_sum && lab[k] < best);
            best = better ? lab[k] : best;
            best_sum = better ? s : best_sum;
        }
        res = (uint8_t)best;
    }
    out[o] = res;
}

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
        cp = cp + zk * s[(size_t)rs_mirror(k, L) * stride];
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
                    cp = cp + zk * my[rs_mirror(k, W)];
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

// the fill of LM_RS_NEAREST in the source's dtype, as the bits of an unsigned integer of its size
uint64_t nearest_fill_bits(int dtype, double fill) {
    uint64_t bits = 0;
    const double r = std::rint(fill);
    switch (dtype) {
        case LM_U8: bits = (uint8_t)fill; break;  // (0 <= fill <= 255: checked by the caller)
        case LM_I16: {
            const int16_t v = r >= 32767.0 ? (int16_t)32767 : (r <= -32768.0 ? (int16_t)-32768 : (int16_t)(int)r);
            std::memcpy(&bits, &v, 2);
            break;
        }
        case LM_I32: {
            const int32_t v = r >= 2147483647.0 ? INT32_MAX : (r <= -2147483648.0 ? INT32_MIN : (int32_t)r);
            std::memcpy(&bits, &v, 4);
            break;
        }
        case LM_I64: {
            const int64_t v = r >= 9223372036854775808.0 ? INT64_MAX : (r <= -9223372036854775808.0 ? INT64_MIN : (int64_t)r);
            std::memcpy(&bits, &v, 8);
            break;
        }
        case LM_F32: {
            const float v = (float)fill;
            std::memcpy(&bits, &v, 4);
            break;
        }
        default: std::memcpy(&bits, &fill, 8);
    }
    return bits;
}

template <class T>
hipError_t launch_linear(const RsMap& m, const void* src, int out_dtype, double fill, void* out, hipStream_t s) {
    const dim3 grid(blocks_for(m.total)), block(kRS);
    if (out_dtype == LM_F32) LM_LAUNCH((rs_linear_kernel<T, float>), grid, block, 0, s, m, static_cast<const T*>(src), fill, static_cast<float*>(out));
    else if (out_dtype == LM_F16)
        LM_LAUNCH((rs_linear_kernel<T, uint16_t>), grid, block, 0, s, m, static_cast<const T*>(src), fill, static_cast<uint16_t*>(out));
    else if constexpr (std::is_integral<T>::value)
        LM_LAUNCH((rs_linear_kernel<T, int16_t>), grid, block, 0, s, m, static_cast<const T*>(src), fill, static_cast<int16_t*>(out));
    return hipGetLastError();
}

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
    const double nsrc = (double)n * h * w, nout = (double)m.total;
    const dim3 grid(blocks_for(m.total)), block(kRS);
    hipError_t err = hipSuccess;
    if (p.mode == LM_RS_NEAREST) {
        const int esz = dtype == LM_U8 ? 1 : dtype_bytes(dtype);
        const uint64_t fb = nearest_fill_bits(dtype, p.fill);
        ProfScope ps(e, "rs_nearest", (nsrc + nout) * esz);
        if (esz == 1) LM_LAUNCH((rs_nearest_kernel<uint8_t>), grid, block, 0, e->stream, m, static_cast<const uint8_t*>(src), (uint8_t)fb, static_cast<uint8_t*>(out));
        else if (esz == 2)
            LM_LAUNCH((rs_nearest_kernel<uint16_t>), grid, block, 0, e->stream, m, static_cast<const uint16_t*>(src), (uint16_t)fb, static_cast<uint16_t*>(out));
        else if (esz == 4)
            LM_LAUNCH((rs_nearest_kernel<uint32_t>), grid, block, 0, e->stream, m, static_cast<const uint32_t*>(src), (uint32_t)fb, static_cast<uint32_t*>(out));
        else
            LM_LAUNCH((rs_nearest_kernel<uint64_t>), grid, block, 0, e->stream, m, static_cast<const uint64_t*>(src), fb, static_cast<uint64_t*>(out));
        err = hipGetLastError();
    } else if (p.mode == LM_RS_LABEL_LINEAR) {
        ProfScope ps(e, "rs_label_linear", nsrc + nout);
        LM_LAUNCH(rs_label_linear_kernel, grid, block, 0, e->stream, m, static_cast<const uint8_t*>(src), (uint8_t)p.fill, static_cast<uint8_t*>(out));
        err = hipGetLastError();
    } else if (p.mode == LM_RS_LINEAR) {
        const int osz = p.out_dtype == LM_F32 ? 4 : 2;
        ProfScope ps(e, "rs_linear", nsrc * dtype_bytes(dtype) + nout * osz);
        switch (dtype) {
            case LM_I16: err = launch_linear<int16_t>(m, src, p.out_dtype, p.fill, out, e->stream); break;
            case LM_I32: err = launch_linear<int32_t>(m, src, p.out_dtype, p.fill, out, e->stream); break;
            case LM_I64: err = launch_linear<int64_t>(m, src, p.out_dtype, p.fill, out, e->stream); break;
            case LM_F32: err = launch_linear<float>(m, src, p.out_dtype, p.fill, out, e->stream); break;
            default: err = launch_linear<double>(m, src, p.out_dtype, p.fill, out, e->stream);
        }
    } else {
        LM_TRY(e->resample.coef.reserve((size_t)n * h * w * sizeof(double)));
        double* coef = e->resample.coef.as<double>();
        LM_TRY(spline_prefilter(e, src, dtype, n, h, w, coef));
        const int osz = p.out_dtype == LM_F32 ? 4 : 2;
        ProfScope ps(e, "rs_cubic", nsrc * 8.0 + nout * osz);
        if (p.out_dtype == LM_F32) LM_LAUNCH((rs_cubic_kernel<float>), grid, block, 0, e->stream, m, coef, p.fill, static_cast<float*>(out));
        else if (p.out_dtype == LM_F16) LM_LAUNCH((rs_cubic_kernel<uint16_t>), grid, block, 0, e->stream, m, coef, p.fill, static_cast<uint16_t*>(out));
        else LM_LAUNCH((rs_cubic_kernel<int16_t>), grid, block, 0, e->stream, m, coef, p.fill, static_cast<int16_t*>(out));
        err = hipGetLastError();
    }
    LM_K(err);
    return LM_OK;
}

}  // namespace lm
