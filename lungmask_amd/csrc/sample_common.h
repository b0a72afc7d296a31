// What the sampling kernels share (resample_, deform_, field_, pair_, register_, roi_kernels.hip): the arithmetic of lm_resample_dev
// (include/lungmask_hip.h) -- the affine coordinate with its inside test and nearest index, the clamped linear and cubic taps, the
// trilinear, tricubic and label-linear values, the output conversion --, the displacement of lm_warp_dev's coordinate rule and
// lm_jacobian_dev's determinant, and the four gathers built from it, written once as templates over the map that turns an output
// index into a source coordinate.  All of it is float64 without contraction in the order written:
// these expressions are the header's contract, and lm_warp_dev, lm_joint_hist_dev and lm_demons_step_dev are defined through them.
// One definition each; compiles under hipcc and under the g++ emulation (lm_platform.h).
//
// A map supplies `total` (output voxels), `e0, e1, e2` (source extents) and `coord(o, c, j)`: the coordinate of output voxel o, the
// nearest index, and whether it lies inside.  The gathers: one thread per output voxel, x fastest, so that a wave's store is one
// contiguous run; the tap indices and weights stay in fully unrolled registers (no scratch, no LDS).
#pragma once
#include <cstring>
#include <string>
#include <type_traits>

#include "volume_common.h"

namespace lm {

constexpr int kGather = 256;  // threads of a gather workgroup

template <class OUT>
__device__ __forceinline__ OUT sample_out(double v);
template <>
__device__ __forceinline__ float sample_out<float>(double v) { return (float)v; }
template <>
__device__ __forceinline__ uint16_t sample_out<uint16_t>(double v) {  // (half)(float)v, round to nearest even both times
#ifdef LM_EMU_BUILD
    return lm_f2h((float)v);
#else
    return __builtin_bit_cast(uint16_t, lm_f2h((float)v));
#endif
}
template <>
__device__ __forceinline__ int16_t sample_out<int16_t>(double v) {  // rint (half to even), saturated
    const double r = rint(v);
    return r >= 32767.0 ? (int16_t)32767 : (r <= -32768.0 ? (int16_t)-32768 : (int16_t)(int)r);
}

// linear index o of a grid with N1 rows per slice and N2 voxels per row -> (slice, row, column)
__device__ __forceinline__ void index_split(unsigned o, unsigned N1, unsigned N2, unsigned& o0, unsigned& o1, unsigned& o2) {
    const unsigned row = o / N2;
    o2 = o - row * N2;
    o0 = row / N1;
    o1 = row - o0 * N1;
}

// Steps 1 and 2 of lm_resample_dev at the point p: the coordinate c = A p + b, the inside test and the nearest index j (0 outside).
__device__ __forceinline__ bool affine_coord(const double A[9], const double b[3], double p0, double p1, double p2, int e0, int e1, int e2,
                                             double c[3], int j[3]) {
    const int e[3] = {e0, e1, e2};
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = ((A[3 * i] * p0 + A[3 * i + 1] * p1) + A[3 * i + 2] * p2) + b[i];
        const double t = floor(c[i] + 0.5);
        const bool in = t >= 0.0 && t < (double)e[i];  // (false for a NaN)
        j[i] = in ? (int)t : 0;
        inside = inside && in;
    }
    return inside;
}

// The first step of the coordinate rule: p = o + u * field_scale at voxel o of a field u [3][N]; p = o without a field.
__device__ __forceinline__ void displace(const float* __restrict__ u, size_t N, unsigned o, const double fs[3], double& p0, double& p1,
                                         double& p2) {
    if (u) {
        p0 = p0 + (double)u[o] * fs[0];
        p1 = p1 + (double)u[N + o] * fs[1];
        p2 = p2 + (double)u[2 * N + o] * fs[2];
    }
}

// lm_jacobian_dev's determinant of I + grad(u * field_scale) at voxel p = (o[0], o[1], o[2]) of a field [3][N] on a grid of extents
// e: central differences inside, one-sided at a face, zero along an axis of extent 1
__device__ __forceinline__ double field_det(const float* __restrict__ field, size_t N, unsigned p, const int o[3], const int e[3],
                                            const size_t stride[3], const double fs[3]) {
    double a[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* __restrict__ ui = field + (size_t)i * N;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool up = o[j] + 1 < e[j], down = o[j] > 0;
            double G = 0.0;  // (an axis of extent 1)
            if (up && down) G = (((double)ui[(size_t)p + stride[j]] - (double)ui[(size_t)p - stride[j]]) * fs[i]) * 0.5;
            else if (up) G = ((double)ui[(size_t)p + stride[j]] - (double)ui[p]) * fs[i];
            else if (down) G = ((double)ui[p] - (double)ui[(size_t)p - stride[j]]) * fs[i];
            a[i][j] = (i == j ? 1.0 : 0.0) + G;
        }
    }
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}

// the linear taps of the clamped coordinate along an axis of extent e
__device__ __forceinline__ void taps2(double c, int e, int& i0, int& i1, double& f) {
    const double last = (double)(e - 1);
    c = c > 0.0 ? c : 0.0;
    c = c < last ? c : last;
    const double fl = floor(c);
    i0 = (int)fl;
    f = c - fl;
    i1 = i0 + 1 < e - 1 ? i0 + 1 : e - 1;
}

__device__ __forceinline__ double lerp(double a, double b, double f) { return a * (1.0 - f) + b * f; }

// the trilinear value (4. of lm_resample_dev) at the coordinate c, clamped here
template <class T>
__device__ __forceinline__ double trilinear(const T* __restrict__ src, const double c[3], int e0, int e1, int e2) {
    int z0, z1, y0, y1, x0, x1;
    double fz, fy, fx;
    taps2(c[0], e0, z0, z1, fz);
    taps2(c[1], e1, y0, y1, fy);
    taps2(c[2], e2, x0, x1, fx);
    const T* __restrict__ r00 = src + ((size_t)z0 * e1 + y0) * e2;
    const T* __restrict__ r01 = src + ((size_t)z0 * e1 + y1) * e2;
    const T* __restrict__ r10 = src + ((size_t)z1 * e1 + y0) * e2;
    const T* __restrict__ r11 = src + ((size_t)z1 * e1 + y1) * e2;
    const double v00 = lerp((double)r00[x0], (double)r00[x1], fx);
    const double v01 = lerp((double)r01[x0], (double)r01[x1], fx);
    const double v10 = lerp((double)r10[x0], (double)r10[x1], fx);
    const double v11 = lerp((double)r11[x0], (double)r11[x1], fx);
    return lerp(lerp(v00, v01, fy), lerp(v10, v11, fy), fz);
}

// m(k) of the header for k >= -1: the mirror index with period 2e - 2
__device__ __forceinline__ int mirror(int k, int e) {
    if (e == 1) return 0;
    const int P = 2 * e - 2;
    int m = k % P;
    m = m < 0 ? m + P : m;
    return m >= e ? P - m : m;
}

// the four cubic taps and weights of the clamped coordinate
__device__ __forceinline__ void taps4(double c, int e, int idx[4], double w[4]) {
    const double last = (double)(e - 1);
    c = c > 0.0 ? c : 0.0;
    c = c < last ? c : last;
    const double fl = floor(c);
    const int i0 = (int)fl;
    const double f = c - fl, g = 1.0 - f;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = mirror(i0 - 1 + k, e);
    w[0] = ((g * g) * g) / 6.0;
    w[1] = 2.0 / 3.0 - ((f * f) * (2.0 - f)) / 2.0;
    w[2] = 2.0 / 3.0 - ((g * g) * (1.0 + f)) / 2.0;
    w[3] = ((f * f) * f) / 6.0;
}

// the cubic B-spline value of the coefficients (lm_spline_prefilter_dev) at the coordinate c: 4 x 4 x 4 taps, x innermost
__device__ __forceinline__ double tricubic(const double* __restrict__ coef, const double c[3], int e0, int e1, int e2) {
    int iz[4], iy[4], ix[4];
    double wz[4], wy[4], wx[4];
    taps4(c[0], e0, iz, wz);
    taps4(c[1], e1, iy, wy);
    taps4(c[2], e2, ix, wx);
    double vz = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double vy = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double* __restrict__ row = coef + ((size_t)iz[a] * e1 + iy[b]) * e2;
            double vx = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) vx = vx + wx[k] * row[ix[k]];
            vy = vy + wy[b] * vx;
        }
        vz = vz + wz[a] * vy;
    }
    return vz;
}

// the label with the largest sum of trilinear weights over the eight corners, the lowest label on ties
__device__ __forceinline__ uint8_t label_linear(const uint8_t* __restrict__ src, const double c[3], int e0, int e1, int e2) {
    int z0, z1, y0, y1, x0, x1;
    double fz, fy, fx;
    taps2(c[0], e0, z0, z1, fz);
    taps2(c[1], e1, y0, y1, fy);
    taps2(c[2], e2, x0, x1, fx);
    const double wz[2] = {1.0 - fz, fz}, wy[2] = {1.0 - fy, fy}, wx[2] = {1.0 - fx, fx};
    const int zi[2] = {z0, z1}, yi[2] = {y0, y1}, xi[2] = {x0, x1};
    int lab[8];
    double wgt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // z-major corner order
        const int a = k >> 2, b = (k >> 1) & 1, d = k & 1;
        lab[k] = src[((size_t)zi[a] * e1 + yi[b]) * e2 + xi[d]];
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
    return (uint8_t)best;
}

// ------------------------------------------------------------------------------------------------ the gathers
// U: an unsigned integer of the element's size -- the raw value goes through untouched; fill_bits: the fill in the source's dtype
template <class Map, class U>
__global__ __launch_bounds__(kGather) void gather_nearest_kernel(Map m, const U* __restrict__ src, U fill_bits, U* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kGather + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    const bool inside = m.coord(o, c, j);
    out[o] = inside ? src[((size_t)j[0] * m.e1 + j[1]) * m.e2 + j[2]] : fill_bits;
}

template <class Map, class T, class OUT>
__global__ __launch_bounds__(kGather) void gather_linear_kernel(Map m, const T* __restrict__ src, double fill, OUT* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kGather + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    double v = fill;
    if (m.coord(o, c, j)) v = trilinear(src, c, m.e0, m.e1, m.e2);
    out[o] = sample_out<OUT>(v);
}

template <class Map, class OUT>
__global__ __launch_bounds__(kGather) void gather_cubic_kernel(Map m, const double* __restrict__ coef, double fill, OUT* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kGather + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    double v = fill;
    if (m.coord(o, c, j)) v = tricubic(coef, c, m.e0, m.e1, m.e2);
    out[o] = sample_out<OUT>(v);
}

template <class Map>
__global__ __launch_bounds__(kGather) void gather_label_linear_kernel(Map m, const uint8_t* __restrict__ src, uint8_t fill,
                                                                      uint8_t* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kGather + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    uint8_t res = fill;
    if (m.coord(o, c, j)) res = label_linear(src, c, m.e0, m.e1, m.e2);
    out[o] = res;
}

// ------------------------------------------------------------------------------------------------ host side
// the fill of LM_RS_NEAREST in the source's dtype, as the bits of an unsigned integer of its size
inline uint64_t nearest_fill_bits(int dtype, double fill) {
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

template <class Map, class T>
hipError_t launch_gather_linear(const Map& m, dim3 grid, const void* src, int out_dtype, double fill, void* out, hipStream_t s) {
    const dim3 block(kGather);
    const T* in = static_cast<const T*>(src);
    if (out_dtype == LM_F32) LM_LAUNCH((gather_linear_kernel<Map, T, float>), grid, block, 0, s, m, in, fill, static_cast<float*>(out));
    else if (out_dtype == LM_F16) LM_LAUNCH((gather_linear_kernel<Map, T, uint16_t>), grid, block, 0, s, m, in, fill, static_cast<uint16_t*>(out));
    else if constexpr (std::is_integral<T>::value)
        LM_LAUNCH((gather_linear_kernel<Map, T, int16_t>), grid, block, 0, s, m, in, fill, static_cast<int16_t*>(out));
    return hipGetLastError();
}

// The gather of p.mode through the map `m` from an [n][h][w] source of `dtype` (LM_RS_CUBIC: the float64 coefficients), profiled as
// kind_prefix + "nearest" / "linear" / "cubic" / "label_linear"; extra_bytes: what the map itself reads per call.
template <class Map>
int launch_gather(lm_engine* e, const Map& m, const char* kind_prefix, const void* src, int dtype, int n, int h, int w,
                  const lm_resample_params& p, double extra_bytes, void* out) {
    const double nsrc = (double)n * h * w, nout = (double)m.total;
    const dim3 grid((m.total + (unsigned)kGather - 1u) / (unsigned)kGather), block(kGather);
    const std::string prefix(kind_prefix);
    hipError_t err = hipSuccess;
    if (p.mode == LM_RS_NEAREST) {
        const int esz = dtype == LM_U8 ? 1 : dtype_bytes(dtype);
        const uint64_t fb = nearest_fill_bits(dtype, p.fill);
        ProfScope ps(e, (prefix + "nearest").c_str(), (nsrc + nout) * esz + extra_bytes);
        if (esz == 1)
            LM_LAUNCH((gather_nearest_kernel<Map, uint8_t>), grid, block, 0, e->stream, m, static_cast<const uint8_t*>(src), (uint8_t)fb,
                      static_cast<uint8_t*>(out));
        else if (esz == 2)
            LM_LAUNCH((gather_nearest_kernel<Map, uint16_t>), grid, block, 0, e->stream, m, static_cast<const uint16_t*>(src), (uint16_t)fb,
                      static_cast<uint16_t*>(out));
        else if (esz == 4)
            LM_LAUNCH((gather_nearest_kernel<Map, uint32_t>), grid, block, 0, e->stream, m, static_cast<const uint32_t*>(src), (uint32_t)fb,
                      static_cast<uint32_t*>(out));
        else
            LM_LAUNCH((gather_nearest_kernel<Map, uint64_t>), grid, block, 0, e->stream, m, static_cast<const uint64_t*>(src), fb,
                      static_cast<uint64_t*>(out));
        err = hipGetLastError();
    } else if (p.mode == LM_RS_LABEL_LINEAR) {
        ProfScope ps(e, (prefix + "label_linear").c_str(), nsrc + nout + extra_bytes);
        LM_LAUNCH((gather_label_linear_kernel<Map>), grid, block, 0, e->stream, m, static_cast<const uint8_t*>(src), (uint8_t)p.fill,
                  static_cast<uint8_t*>(out));
        err = hipGetLastError();
    } else if (p.mode == LM_RS_LINEAR) {
        const int osz = p.out_dtype == LM_F32 ? 4 : 2;
        ProfScope ps(e, (prefix + "linear").c_str(), nsrc * dtype_bytes(dtype) + nout * osz + extra_bytes);
        switch (dtype) {
            case LM_I16: err = launch_gather_linear<Map, int16_t>(m, grid, src, p.out_dtype, p.fill, out, e->stream); break;
            case LM_I32: err = launch_gather_linear<Map, int32_t>(m, grid, src, p.out_dtype, p.fill, out, e->stream); break;
            case LM_I64: err = launch_gather_linear<Map, int64_t>(m, grid, src, p.out_dtype, p.fill, out, e->stream); break;
            case LM_F32: err = launch_gather_linear<Map, float>(m, grid, src, p.out_dtype, p.fill, out, e->stream); break;
            default: err = launch_gather_linear<Map, double>(m, grid, src, p.out_dtype, p.fill, out, e->stream);
        }
    } else {
        const int osz = p.out_dtype == LM_F32 ? 4 : 2;
        const double* coef = static_cast<const double*>(src);
        ProfScope ps(e, (prefix + "cubic").c_str(), nsrc * 8.0 + nout * osz + extra_bytes);
        if (p.out_dtype == LM_F32) LM_LAUNCH((gather_cubic_kernel<Map, float>), grid, block, 0, e->stream, m, coef, p.fill, static_cast<float*>(out));
        else if (p.out_dtype == LM_F16)
            LM_LAUNCH((gather_cubic_kernel<Map, uint16_t>), grid, block, 0, e->stream, m, coef, p.fill, static_cast<uint16_t*>(out));
        else LM_LAUNCH((gather_cubic_kernel<Map, int16_t>), grid, block, 0, e->stream, m, coef, p.fill, static_cast<int16_t*>(out));
        err = hipGetLastError();
    }
    LM_K(err);
    return LM_OK;
}

// The workgroups of a kernel that walks a contiguous run of `total` items in sweeps of `threads`, and the items each takes: whole
// sweeps, so that a wave reads a contiguous run.  The grid grows once a thread has more than per_thread items, up to max_blocks.
inline int walk_plan(unsigned total, int threads, int per_thread, int max_blocks, unsigned& per_block) {
    const unsigned chunk = (unsigned)(threads * per_thread);
    int blocks = (int)std::min<unsigned>((total + chunk - 1u) / chunk, (unsigned)max_blocks);
    blocks = std::max(blocks, 1);
    const unsigned per = (total + (unsigned)blocks - 1u) / (unsigned)blocks;
    per_block = (per + (unsigned)threads - 1u) / (unsigned)threads * (unsigned)threads;
    return blocks;
}

}  // namespace lm
