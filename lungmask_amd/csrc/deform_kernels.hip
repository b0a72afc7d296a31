// Deformable registration (lm_warp_dev, lm_demons_step_dev, lm_jacobian_dev; include/lungmask_hip.h): a volume gathered through a dense
// displacement field, one additive demons iteration, and the Jacobian determinant of a field.  The arithmetic is the header's: float64
// without contraction in the order written, one rounding to float32 at the end; every sum across threads is an integer sum, so no
// result depends on the schedule.  The coordinate, the inside test, the clamp and the taps are lm_resample_dev's, restated here
// (resample_kernels.hip keeps its kernel set): df_taps2, df_lerp, df_mirror, df_taps4 and df_out are its rs_* helpers word for word.
//
// The gathers (df_nearest_kernel, df_linear_kernel, df_cubic_kernel, df_label_linear_kernel): one thread per output voxel, x fastest,
// the three field components read as three contiguous runs per wave, the eight corners or 64 taps in registers (no scratch, no LDS).
//
// df_demons_kernel<T> (T: the moving volume's element; the fixed volume's dtype is read at run time -- seven loads per voxel) and
// df_jacobian_kernel: a workgroup of kDF = 256 threads walks a contiguous run of voxels in sweeps of 256, so that a wave reads and
// writes contiguous runs of every component.  The counts are kept per thread, added to LDS counters once per thread and flushed with
// one 64-bit atomic per counter and workgroup into the output, which the call zeroes first (hipMemsetAsync on the same stream).
//   LDS per workgroup: 40 (five counters) + 256 (label table) = 296 bytes for the demons step, 16 bytes (two counters) for the Jacobian.
//   A contribution to counts[4] is at most 2^28 and a volume has fewer than 2^31 voxels: the sum stays below 2^59.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kDF = 256;            // threads of a workgroup
constexpr int kDFMaxBlocks = 2048;  // demons step and Jacobian: eight workgroups per CU
constexpr int kDFPerThread = 8;     // voxels per thread before the grid grows

struct DfMap {
    double A[9], b[3], fs[3];
    int e0, e1, e2;  // source extents
    int N1, N2;      // output rows per slice, voxels per row
    unsigned total;  // output voxels
};

template <class OUT>
__device__ __forceinline__ OUT df_out(double v);
template <>
__device__ __forceinline__ float df_out<float>(double v) { return (float)v; }
template <>
__device__ __forceinline__ uint16_t df_out<uint16_t>(double v) {  // (half)(float)v, round to nearest even both times
#ifdef LM_EMU_BUILD
    return lm_f2h((float)v);
#else
    return __builtin_bit_cast(uint16_t, lm_f2h((float)v));
#endif
}
template <>
__device__ __forceinline__ int16_t df_out<int16_t>(double v) {  // rint (half to even), saturated
    const double r = rint(v);
    return r >= 32767.0 ? (int16_t)32767 : (r <= -32768.0 ? (int16_t)-32768 : (int16_t)(int)r);
}

// The coordinate rule for output voxel `o` at index (o0, o1, o2): p = o + u * field_scale (p = o without a field), c = A p + b, the
// inside test and the nearest index.
__device__ __forceinline__ bool df_coord_at(const double A[9], const double b[3], const double fs[3], const float* __restrict__ field,
                                            size_t total, size_t o, double o0, double o1, double o2, int e0, int e1, int e2, double c[3],
                                            int j[3]) {
    double p0 = o0, p1 = o1, p2 = o2;
    if (field) {
        p0 = o0 + (double)field[o] * fs[0];
        p1 = o1 + (double)field[total + o] * fs[1];
        p2 = o2 + (double)field[2 * total + o] * fs[2];
    }
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

__device__ __forceinline__ bool df_coord(const DfMap& m, const float* __restrict__ field, unsigned o, double c[3], int j[3]) {
    const unsigned row = o / (unsigned)m.N2;
    const double o2 = (double)(o - row * (unsigned)m.N2);
    const unsigned sl = row / (unsigned)m.N1;
    const double o1 = (double)(row - sl * (unsigned)m.N1), o0 = (double)sl;
    return df_coord_at(m.A, m.b, m.fs, field, (size_t)m.total, (size_t)o, o0, o1, o2, m.e0, m.e1, m.e2, c, j);
}

// the linear taps of the clamped coordinate along an axis of extent e
__device__ __forceinline__ void df_taps2(double c, int e, int& i0, int& i1, double& f) {
    const double last = (double)(e - 1);
    c = c > 0.0 ? c : 0.0;
    c = c < last ? c : last;
    const double fl = floor(c);
    i0 = (int)fl;
    f = c - fl;
    i1 = i0 + 1 < e - 1 ? i0 + 1 : e - 1;
}

__device__ __forceinline__ double df_lerp(double a, double b, double f) { return a * (1.0 - f) + b * f; }

// the trilinear value of lm_resample_dev (4. there) on the coordinate c, clamped here
template <class T>
__device__ __forceinline__ double df_trilinear(const T* __restrict__ src, const double c[3], int e0, int e1, int e2) {
    int z0, z1, y0, y1, x0, x1;
    double fz, fy, fx;
    df_taps2(c[0], e0, z0, z1, fz);
    df_taps2(c[1], e1, y0, y1, fy);
    df_taps2(c[2], e2, x0, x1, fx);
    const T* __restrict__ r00 = src + ((size_t)z0 * e1 + y0) * e2;
    const T* __restrict__ r01 = src + ((size_t)z0 * e1 + y1) * e2;
    const T* __restrict__ r10 = src + ((size_t)z1 * e1 + y0) * e2;
    const T* __restrict__ r11 = src + ((size_t)z1 * e1 + y1) * e2;
    const double v00 = df_lerp((double)r00[x0], (double)r00[x1], fx);
    const double v01 = df_lerp((double)r01[x0], (double)r01[x1], fx);
    const double v10 = df_lerp((double)r10[x0], (double)r10[x1], fx);
    const double v11 = df_lerp((double)r11[x0], (double)r11[x1], fx);
    return df_lerp(df_lerp(v00, v01, fy), df_lerp(v10, v11, fy), fz);
}

// m(k) of the header for k >= -1: the mirror index with period 2e - 2
__device__ __forceinline__ int df_mirror(int k, int e) {
    if (e == 1) return 0;
    const int P = 2 * e - 2;
    int m = k % P;
    m = m < 0 ? m + P : m;
    return m >= e ? P - m : m;
}

// the four cubic taps and weights of the clamped coordinate
__device__ __forceinline__ void df_taps4(double c, int e, int idx[4], double w[4]) {
    const double last = (double)(e - 1);
    c = c > 0.0 ? c : 0.0;
    c = c < last ? c : last;
    const double fl = floor(c);
    const int i0 = (int)fl;
    const double f = c - fl, g = 1.0 - f;
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = df_mirror(i0 - 1 + k, e);
    w[0] = ((g * g) * g) / 6.0;
    w[1] = 2.0 / 3.0 - ((f * f) * (2.0 - f)) / 2.0;
    w[2] = 2.0 / 3.0 - ((g * g) * (1.0 + f)) / 2.0;
    w[3] = ((f * f) * f) / 6.0;
}

// U: an unsigned integer of the element's size -- the raw value goes through untouched; fill_bits: the fill in the source's dtype
template <class U>
__global__ __launch_bounds__(kDF) void df_nearest_kernel(DfMap m, const U* __restrict__ src, const float* __restrict__ field, U fill_bits,
                                                        U* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kDF + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    const bool inside = df_coord(m, field, o, c, j);
    out[o] = inside ? src[((size_t)j[0] * m.e1 + j[1]) * m.e2 + j[2]] : fill_bits;
}

template <class T, class OUT>
__global__ __launch_bounds__(kDF) void df_linear_kernel(DfMap m, const T* __restrict__ src, const float* __restrict__ field, double fill,
                                                       OUT* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kDF + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    double v = fill;
    if (df_coord(m, field, o, c, j)) v = df_trilinear(src, c, m.e0, m.e1, m.e2);
    out[o] = df_out<OUT>(v);
}

template <class OUT>
__global__ __launch_bounds__(kDF) void df_cubic_kernel(DfMap m, const double* __restrict__ coef, const float* __restrict__ field, double fill,
                                                      OUT* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kDF + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    double v = fill;
    if (df_coord(m, field, o, c, j)) {
        int iz[4], iy[4], ix[4];
        double wz[4], wy[4], wx[4];
        df_taps4(c[0], m.e0, iz, wz);
        df_taps4(c[1], m.e1, iy, wy);
        df_taps4(c[2], m.e2, ix, wx);
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
    out[o] = df_out<OUT>(v);
}

__global__ __launch_bounds__(kDF) void df_label_linear_kernel(DfMap m, const uint8_t* __restrict__ src, const float* __restrict__ field,
                                                             uint8_t fill, uint8_t* __restrict__ out) {
    const unsigned o = blockIdx.x * (unsigned)kDF + threadIdx.x;
    if (o >= m.total) return;
    double c[3];
    int j[3];
    uint8_t res = fill;
    if (df_coord(m, field, o, c, j)) {
        int z0, z1, y0, y1, x0, x1;
        double fz, fy, fx;
        df_taps2(c[0], m.e0, z0, z1, fz);
        df_taps2(c[1], m.e1, y0, y1, fy);
        df_taps2(c[2], m.e2, x0, x1, fx);
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

// ------------------------------------------------------------------------------------------------ demons step
struct DemMap {
    double A[9], b[3], fs[3], gs[3];
    double inv_k2, den_min;
    int fe0, fe1, fe2;   // fixed extents
    int me0, me1, me2;   // moving extents
    unsigned total;      // fixed voxels
    unsigned per_block;  // voxels per workgroup
    int fdtype;
    LabelTable keep;
};

__device__ __forceinline__ double df_load(const void* vol, int dtype, size_t v) {
    switch (dtype) {
        case LM_I16: return (double)static_cast<const int16_t*>(vol)[v];
        case LM_I32: return (double)static_cast<const int32_t*>(vol)[v];
        case LM_I64: return (double)static_cast<const int64_t*>(vol)[v];
        case LM_F32: return (double)static_cast<const float*>(vol)[v];
        default: return static_cast<const double*>(vol)[v];
    }
}

template <class T>
__global__ __launch_bounds__(kDF) void df_demons_kernel(DemMap m, const void* __restrict__ fixed, const uint8_t* __restrict__ flab,
                                                       const T* __restrict__ mov, const float* __restrict__ u, float* __restrict__ out,
                                                       unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long cnt[5];
    __shared__ uint8_t table[256];
    const int tid = threadIdx.x;
    if (tid < 5) cnt[tid] = 0ull;
    stage_table(m.keep, table, tid);
    __syncthreads();

    unsigned c_sel = 0, c_in = 0, c_out = 0, c_nan = 0;
    unsigned long long c_d2 = 0ull;
    const size_t N = (size_t)m.total;
    const int fe[3] = {m.fe0, m.fe1, m.fe2};
    const size_t stride[3] = {(size_t)m.fe1 * m.fe2, (size_t)m.fe2, (size_t)1};
    const unsigned first = blockIdx.x * m.per_block;
    const unsigned last = min(m.total, first + m.per_block);  // (first < 2^31 + 2^19: no wrap)
    for (unsigned p = first + (unsigned)tid; p < last; p += (unsigned)kDF) {
        const unsigned row = p / (unsigned)m.fe2;
        const unsigned sl = row / (unsigned)m.fe1;
        const int o[3] = {(int)sl, (int)(row - sl * (unsigned)m.fe1), (int)(p - row * (unsigned)m.fe2)};
        const float u0 = u[p], u1 = u[N + p], u2 = u[2 * N + p];
        float r0 = u0, r1 = u1, r2 = u2;
        if (!flab || table[flab[p]]) {
            ++c_sel;
            const double f = df_load(fixed, m.fdtype, (size_t)p);
            double c[3];
            int j[3];
            if (f != f) {
                ++c_nan;
            } else if (!df_coord_at(m.A, m.b, m.fs, u, N, (size_t)p, (double)o[0], (double)o[1], (double)o[2], m.me0, m.me1, m.me2, c, j)) {
                ++c_out;
            } else {
                const double mv = df_trilinear(mov, c, m.me0, m.me1, m.me2);
                double g[3];
                bool nan = mv != mv;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const size_t hi = o[a] + 1 < fe[a] ? (size_t)p + stride[a] : (size_t)p;
                    const size_t lo = o[a] > 0 ? (size_t)p - stride[a] : (size_t)p;
                    g[a] = fe[a] == 1 ? 0.0 : (df_load(fixed, m.fdtype, hi) - df_load(fixed, m.fdtype, lo)) * m.gs[a];
                    nan = nan || g[a] != g[a];
                }
                if (nan) {
                    ++c_nan;
                } else {
                    const double d = f - mv;
                    const double dd = d * d;
                    const double den = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + dd * m.inv_k2;
                    const bool still = den < m.den_min;
                    const double s0 = still ? 0.0 : (d * g[0]) / den;
                    const double s1 = still ? 0.0 : (d * g[1]) / den;
                    const double s2 = still ? 0.0 : (d * g[2]) / den;
                    r0 = (float)((double)u0 + s0);
                    r1 = (float)((double)u1 + s1);
                    r2 = (float)((double)u2 + s2);
                    ++c_in;
                    const double capped = dd < 16777216.0 ? dd : 16777216.0;  // (a NaN d * d takes the cap)
                    c_d2 += (unsigned long long)(long long)floor(capped * 16.0 + 0.5);
                }
            }
        }
        out[p] = r0;
        out[N + p] = r1;
        out[2 * N + p] = r2;
    }
    if (c_sel) atomicAdd(&cnt[0], (unsigned long long)c_sel);
    if (c_in) atomicAdd(&cnt[1], (unsigned long long)c_in);
    if (c_out) atomicAdd(&cnt[2], (unsigned long long)c_out);
    if (c_nan) atomicAdd(&cnt[3], (unsigned long long)c_nan);
    if (c_d2) atomicAdd(&cnt[4], c_d2);
    __syncthreads();
    if (tid < 5 && cnt[tid]) atomicAdd(counts + tid, cnt[tid]);
}

// ------------------------------------------------------------------------------------------------ Jacobian determinant
struct JacMap {
    double fs[3];
    int e0, e1, e2;
    unsigned total, per_block;
};

__global__ __launch_bounds__(kDF) void df_jacobian_kernel(JacMap m, const float* __restrict__ field, float* __restrict__ det_out,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long cnt[2];
    const int tid = threadIdx.x;
    if (tid < 2) cnt[tid] = 0ull;
    __syncthreads();
    unsigned c_fold = 0, c_nan = 0;
    const size_t N = (size_t)m.total;
    const int e[3] = {m.e0, m.e1, m.e2};
    const size_t stride[3] = {(size_t)m.e1 * m.e2, (size_t)m.e2, (size_t)1};
    const unsigned first = blockIdx.x * m.per_block;
    const unsigned last = min(m.total, first + m.per_block);
    for (unsigned p = first + (unsigned)tid; p < last; p += (unsigned)kDF) {
        const unsigned row = p / (unsigned)m.e2;
        const unsigned sl = row / (unsigned)m.e1;
        const int o[3] = {(int)sl, (int)(row - sl * (unsigned)m.e1), (int)(p - row * (unsigned)m.e2)};
        double a[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float* __restrict__ ui = field + (size_t)i * N;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const bool up = o[j] + 1 < e[j], down = o[j] > 0;
                double G = 0.0;  // (an axis of extent 1)
                if (up && down) G = (((double)ui[(size_t)p + stride[j]] - (double)ui[(size_t)p - stride[j]]) * m.fs[i]) * 0.5;
                else if (up) G = ((double)ui[(size_t)p + stride[j]] - (double)ui[p]) * m.fs[i];
                else if (down) G = ((double)ui[p] - (double)ui[(size_t)p - stride[j]]) * m.fs[i];
                a[i][j] = (i == j ? 1.0 : 0.0) + G;
            }
        }
        const double det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) +
                           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
        det_out[p] = (float)det;
        c_fold += det <= 0.0 ? 1u : 0u;
        c_nan += det != det ? 1u : 0u;
    }
    if (counts) {
        if (c_fold) atomicAdd(&cnt[0], (unsigned long long)c_fold);
        if (c_nan) atomicAdd(&cnt[1], (unsigned long long)c_nan);
        __syncthreads();
        if (tid < 2 && cnt[tid]) atomicAdd(counts + tid, cnt[tid]);
    }
}

inline unsigned blocks_for(unsigned total) { return (total + (unsigned)kDF - 1u) / (unsigned)kDF; }

// the workgroups of a walking kernel and the voxels each takes: whole sweeps, so that a wave reads a contiguous run
inline int walk_plan(unsigned total, unsigned& per_block) {
    const unsigned chunk = (unsigned)(kDF * kDFPerThread);
    int blocks = (int)std::min<unsigned>((total + chunk - 1u) / chunk, (unsigned)kDFMaxBlocks);
    blocks = std::max(blocks, 1);
    const unsigned per = (total + (unsigned)blocks - 1u) / (unsigned)blocks;
    per_block = (per + (unsigned)kDF - 1u) / (unsigned)kDF * (unsigned)kDF;
    return blocks;
}

// the fill of LM_RS_NEAREST in the source's dtype, as the bits of an unsigned integer of its size (lm_resample_dev's rule)
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
hipError_t launch_linear(const DfMap& m, const void* src, const float* field, int out_dtype, double fill, void* out, hipStream_t s) {
    const dim3 grid(blocks_for(m.total)), block(kDF);
    if (out_dtype == LM_F32)
        LM_LAUNCH((df_linear_kernel<T, float>), grid, block, 0, s, m, static_cast<const T*>(src), field, fill, static_cast<float*>(out));
    else if (out_dtype == LM_F16)
        LM_LAUNCH((df_linear_kernel<T, uint16_t>), grid, block, 0, s, m, static_cast<const T*>(src), field, fill, static_cast<uint16_t*>(out));
    else if constexpr (std::is_integral<T>::value)
        LM_LAUNCH((df_linear_kernel<T, int16_t>), grid, block, 0, s, m, static_cast<const T*>(src), field, fill, static_cast<int16_t*>(out));
    return hipGetLastError();
}

template <class T>
hipError_t launch_demons(const DemMap& m, int blocks, const void* fixed, const uint8_t* flab, const void* mov, const float* u, float* out,
                         unsigned long long* counts, hipStream_t s) {
    LM_LAUNCH((df_demons_kernel<T>), dim3(blocks), dim3(kDF), 0, s, m, fixed, flab, static_cast<const T*>(mov), u, out, counts);
    return hipGetLastError();
}

}  // namespace

int warp(lm_engine* e, const void* src, int dtype, int n, int h, int w, const float* field, const lm_resample_params& p,
         const double field_scale[3], void* out) {
    DfMap m;
    for (int i = 0; i < 9; ++i) m.A[i] = p.A[i];
    for (int i = 0; i < 3; ++i) m.b[i] = p.b[i], m.fs[i] = field_scale[i];
    m.e0 = n, m.e1 = h, m.e2 = w;
    m.N1 = p.out_dims[1], m.N2 = p.out_dims[2];
    m.total = (unsigned)((size_t)p.out_dims[0] * p.out_dims[1] * p.out_dims[2]);
    const double nsrc = (double)n * h * w, nout = (double)m.total, nfield = field ? 12.0 * nout : 0.0;
    const dim3 grid(blocks_for(m.total)), block(kDF);
    hipError_t err = hipSuccess;
    if (p.mode == LM_RS_NEAREST) {
        const int esz = dtype == LM_U8 ? 1 : dtype_bytes(dtype);
        const uint64_t fb = nearest_fill_bits(dtype, p.fill);
        ProfScope ps(e, "df_nearest", (nsrc + nout) * esz + nfield);
        if (esz == 1)
            LM_LAUNCH((df_nearest_kernel<uint8_t>), grid, block, 0, e->stream, m, static_cast<const uint8_t*>(src), field, (uint8_t)fb,
                      static_cast<uint8_t*>(out));
        else if (esz == 2)
            LM_LAUNCH((df_nearest_kernel<uint16_t>), grid, block, 0, e->stream, m, static_cast<const uint16_t*>(src), field, (uint16_t)fb,
                      static_cast<uint16_t*>(out));
        else if (esz == 4)
            LM_LAUNCH((df_nearest_kernel<uint32_t>), grid, block, 0, e->stream, m, static_cast<const uint32_t*>(src), field, (uint32_t)fb,
                      static_cast<uint32_t*>(out));
        else
            LM_LAUNCH((df_nearest_kernel<uint64_t>), grid, block, 0, e->stream, m, static_cast<const uint64_t*>(src), field, fb,
                      static_cast<uint64_t*>(out));
        err = hipGetLastError();
    } else if (p.mode == LM_RS_LABEL_LINEAR) {
        ProfScope ps(e, "df_label_linear", nsrc + nout + nfield);
        LM_LAUNCH(df_label_linear_kernel, grid, block, 0, e->stream, m, static_cast<const uint8_t*>(src), field, (uint8_t)p.fill,
                  static_cast<uint8_t*>(out));
        err = hipGetLastError();
    } else if (p.mode == LM_RS_LINEAR) {
        const int osz = p.out_dtype == LM_F32 ? 4 : 2;
        ProfScope ps(e, "df_linear", nsrc * dtype_bytes(dtype) + nout * osz + nfield);
        switch (dtype) {
            case LM_I16: err = launch_linear<int16_t>(m, src, field, p.out_dtype, p.fill, out, e->stream); break;
            case LM_I32: err = launch_linear<int32_t>(m, src, field, p.out_dtype, p.fill, out, e->stream); break;
            case LM_I64: err = launch_linear<int64_t>(m, src, field, p.out_dtype, p.fill, out, e->stream); break;
            case LM_F32: err = launch_linear<float>(m, src, field, p.out_dtype, p.fill, out, e->stream); break;
            default: err = launch_linear<double>(m, src, field, p.out_dtype, p.fill, out, e->stream);
        }
    } else {
        const int osz = p.out_dtype == LM_F32 ? 4 : 2;
        const double* coef = static_cast<const double*>(src);
        ProfScope ps(e, "df_cubic", nsrc * 8.0 + nout * osz + nfield);
        if (p.out_dtype == LM_F32) LM_LAUNCH((df_cubic_kernel<float>), grid, block, 0, e->stream, m, coef, field, p.fill, static_cast<float*>(out));
        else if (p.out_dtype == LM_F16)
            LM_LAUNCH((df_cubic_kernel<uint16_t>), grid, block, 0, e->stream, m, coef, field, p.fill, static_cast<uint16_t*>(out));
        else LM_LAUNCH((df_cubic_kernel<int16_t>), grid, block, 0, e->stream, m, coef, field, p.fill, static_cast<int16_t*>(out));
        err = hipGetLastError();
    }
    LM_K(err);
    return LM_OK;
}

int demons_step(lm_engine* e, const void* fixed, int fdtype, int fn, int fh, int fw, const uint8_t* flab, const void* mov, int mdtype, int mn,
                int mh, int mw, const float* u, const lm_demons_params& p, float* out, int64_t* counts_out) {
    DemMap m;
    for (int i = 0; i < 9; ++i) m.A[i] = p.A[i];
    for (int i = 0; i < 3; ++i) m.b[i] = p.b[i], m.fs[i] = p.field_scale[i], m.gs[i] = p.grad_scale[i];
    m.inv_k2 = p.inv_k2, m.den_min = p.den_min;
    m.fe0 = fn, m.fe1 = fh, m.fe2 = fw;
    m.me0 = mn, m.me1 = mh, m.me2 = mw;
    m.total = (unsigned)((size_t)fn * fh * fw);
    m.fdtype = fdtype;
    m.keep = label_table(p.keep);
    const int blocks = walk_plan(m.total, m.per_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
    LM_K(hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), e->stream));
    // reads: the fixed value and its six neighbours (from cache), the labels, the field, the moving corners; writes: three components
    ProfScope ps(e, "df_demons", (double)m.total * (dtype_bytes(fdtype) + (flab ? 1 : 0) + 12 + dtype_bytes(mdtype) + 12));
    hipError_t err;
    switch (mdtype) {
        case LM_I16: err = launch_demons<int16_t>(m, blocks, fixed, flab, mov, u, out, counts, e->stream); break;
        case LM_I32: err = launch_demons<int32_t>(m, blocks, fixed, flab, mov, u, out, counts, e->stream); break;
        case LM_I64: err = launch_demons<int64_t>(m, blocks, fixed, flab, mov, u, out, counts, e->stream); break;
        case LM_F32: err = launch_demons<float>(m, blocks, fixed, flab, mov, u, out, counts, e->stream); break;
        default: err = launch_demons<double>(m, blocks, fixed, flab, mov, u, out, counts, e->stream);
    }
    LM_K(err);
    return LM_OK;
}

int jacobian(lm_engine* e, const float* field, int n, int h, int w, const double field_scale[3], float* det_out, int64_t* counts_out) {
    JacMap m;
    for (int i = 0; i < 3; ++i) m.fs[i] = field_scale[i];
    m.e0 = n, m.e1 = h, m.e2 = w;
    m.total = (unsigned)((size_t)n * h * w);
    const int blocks = walk_plan(m.total, m.per_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
    if (counts) LM_K(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), e->stream));
    ProfScope ps(e, "df_jacobian", (double)m.total * 16.0);
    LM_LAUNCH(df_jacobian_kernel, dim3(blocks), dim3(kDF), 0, e->stream, m, field, det_out, counts);
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace lm
