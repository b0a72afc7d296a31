// Deformable registration (lm_warp_dev, lm_demons_step_dev, lm_jacobian_dev; include/lungmask_hip.h): a volume gathered through a dense
// displacement field, one additive demons iteration, and the Jacobian determinant of a field.  The arithmetic is the header's: float64
// without contraction in the order written, one rounding to float32 at the end; every sum across threads is an integer sum, so no
// result depends on the schedule.  The coordinate, the inside test, the clamp, the taps and the output conversion are
// lm_resample_dev's, from sample_common.h: one definition, so lm_warp_dev without a field IS lm_resample_dev.
//
// The gathers are sample_common.h's (gather_nearest_kernel, gather_linear_kernel, gather_cubic_kernel, gather_label_linear_kernel),
// instantiated here with DfMap, which displaces the output index by the field before the affine map: the three field components are
// read as three contiguous runs per wave, the eight corners or 64 taps stay in registers (no scratch, no LDS).
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

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kDF = 256;            // threads of a workgroup
constexpr int kDFMaxBlocks = 2048;  // demons step and Jacobian: eight workgroups per CU
constexpr int kDFPerThread = 8;     // voxels per thread before the grid grows

struct DfMap {
    double A[9], b[3], fs[3];
    int e0, e1, e2;      // source extents
    int N1, N2;          // output rows per slice, voxels per row
    unsigned total;      // output voxels
    const float* field;  // [3][total] displacements, or NULL: p = o (last: in front of the extents the gathers take 58 SGPRs, not 50 / 52)
    // p = o + u * field_scale (p = o without a field), then lm_resample_dev's coordinate of p
    __device__ __forceinline__ bool coord(unsigned o, double c[3], int j[3]) const {
        unsigned o0, o1, o2;
        index_split(o, (unsigned)N1, (unsigned)N2, o0, o1, o2);
        double p0 = (double)o0, p1 = (double)o1, p2 = (double)o2;
        displace(field, (size_t)total, o, fs, p0, p1, p2);
        return affine_coord(A, b, p0, p1, p2, e0, e1, e2, c, j);
    }
};

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
        unsigned q0, q1, q2;
        index_split(p, (unsigned)m.fe1, (unsigned)m.fe2, q0, q1, q2);
        const int o[3] = {(int)q0, (int)q1, (int)q2};
        const float u0 = u[p], u1 = u[N + p], u2 = u[2 * N + p];
        float r0 = u0, r1 = u1, r2 = u2;
        if (!flab || table[flab[p]]) {
            ++c_sel;
            const double f = load_as<double>(fixed, m.fdtype, (size_t)p);
            double p0 = (double)o[0], p1 = (double)o[1], p2 = (double)o[2], c[3];
            int j[3];
            // u is never NULL here; the test inside displace, which the kernel shares with DfMap, keeps it at 67 to 69 VGPRs (72 to 74
            // and one wave less for float64 and int64 without it)
            displace(u, N, p, m.fs, p0, p1, p2);
            if (f != f) {
                ++c_nan;
            } else if (!affine_coord(m.A, m.b, p0, p1, p2, m.me0, m.me1, m.me2, c, j)) {
                ++c_out;
            } else {
                const double mv = trilinear(mov, c, m.me0, m.me1, m.me2);
                double g[3];
                bool nan = mv != mv;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const size_t hi = o[a] + 1 < fe[a] ? (size_t)p + stride[a] : (size_t)p;
                    const size_t lo = o[a] > 0 ? (size_t)p - stride[a] : (size_t)p;
                    g[a] = fe[a] == 1 ? 0.0 : (load_as<double>(fixed, m.fdtype, hi) - load_as<double>(fixed, m.fdtype, lo)) * m.gs[a];
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
        unsigned q0, q1, q2;
        index_split(p, (unsigned)m.e1, (unsigned)m.e2, q0, q1, q2);
        const int o[3] = {(int)q0, (int)q1, (int)q2};
        const double det = field_det(field, N, p, o, e, stride, m.fs);
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
    m.field = field;
    m.e0 = n, m.e1 = h, m.e2 = w;
    m.N1 = p.out_dims[1], m.N2 = p.out_dims[2];
    m.total = (unsigned)((size_t)p.out_dims[0] * p.out_dims[1] * p.out_dims[2]);
    return launch_gather(e, m, "df_", src, dtype, n, h, w, p, field ? 12.0 * (double)m.total : 0.0, out);
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
    const int blocks = walk_plan(m.total, kDF, kDFPerThread, kDFMaxBlocks, m.per_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
    LM_K(hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), e->stream));
    // reads: the fixed value and its six neighbours (from cache), the labels, the field, the moving corners; writes: three components
    ProfScope ps(e, "df_demons", (double)m.total * (dtype_bytes(fdtype) + (flab ? 1 : 0) + 12 + dtype_bytes(mdtype) + 12));
    LM_K(with_image_type(mdtype, [&](auto tag) {
        return launch_demons<typename decltype(tag)::type>(m, blocks, fixed, flab, mov, u, out, counts, e->stream);
    }));
    return LM_OK;
}

int jacobian(lm_engine* e, const float* field, int n, int h, int w, const double field_scale[3], float* det_out, int64_t* counts_out) {
    JacMap m;
    for (int i = 0; i < 3; ++i) m.fs[i] = field_scale[i];
    m.e0 = n, m.e1 = h, m.e2 = w;
    m.total = (unsigned)((size_t)n * h * w);
    const int blocks = walk_plan(m.total, kDF, kDFPerThread, kDFMaxBlocks, m.per_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
    if (counts) LM_K(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), e->stream));
    ProfScope ps(e, "df_jacobian", (double)m.total * 16.0);
    LM_LAUNCH(df_jacobian_kernel, dim3(blocks), dim3(kDF), 0, e->stream, m, field, det_out, counts);
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace lm
