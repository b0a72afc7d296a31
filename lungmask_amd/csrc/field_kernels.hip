// Displacement fields as operands (lm_field_combine_dev; include/lungmask_hip.h): a field sampled through another field, rotated,
// scaled and added -- the one device operation under inversion, composition, transport onto another grid and the difference of two
// fields (lungmask_amd.deformable: invert, compose, inverse_consistency).  The arithmetic is the header's: float64 without
// contraction in the order written, one rounding to float32 per component; the coordinate, the inside test, the clamp and the taps
// are lm_resample_dev's, from sample_common.h.  Every sum across threads is an integer sum and the maximum is an integer maximum, so
// no result depends on the schedule.
//
// fc_combine_kernel: a workgroup of kFC = 256 threads walks a contiguous run of output voxels in sweeps of 256 (walk_plan), x
// fastest, so that a wave reads and writes contiguous runs of every component of coord, add, ref and out.  The taps of the clamped
// coordinate are computed once and shared by the three components: 24 corner loads per voxel, all in registers (no scratch).  The
// counts are kept per thread, merged into LDS counters once per thread (atomicAdd, atomicMax for the maximum) and flushed with one
// 64-bit atomic per counter and workgroup into the output, which the call zeroes first (hipMemsetAsync on the same stream).
//   LDS per workgroup: 32 bytes (four counters).  VGPRs: 87 (five waves per SIMD; the compiler's report for gfx950 at -O3), no scratch.
//   A contribution to counts[2] is at most 2^30 and a grid has fewer than 2^31 voxels: the sum stays below 2^61.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kFC = 256;            // threads of a workgroup
constexpr int kFCMaxBlocks = 2048;  // eight workgroups per CU
constexpr int kFCPerThread = 8;     // voxels per thread before the grid grows

struct FcMap {
    double A[9], b[3], fs[3], R[9];
    double alpha, beta;
    int e0, e1, e2;      // source extents
    int N1, N2;          // output rows per slice, voxels per row
    unsigned total;      // output voxels
    unsigned per_block;  // voxels per workgroup
};

__global__ __launch_bounds__(kFC) void fc_combine_kernel(FcMap m, const float* __restrict__ add, const float* __restrict__ coord,
                                                        const float* __restrict__ src, const float* __restrict__ ref,
                                                        float* __restrict__ out, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long cnt[4];
    const int tid = threadIdx.x;
    if (tid < 4) cnt[tid] = 0ull;
    __syncthreads();

    unsigned c_out = 0, c_nan = 0;
    unsigned long long c_sum = 0ull, c_max = 0ull;
    const size_t N = (size_t)m.total;
    const size_t S = ((size_t)m.e0 * m.e1) * m.e2;  // voxels of a source component
    const unsigned first = blockIdx.x * m.per_block;
    const unsigned last = min(m.total, first + m.per_block);  // (first < 2^31 + 2^19: no wrap)
    for (unsigned p = first + (unsigned)tid; p < last; p += (unsigned)kFC) {
        unsigned q0, q1, q2;
        index_split(p, (unsigned)m.N1, (unsigned)m.N2, q0, q1, q2);
        // 1. the coordinate rule with coord as the field, the inside test; an outside voxel is sampled at the clamped coordinate
        double p0 = (double)q0, p1 = (double)q1, p2 = (double)q2, c[3];
        int j[3];
        displace(coord, N, p, m.fs, p0, p1, p2);
        if (!affine_coord(m.A, m.b, p0, p1, p2, m.e0, m.e1, m.e2, c, j)) ++c_out;
        // 2. one set of taps, three trilinear values (lm_resample_dev's 4., the order of sample_common.h's trilinear)
        int z0, z1, y0, y1, x0, x1;
        double fz, fy, fx;
        taps2(c[0], m.e0, z0, z1, fz);
        taps2(c[1], m.e1, y0, y1, fy);
        taps2(c[2], m.e2, x0, x1, fx);
        const size_t r00 = ((size_t)z0 * m.e1 + y0) * m.e2, r01 = ((size_t)z0 * m.e1 + y1) * m.e2;
        const size_t r10 = ((size_t)z1 * m.e1 + y0) * m.e2, r11 = ((size_t)z1 * m.e1 + y1) * m.e2;
        double s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* __restrict__ sk = src + (size_t)k * S;
            const double v00 = lerp((double)sk[r00 + x0], (double)sk[r00 + x1], fx);
            const double v01 = lerp((double)sk[r01 + x0], (double)sk[r01 + x1], fx);
            const double v10 = lerp((double)sk[r10 + x0], (double)sk[r10 + x1], fx);
            const double v11 = lerp((double)sk[r11 + x0], (double)sk[r11 + x1], fx);
            s[k] = lerp(lerp(v00, v01, fy), lerp(v10, v11, fy), fz);
        }
        // 3. rotate, 4. combine, 5. the squared difference from ref
        double d2 = 0.0, d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double t = (m.R[3 * k] * s[0] + m.R[3 * k + 1] * s[1]) + m.R[3 * k + 2] * s[2];
            double v = m.beta * t;
            if (add) v = m.alpha * (double)add[(size_t)k * N + p] + m.beta * t;
            const float o = (float)v;
            out[(size_t)k * N + p] = o;
            d[k] = (double)o - (ref ? (double)ref[(size_t)k * N + p] : 0.0);
        }
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        if (d2 != d2) {
            ++c_nan;
        } else {
            const double capped = d2 < 256.0 ? d2 : 256.0;
            const unsigned long long q = (unsigned long long)(long long)floor(capped * 4194304.0 + 0.5);
            c_sum += q;
            c_max = q > c_max ? q : c_max;
        }
    }
    if (counts) {
        if (c_out) atomicAdd(&cnt[0], (unsigned long long)c_out);
        if (c_nan) atomicAdd(&cnt[1], (unsigned long long)c_nan);
        if (c_sum) atomicAdd(&cnt[2], c_sum);
        if (c_max) atomicMax(&cnt[3], c_max);
        __syncthreads();
        if (tid < 3 && cnt[tid]) atomicAdd(counts + tid, cnt[tid]);
        if (tid == 3 && cnt[3]) atomicMax(counts + 3, cnt[3]);
    }
}

}  // namespace

int field_combine(lm_engine* e, const float* add, const float* coord, const float* src, int n, int h, int w, const float* ref,
                  const lm_field_combine_params& p, float* out, int64_t* counts_out) {
    FcMap m;
    for (int i = 0; i < 9; ++i) m.A[i] = p.A[i], m.R[i] = p.R[i];
    for (int i = 0; i < 3; ++i) m.b[i] = p.b[i], m.fs[i] = p.field_scale[i];
    m.alpha = p.alpha, m.beta = p.beta;
    m.e0 = n, m.e1 = h, m.e2 = w;
    m.N1 = p.out_dims[1], m.N2 = p.out_dims[2];
    m.total = (unsigned)((size_t)p.out_dims[0] * p.out_dims[1] * p.out_dims[2]);
    const int blocks = walk_plan(m.total, kFC, kFCPerThread, kFCMaxBlocks, m.per_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
    if (counts) LM_K(hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), e->stream));
    // reads: the coordinate field, the added field, the reference, the source's corners (each voxel once from memory); writes: three components
    ProfScope ps(e, "fc_combine", (double)m.total * (12.0 * ((coord ? 1 : 0) + (add ? 1 : 0) + (ref ? 1 : 0)) + 12.0) + 12.0 * (double)n * h * w);
    LM_LAUNCH(fc_combine_kernel, dim3(blocks), dim3(kFC), 0, e->stream, m, add, coord, src, ref, out, counts);
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace lm
