// Local-correlation metric of the deformable registration (lm_local_moments_dev, lm_lcc_step_dev; include/lungmask_hip.h): the six
// window sums of a fixed volume and a warped moving volume, and one additive demons iteration whose intensity difference is the
// residual of the window's affine intensity fit and whose force is the gradient of the warped moving volume scaled by the fit's gain.
// The arithmetic is the header's: float64 without contraction in the order written, one rounding to float32 at the end; every sum
// across threads is an integer sum, so no result depends on the schedule.  The coordinate of the outside test is lm_warp_dev's
// (displace and affine_coord of sample_common.h), the label table and the walk of the step are df_demons_kernel's.
//
// Window sums: three passes of direct sums (no sliding update: the order of a window's additions is the header's), x, y, z.
//   lc_moments_x_kernel     a wave owns a row and walks it in chunks of 256 outputs: the two float32 lines go ONCE into an LDS line tile
//                           (256 + 2 * 8 cells each; a cell outside the row or not valid is a NaN in the f tile), and every lane forms the
//                           six terms of a cell in float64 and adds them, a zero for a cell that does not count -- adding 0.0 changes no
//                           bit of a sum that starts at +0.0.  Lanes run along x: the tile reads and the six stores are contiguous runs.
//   lc_moments_line_kernel  y and z: a tile of 64 outputs along the line + 2 * 8 of halo, 64 lanes wide along x, of one channel (the
//                           channel is one more outer index): global accesses are runs of 64 consecutive doubles, LDS reads are
//                           conflict-free; cells outside the volume are 0.0.
//   LDS per workgroup: 8704 bytes for the x pass (4 waves x 2 lines x 272 floats), 40960 bytes for a line pass (80 x 64 doubles).
// lc_step_kernel: a workgroup of 256 threads walks a contiguous run of voxels in sweeps of 256 (walk_plan); the counts are kept per
// thread, added to LDS counters once per thread and flushed with one 64-bit atomic per counter and workgroup into the output, which
// the call zeroes first.
//   LDS per workgroup: 48 (six counters) + 256 (label table) = 304 bytes for the step.
//   A contribution to counts[4] is at most 2^28 and one to counts[5] at most 2^20; a volume has fewer than 2^31 voxels.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kLcMaxR = 8;    // the largest window radius
constexpr int kLcT = 256;     // threads of every workgroup here: 4 waves
constexpr int kLcXC = 256;    // x pass: outputs of one chunk of a row
constexpr int kLcLL = 64;     // line passes: outputs of one tile along the line
constexpr int kLcMaxBlocks = 2048;
constexpr int kLcPerThread = 8;

__device__ __forceinline__ bool lc_finite(float v) { return v - v == 0.f; }  // (false for a NaN and for +-inf)

struct MomArgs {
    int n, h, w;
    int r;     // the radius of this pass
    size_t N;  // voxels of one channel
};

__global__ __launch_bounds__(kLcT) void lc_moments_x_kernel(MomArgs a, const float* __restrict__ f, const float* __restrict__ m,
                                                           double* __restrict__ out) {
    __shared__ float tf[kLcT / 64][kLcXC + 2 * kLcMaxR];
    __shared__ float tm[kLcT / 64][kLcXC + 2 * kLcMaxR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = a.n * a.h, groups = (rows + kLcT / 64 - 1) / (kLcT / 64), r = a.r;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {  // (uniform trip counts: barriers inside)
        const int row = grp * (kLcT / 64) + wave;
        const bool live = row < rows;
        const size_t base = live ? (size_t)row * a.w : 0;
        for (int c0 = 0; c0 < a.w; c0 += kLcXC) {
            const int outs = a.w - c0 < kLcXC ? a.w - c0 : kLcXC;
            for (int i = lane; i < outs + 2 * r; i += 64) {
                const int x = c0 - r + i;
                float fv = NAN, mv = 0.f;
                if (live && x >= 0 && x < a.w) {
                    fv = f[base + x];
                    mv = m[base + x];
                    if (!lc_finite(fv) || !lc_finite(mv)) fv = NAN;  // not valid: the f cell says so
                }
                tf[wave][i] = fv;
                tm[wave][i] = mv;
            }
            __syncthreads();
            for (int i = lane; i < outs; i += 64) {
                if (!live) break;
                double s1 = 0.0, sf = 0.0, sm = 0.0, sff = 0.0, smm = 0.0, sfm = 0.0;
                for (int k = 0; k <= 2 * r; ++k) {
                    const float fc = tf[wave][i + k];
                    const bool ok = fc == fc;
                    const double fd = ok ? (double)fc : 0.0, md = ok ? (double)tm[wave][i + k] : 0.0;
                    s1 = s1 + (ok ? 1.0 : 0.0);
                    sf = sf + fd;
                    sm = sm + md;
                    sff = sff + fd * fd;
                    smm = smm + md * md;
                    sfm = sfm + fd * md;
                }
                const size_t o = base + c0 + i;
                out[o] = s1;
                out[a.N + o] = sf;
                out[2 * a.N + o] = sm;
                out[3 * a.N + o] = sff;
                out[4 * a.N + o] = smm;
                out[5 * a.N + o] = sfm;
            }
            __syncthreads();
        }
    }
}

// axis 1: lines along y (outer index: channel * n + z); axis 0: lines along z (outer index: channel * h + y)
__global__ __launch_bounds__(kLcT) void lc_moments_line_kernel(MomArgs a, int axis, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double t[(kLcLL + 2 * kLcMaxR) * 64];
    const int L = axis == 1 ? a.h : a.n, n_outer = 6 * (axis == 1 ? a.n : a.h), r = a.r;
    const int nxt = (a.w + 63) / 64, nlt = (L + kLcLL - 1) / kLcLL;
    const size_t sl = axis == 1 ? (size_t)a.w : (size_t)a.h * a.w;
    const long long tiles = (long long)n_outer * nlt * nxt;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform trip count: barriers inside)
        const int x0 = (int)(tile % nxt) * 64, l0 = (int)((tile / nxt) % nlt) * kLcLL, o = (int)(tile / ((long long)nxt * nlt));
        // the first element of the line: channel c and slice z (axis 1) or channel c and row y (axis 0)
        const size_t line = axis == 1 ? (size_t)o * a.h * a.w : (size_t)(o / a.h) * a.N + (size_t)(o % a.h) * a.w;
        const int outs = L - l0 < kLcLL ? L - l0 : kLcLL;
        for (int p = threadIdx.x; p < (outs + 2 * r) * 64; p += kLcT) {
            const int l = l0 - r + (p >> 6), x = x0 + (p & 63);
            t[p] = (x < a.w && l >= 0 && l < L) ? in[line + (size_t)l * sl + x] : 0.0;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < outs * 64; p += kLcT) {
            const int x = x0 + (p & 63);
            if (x >= a.w) continue;
            double acc = 0.0;
            for (int k = 0; k <= 2 * r; ++k) acc = acc + t[p + k * 64];
            out[line + (size_t)(l0 + (p >> 6)) * sl + x] = acc;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ the step
struct LccMap {
    double A[9], b[3], fs[3], gs[3];
    double inv_k2, den_min, var_eps, a_max;
    int e0, e1, e2;      // fixed extents
    int me0, me1, me2;   // moving extents (the outside test only)
    unsigned total;      // fixed voxels
    unsigned per_block;  // voxels per workgroup
    LabelTable keep;
};

__global__ __launch_bounds__(kLcT) void lc_step_kernel(LccMap q, const float* __restrict__ f, const float* __restrict__ m,
                                                      const double* __restrict__ S, const uint8_t* __restrict__ flab,
                                                      const float* __restrict__ u, float* __restrict__ out,
                                                      unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long cnt[6];
    __shared__ uint8_t table[256];
    const int tid = threadIdx.x;
    if (tid < 6) cnt[tid] = 0ull;
    stage_table(q.keep, table, tid);
    __syncthreads();

    unsigned c_sel = 0, c_in = 0, c_out = 0, c_nan = 0;
    unsigned long long c_d2 = 0ull, c_rho = 0ull;
    const size_t N = (size_t)q.total;
    const int fe[3] = {q.e0, q.e1, q.e2};
    const size_t stride[3] = {(size_t)q.e1 * q.e2, (size_t)q.e2, (size_t)1};
    const unsigned first = blockIdx.x * q.per_block;
    const unsigned last = min(q.total, first + q.per_block);
    for (unsigned p = first + (unsigned)tid; p < last; p += (unsigned)kLcT) {
        unsigned q0, q1, q2;
        index_split(p, (unsigned)q.e1, (unsigned)q.e2, q0, q1, q2);
        const int o[3] = {(int)q0, (int)q1, (int)q2};
        const float u0 = u[p], u1 = u[N + p], u2 = u[2 * N + p];
        float r0 = u0, r1 = u1, r2 = u2;
        if (!flab || table[flab[p]]) {
            ++c_sel;
            double p0 = (double)o[0], p1 = (double)o[1], p2 = (double)o[2], c[3];
            int j[3];
            displace(u, N, p, q.fs, p0, p1, p2);
            const float fv = f[p], mv = m[p];
            const double n1 = S[p];
            if (!affine_coord(q.A, q.b, p0, p1, p2, q.me0, q.me1, q.me2, c, j)) {
                ++c_out;
            } else if (!lc_finite(fv) || !lc_finite(mv) || !(n1 >= 2.0)) {
                ++c_nan;
            } else {
                const double sf = S[N + p], sm = S[2 * N + p], sff = S[3 * N + p], smm = S[4 * N + p], sfm = S[5 * N + p];
                const double mu_f = sf / n1, mu_m = sm / n1;
                const double c_fm = sfm - (sf * sm) / n1;
                const double c_mm = smm - (sm * sm) / n1;
                const double c_ff = sff - (sf * sf) / n1;
                double a = c_fm / (c_mm + q.var_eps * n1);
                a = a < 0.0 ? 0.0 : (a > q.a_max ? q.a_max : a);  // (a NaN stays a NaN)
                const double d = ((double)fv - mu_f) - a * ((double)mv - mu_m);
                double g[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const size_t hi = o[k] + 1 < fe[k] ? (size_t)p + stride[k] : (size_t)p;
                    const size_t lo = o[k] > 0 ? (size_t)p - stride[k] : (size_t)p;
                    g[k] = fe[k] == 1 ? 0.0 : a * (((double)m[hi] - (double)m[lo]) * q.gs[k]);
                }
                const double dd = d * d;
                const double den = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + dd * q.inv_k2;
                const bool still = den < q.den_min;
                const double s0 = still ? 0.0 : (d * g[0]) / den;
                const double s1 = still ? 0.0 : (d * g[1]) / den;
                const double s2 = still ? 0.0 : (d * g[2]) / den;
                if (a != a || den != den || s0 != s0 || s1 != s1 || s2 != s2) {
                    ++c_nan;
                } else {
                    r0 = (float)((double)u0 + s0);
                    r1 = (float)((double)u1 + s1);
                    r2 = (float)((double)u2 + s2);
                    ++c_in;
                    const double capped = dd < 16777216.0 ? dd : 16777216.0;
                    c_d2 += (unsigned long long)(long long)floor(capped * 16.0 + 0.5);
                    const double vv = c_mm * c_ff;
                    double rho2 = 0.0;
                    if (vv > 0.0) {
                        rho2 = (c_fm * c_fm) / vv;
                        rho2 = rho2 > 0.0 ? rho2 : 0.0;
                        rho2 = rho2 < 1.0 ? rho2 : 1.0;
                    }
                    c_rho += (unsigned long long)(long long)floor(rho2 * 1048576.0 + 0.5);
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
    if (c_rho) atomicAdd(&cnt[5], c_rho);
    __syncthreads();
    if (tid < 6 && cnt[tid]) atomicAdd(counts + tid, cnt[tid]);
}

}  // namespace

int local_moments(lm_engine* e, const float* f, const float* m, int n, int h, int w, const int32_t radius[3], double* out) {
    MomArgs a;
    a.n = n, a.h = h, a.w = w;
    a.N = (size_t)n * h * w;
    const double vox = (double)a.N;
    // the passes that run: x always (it forms the channels), y and z with a radius > 0 -- x -> y -> z, the last one into `out`
    const int line_axes[2] = {1, 0};
    int axes[2], nline = 0;
    for (int k = 0; k < 2; ++k)
        if (radius[line_axes[k]] > 0) axes[nline++] = line_axes[k];
    double* ws = nullptr;
    if (nline > 0) {
        LM_TRY(e->lcc.sums.reserve(6 * a.N * sizeof(double)));
        ws = e->lcc.sums.as<double>();
    }
    double* dst = nline == 1 ? ws : out;  // (two line passes: out, ws, out)
    {
        a.r = radius[2];
        ProfScope ps(e, "lcc_moments_x", vox * (8.0 + 48.0));
        const int groups = (n * h + kLcT / 64 - 1) / (kLcT / 64);
        LM_LAUNCH(lc_moments_x_kernel, dim3((unsigned)std::min(groups, 1 << 16)), dim3(kLcT), 0, e->stream, a, f, m, dst);
        LM_K(hipGetLastError());
    }
    for (int k = 0; k < nline; ++k) {
        const int axis = axes[k];
        const double* src = dst;
        dst = src == out ? ws : out;
        a.r = radius[axis];
        ProfScope ps(e, axis == 1 ? "lcc_moments_y" : "lcc_moments_z", vox * 96.0);
        const int L = axis == 1 ? h : n, n_outer = 6 * (axis == 1 ? n : h);
        const long long tiles = (long long)n_outer * ((L + kLcLL - 1) / kLcLL) * ((w + 63) / 64);
        LM_LAUNCH(lc_moments_line_kernel, dim3((unsigned)std::min<long long>(tiles, 1 << 20)), dim3(kLcT), 0, e->stream, a, axis, src, dst);
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

int lcc_step(lm_engine* e, const float* f, const float* m, const double* moments, const uint8_t* flab, int n, int h, int w, const float* u,
             const lm_lcc_params& p, float* out, int64_t* counts_out) {
    LccMap q;
    for (int i = 0; i < 9; ++i) q.A[i] = p.A[i];
    for (int i = 0; i < 3; ++i) q.b[i] = p.b[i], q.fs[i] = p.field_scale[i], q.gs[i] = p.grad_scale[i];
    q.inv_k2 = p.inv_k2, q.den_min = p.den_min, q.var_eps = p.var_eps, q.a_max = p.a_max;
    q.e0 = n, q.e1 = h, q.e2 = w;
    q.me0 = p.moving_dims[0], q.me1 = p.moving_dims[1], q.me2 = p.moving_dims[2];
    q.total = (unsigned)((size_t)n * h * w);
    q.keep = label_table(p.keep);
    const int blocks = walk_plan(q.total, kLcT, kLcPerThread, kLcMaxBlocks, q.per_block);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_out);
    LM_K(hipMemsetAsync(counts, 0, 6 * sizeof(unsigned long long), e->stream));
    // reads: f, m (and its six neighbours, from cache), the six sums, the labels, the field; writes: three components
    ProfScope ps(e, "lcc_step", (double)q.total * (4 + 4 + 48 + (flab ? 1 : 0) + 12 + 12));
    LM_LAUNCH(lc_step_kernel, dim3(blocks), dim3(kLcT), 0, e->stream, q, f, m, moments, flab, u, out, counts);
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace lm
