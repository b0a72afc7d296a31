// Hessian, eigenvalues and Frangi vesselness (lm_hessian_dev, lm_vesselness_dev, lm_vessel_counts_dev; include/lungmask_hip.h has the
// definitions).  Per scale three passes in lm_filter_dev's order x, y, z, each one lm_filter_dev's unmasked pass bit for bit
// (acc = fl32(acc + fl32(in * w)), taps ascending, indices clamped), but every pass applies up to three tap sets -- the Gaussian and
// its first and second derivative -- to what it has loaded once:
//   vessel_x_kernel   source (float)v -> X0, X1, X2 (x order 0, 1, 2).  A wave owns a row and walks it in chunks of 256 outputs.
//   vessel_y_kernel   X0 -> Y00, Y01, Y02; X1 -> Y10, Y11; X2 -> Y20 (Yab: x order a, y order b).  One LDS line tile (64 outputs + 2 r of
//                     halo, 64 lanes along x), loaded three times.
//   vessel_z_kernel   the same tile (32 outputs + halo) loaded six times: Hxx <- Y20, Hyy <- Y02, Hzz <- Y00 (z order 2), Hxy <- Y11,
//                     Hxz <- Y10 (z order 1), Hyz <- Y01 (z order 1), the six sums of a thread's 8 voxels in registers (constant
//                     indices only: no scratch).  Then, per voxel: scale normalisation, four cyclic Jacobi sweeps on fixed (p, q, r)
//                     triples, the sort by |lambda|, the vesselness, and the max-over-scales update of V and scale.  The components
//                     and the eigenvalues reach memory only for lm_hessian_dev.
// 20 volume transfers per scale (1 + 3, 3 + 6, 6 + 1) against the 36 of eighteen lm_filter_dev passes.
// All intermediate volumes are float32 volumes of the BOX: the volume, or with labels the box of the selection grown by the radii.
// The x pass reads the source with the index clamped to the volume; the line passes clamp to the box, which for every value a
// selected voxel depends on is the same index.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kMaxR = 32;
constexpr int kVT = 256;   // every kernel: 4 waves
constexpr int kVXC = 256;  // x pass: outputs of one chunk of a row
constexpr int kVLY = 64;   // y pass: outputs of one tile along the line
constexpr int kVLZ = 32;   // z pass: 32 x 64 outputs = 8 per thread, times six accumulators
constexpr int kVJ = kVLZ * 64 / kVT;

// the taps of one axis: w[order][k] = the tap of derivative order `order` at offset k - r.  ident: r == 0 and w[0][0] == 1, the pass
// lm_filter_dev skips -- order 0 is then the input itself
struct Taps3 {
    float w[3][2 * kMaxR + 1];
    int r, ident;
};

// ------------------------------------------------------------------------------------------------ x pass
struct XArgs {
    const void* vol;
    int dtype, H, W;  // the volume's rows and columns
    VolBox b;
    float *x0, *x1, *x2;  // box layout
};

__global__ __launch_bounds__(kVT) void vessel_x_kernel(XArgs a, Taps3 t) {
    __shared__ float tile[kVT / 64][kVXC + 2 * kMaxR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const VolBox b = a.b;
    const int rows = b.n * b.h, groups = (rows + kVT / 64 - 1) / (kVT / 64), r = t.r;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {  // (uniform trip counts: barriers inside)
        const int row = grp * (kVT / 64) + wave;
        const bool live = row < rows;
        const int z = live ? row / b.h : 0, y = live ? row - z * b.h : 0;
        const size_t src = ((size_t)(b.z0 + z) * a.H + (b.y0 + y)) * a.W;
        for (int c0 = 0; c0 < b.w; c0 += kVXC) {
            const int outs = b.w - c0 < kVXC ? b.w - c0 : kVXC;
            for (int i = lane; i < outs + 2 * r; i += 64) {
                int x = b.x0 + c0 - r + i;
                x = x < 0 ? 0 : (x >= a.W ? a.W - 1 : x);  // the VOLUME's border
                tile[wave][i] = live ? load_as<float>(a.vol, a.dtype, src + x) : 0.f;
            }
            __syncthreads();
            for (int i = lane; i < outs; i += 64) {
                if (!live) break;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
                for (int k = 0; k <= 2 * r; ++k) {
                    const float v = tile[wave][i + k];
                    s0 = s0 + v * t.w[0][k];
                    s1 = s1 + v * t.w[1][k];
                    s2 = s2 + v * t.w[2][k];
                }
                if (t.ident) s0 = tile[wave][i];
                const size_t o = (size_t)row * b.w + c0 + i;
                a.x0[o] = s0;
                a.x1[o] = s1;
                a.x2[o] = s2;
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------ line passes
// Tile geometry of a line pass over the box: axis 1 lines along y (outer index z), axis 0 lines along z (outer index y)
struct LineGeo {
    int L, n_outer;
    size_t so, sl;  // strides of the outer index and of the line index in the box
};

__device__ __forceinline__ LineGeo line_geo(const VolBox& b, int axis) {
    const size_t plane = (size_t)b.h * b.w;
    LineGeo g;
    g.L = axis == 1 ? b.h : b.n;
    g.n_outer = axis == 1 ? b.n : b.h;
    g.so = axis == 1 ? plane : (size_t)b.w;
    g.sl = axis == 1 ? (size_t)b.w : plane;
    return g;
}

// rows [l0 - r, l0 + outs + r) of the line, clamped to the box, 64 columns from x0: the tile of one source
__device__ __forceinline__ void load_line_tile(float* tile, const float* src, const LineGeo& g, int bw, int o, int l0, int x0, int outs, int r) {
    for (int p = threadIdx.x; p < (outs + 2 * r) * 64; p += kVT) {
        int l = l0 - r + (p >> 6);
        l = l < 0 ? 0 : (l >= g.L ? g.L - 1 : l);
        const int x = x0 + (p & 63);
        tile[p] = x < bw ? src[(size_t)o * g.so + (size_t)l * g.sl + x] : 0.f;
    }
}

struct YArgs {
    const float *x0, *x1, *x2;
    float *y00, *y01, *y02, *y10, *y11, *y20;
    VolBox b;
};

// orders 0 .. NOUT - 1 along y of one source
template <int NOUT>
__device__ __forceinline__ void y_outputs(const float* tile, const Taps3& t, const LineGeo& g, int bw, int o, int l0, int x0, int outs, float* o0,
                                          float* o1, float* o2) {
    const int r = t.r;
    for (int p = threadIdx.x; p < outs * 64; p += kVT) {
        const int x = x0 + (p & 63);
        if (x >= bw) continue;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int k = 0; k <= 2 * r; ++k) {
            const float v = tile[p + k * 64];
            s0 = s0 + v * t.w[0][k];
            if (NOUT > 1) s1 = s1 + v * t.w[1][k];
            if (NOUT > 2) s2 = s2 + v * t.w[2][k];
        }
        if (t.ident) s0 = tile[p];
        const size_t i = (size_t)o * g.so + (size_t)(l0 + (p >> 6)) * g.sl + x;
        o0[i] = s0;
        if (NOUT > 1) o1[i] = s1;
        if (NOUT > 2) o2[i] = s2;
    }
}

__global__ __launch_bounds__(kVT) void vessel_y_kernel(YArgs a, Taps3 t) {
    __shared__ float tile[(kVLY + 2 * kMaxR) * 64];
    const VolBox b = a.b;
    const LineGeo g = line_geo(b, 1);
    const int nxt = (b.w + 63) / 64, nlt = (g.L + kVLY - 1) / kVLY, r = t.r;
    const long long tiles = (long long)g.n_outer * nlt * nxt;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {  // (uniform trip count: barriers inside)
        const int x0 = (int)(tl % nxt) * 64, l0 = (int)((tl / nxt) % nlt) * kVLY, o = (int)(tl / ((long long)nxt * nlt));
        const int outs = g.L - l0 < kVLY ? g.L - l0 : kVLY;
        load_line_tile(tile, a.x0, g, b.w, o, l0, x0, outs, r);
        __syncthreads();
        y_outputs<3>(tile, t, g, b.w, o, l0, x0, outs, a.y00, a.y01, a.y02);
        __syncthreads();
        load_line_tile(tile, a.x1, g, b.w, o, l0, x0, outs, r);
        __syncthreads();
        y_outputs<2>(tile, t, g, b.w, o, l0, x0, outs, a.y10, a.y11, nullptr);
        __syncthreads();
        load_line_tile(tile, a.x2, g, b.w, o, l0, x0, outs, r);
        __syncthreads();
        y_outputs<1>(tile, t, g, b.w, o, l0, x0, outs, a.y20, nullptr, nullptr);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ analysis of one voxel
// One Jacobi rotation that annihilates a_pq; r is the third index.  Skipped for a_pq == 0.  (include/lungmask_hip.h: Eigenvalues)
__device__ __forceinline__ void jacobi_rotate(float& app, float& aqq, float& apq, float& arp, float& arq) {
    if (apq != 0.f) {
        const float theta = (aqq - app) / (2.f * apq);
        const float t = (theta < 0.f ? -1.f : 1.f) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
        const float c = 1.f / sqrtf(t * t + 1.f);
        const float s = t * c;
        const float tau = s / (1.f + c);
        const float h = t * apq;
        app = app - h;
        aqq = aqq + h;
        apq = 0.f;
        const float rp = arp, rq = arq;
        arp = rp - s * (rq + tau * rp);
        arq = rq + s * (rp - tau * rq);
    }
}

__device__ __forceinline__ void order_by_abs(float& a, float& b) {
    if (fabsf(a) > fabsf(b)) {
        const float c = a;
        a = b;
        b = c;
    }
}

// the eigenvalues of the symmetric matrix (index 0 = x, 1 = y, 2 = z), ascending |lambda|
__device__ __forceinline__ void eigenvalues3(float axx, float ayy, float azz, float axy, float axz, float ayz, float& l1, float& l2, float& l3) {
#pragma unroll
    for (int sweep = 0; sweep < 4; ++sweep) {
        jacobi_rotate(axx, ayy, axy, axz, ayz);  // (p, q, r) = (0, 1, 2)
        jacobi_rotate(axx, azz, axz, axy, ayz);  // (0, 2, 1)
        jacobi_rotate(ayy, azz, ayz, axy, axz);  // (1, 2, 0)
    }
    l1 = axx, l2 = ayy, l3 = azz;
    order_by_abs(l1, l2);
    order_by_abs(l2, l3);
    order_by_abs(l1, l2);
}

// exp(x) for x <= 0 (include/lungmask_hip.h: vexp); NaN gives NaN
__device__ __forceinline__ float vexp(float x) {
    if (x != x) return x;
    if (x < -87.f) return 0.f;
    const float k = rintf(x * 1.44269504f);
    const float r = (x - k * 0.693359375f) - k * -2.12194440e-4f;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = (p * (r * r) + r) + 1.f;
    const unsigned bits = (unsigned)((int)k + 127) << 23;  // 2^k, -126 <= k <= 0: a normal number, and so is the product
    float two_k;
    memcpy(&two_k, &bits, 4);
    return y * two_k;
}

__device__ __forceinline__ float frangi(float l1, float l2, float l3, float ka, float kb, float kc) {
    const float l23 = l2 * l3;
    if (!(l2 < 0.f && l3 < 0.f && l23 > 0.f)) return 0.f;
    const float a1 = l1 * l1, a2 = l2 * l2, a3 = l3 * l3;
    const float ra2 = a2 / a3, rb2 = a1 / l23, s2 = (a1 + a2) + a3;
    return ((1.f - vexp(-(ra2 * ka))) * vexp(-(rb2 * kb))) * (1.f - vexp(-(s2 * kc)));
}

// ------------------------------------------------------------------------------------------------ z pass + analysis
struct ZArgs {
    const float *y20, *y02, *y00, *y11, *y10, *y01;  // the sources of Hxx, Hyy, Hzz, Hxy, Hxz, Hyz
    VolBox b;
    int H, W;
    size_t nvox;
    const uint8_t* lab;
    LabelTable keep;
    float nrm[6];  // xx, yy, zz, xy, xz, yz
    int dark;
    float ka, kb, kc;
    float* comp;     // [6][n][h][w] or NULL
    float* eig;      // [3][n][h][w] or NULL
    float* V;        // [n][h][w] or NULL: the running maximum
    uint8_t* scale;  // or NULL
    int scale_index;  // 1-based
};

template <bool MASKED>
__global__ __launch_bounds__(kVT) void vessel_z_kernel(ZArgs a, Taps3 t) {
    __shared__ float tile[(kVLZ + 2 * kMaxR) * 64];
    __shared__ uint8_t keep[256];
    stage_table(a.keep, keep, threadIdx.x);
    __syncthreads();
    const VolBox b = a.b;
    const LineGeo g = line_geo(b, 0);
    const int nxt = (b.w + 63) / 64, nlt = (g.L + kVLZ - 1) / kVLZ, r = t.r;
    const long long tiles = (long long)g.n_outer * nlt * nxt;
    const int lx = threadIdx.x & 63, row0 = threadIdx.x >> 6;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {  // (uniform trip count: barriers inside)
        const int x0 = (int)(tl % nxt) * 64, l0 = (int)((tl / nxt) % nlt) * kVLZ, o = (int)(tl / ((long long)nxt * nlt));
        const int outs = g.L - l0 < kVLZ ? g.L - l0 : kVLZ;
        float acc[6][kVJ];  // (every index below is a constant once the loops are unrolled)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const float* src = c == 0 ? a.y20 : c == 1 ? a.y02 : c == 2 ? a.y00 : c == 3 ? a.y11 : c == 4 ? a.y10 : a.y01;
            const int order = c == 2 ? 2 : (c >= 4 ? 1 : 0);
            load_line_tile(tile, src, g, b.w, o, l0, x0, outs, r);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kVJ; ++j) {
                const int p = (row0 + 4 * j) * 64 + lx;
                float s = 0.f;
                if (row0 + 4 * j < outs) {
                    for (int k = 0; k <= 2 * r; ++k) s = s + tile[p + k * 64] * t.w[order][k];
                    if (order == 0 && t.ident) s = tile[p];
                }
                acc[c][j] = s;
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kVJ; ++j) {
            const int row = row0 + 4 * j, x = x0 + lx;
            if (row >= outs || x >= b.w) continue;
            const size_t v = ((size_t)(b.z0 + l0 + row) * a.H + (b.y0 + o)) * a.W + (b.x0 + x);
            if (MASKED && keep[a.lab[v]] == 0) continue;
            float hc[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) hc[c] = a.nrm[c] * (a.dark ? -acc[c][j] : acc[c][j]);
            if (a.comp) {
#pragma unroll
                for (int c = 0; c < 6; ++c) a.comp[(size_t)c * a.nvox + v] = hc[c];
            }
            if (!a.eig && !a.V) continue;
            float l1, l2, l3;
            eigenvalues3(hc[0], hc[1], hc[2], hc[3], hc[4], hc[5], l1, l2, l3);
            if (a.eig) {
                a.eig[v] = l1;
                a.eig[a.nvox + v] = l2;
                a.eig[2 * a.nvox + v] = l3;
            }
            if (a.V) {
                const float f = frangi(l1, l2, l3, a.ka, a.kb, a.kc);
                if (f > a.V[v]) {  // strictly greater: the first scale that attains the maximum keeps it
                    a.V[v] = f;
                    if (a.scale) a.scale[v] = (uint8_t)a.scale_index;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ counts
constexpr int kCountLabels = 16, kCountScales = 9;

__global__ __launch_bounds__(kVT) void vessel_counts_kernel(const float* V, const uint8_t* scale, const uint8_t* lab, size_t nvox, int n_labels,
                                                            float threshold, unsigned long long* cnt) {
    __shared__ unsigned hist[kCountLabels * kCountScales];
    for (int i = threadIdx.x; i < kCountLabels * kCountScales; i += kVT) hist[i] = 0u;
    __syncthreads();
    // (a workgroup adds fewer than 2^32 voxels: n * h * w < 2^31)
    for (size_t v = (size_t)blockIdx.x * kVT + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kVT) {
        const int l = lab[v], s = scale[v];
        if (l >= 1 && l < n_labels && s < kCountScales && V[v] >= threshold) atomicAdd(&hist[l * kCountScales + s], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCountLabels * kCountScales; i += kVT)
        if (hist[i]) atomicAdd(&cnt[i], (unsigned long long)hist[i]);
}

// ------------------------------------------------------------------------------------------------ host
Taps3 axis_taps(const lm_vessel_scale& sc, int axis) {
    Taps3 t;
    std::memset(&t, 0, sizeof t);
    t.r = sc.radius[axis];
    for (int o = 0; o < 3; ++o) std::memcpy(t.w[o], sc.taps[axis][o], sizeof(float) * (2 * t.r + 1));
    t.ident = (t.r == 0 && t.w[0][0] == 1.0f) ? 1 : 0;
    return t;
}

struct VesselOut {
    float *comp, *eig, *V;
    uint8_t* scale;
};

// one scale: the three passes over the box of the selection grown by this scale's radii
int vessel_scale(lm_engine* e, const void* vol, int dtype, const uint8_t* lab, int n, int h, int w, const lm_vessel_params& p, int si,
                 const int32_t bb[6], const VesselOut& out) {
    const lm_vessel_scale& sc = p.scales[si];
    const bool masked = (p.flags & LM_VESSEL_MASKED) != 0;
    const int dim[3] = {n, h, w};
    const double margin[3] = {(double)sc.radius[0], (double)sc.radius[1], (double)sc.radius[2]};
    const VolBox b = grown_box(bb, margin, dim);  // (unmasked: bb is the volume, which no margin grows)
    const size_t bvox = (size_t)b.n * b.h * b.w;
    VesselWorkspace& ws = e->vessel;
    float* f[9];
    for (int k = 0; k < 9; ++k) {
        LM_TRY(ws.vol[k].reserve(bvox * sizeof(float)));
        f[k] = ws.vol[k].as<float>();
    }
    const double vox = (double)bvox;
    {
        XArgs a;
        a.vol = vol, a.dtype = dtype, a.H = h, a.W = w, a.b = b;
        a.x0 = f[0], a.x1 = f[1], a.x2 = f[2];
        ProfScope ps(e, "vessel_x", vox * (dtype_bytes(dtype) + 12.0));
        const int groups = (b.n * b.h + kVT / 64 - 1) / (kVT / 64);
        LM_LAUNCH(vessel_x_kernel, dim3((unsigned)std::min(groups, 1 << 16)), dim3(kVT), 0, e->stream, a, axis_taps(sc, 2));
        LM_K(hipGetLastError());
    }
    {
        YArgs a;
        a.x0 = f[0], a.x1 = f[1], a.x2 = f[2];
        a.y00 = f[3], a.y01 = f[4], a.y02 = f[5], a.y10 = f[6], a.y11 = f[7], a.y20 = f[8];
        a.b = b;
        ProfScope ps(e, "vessel_y", vox * 36.0);
        const long long tiles = (long long)b.n * ((b.h + kVLY - 1) / kVLY) * ((b.w + 63) / 64);
        LM_LAUNCH(vessel_y_kernel, dim3((unsigned)std::min<long long>(tiles, 1 << 20)), dim3(kVT), 0, e->stream, a, axis_taps(sc, 1));
        LM_K(hipGetLastError());
    }
    {
        ZArgs a;
        std::memset(&a, 0, sizeof a);
        a.y20 = f[8], a.y02 = f[5], a.y00 = f[3], a.y11 = f[7], a.y10 = f[6], a.y01 = f[4];
        a.b = b, a.H = h, a.W = w, a.nvox = (size_t)n * h * w;
        a.lab = lab, a.keep = label_table(p.keep);
        std::memcpy(a.nrm, sc.nrm, sizeof a.nrm);
        a.dark = (p.flags & LM_VESSEL_DARK) ? 1 : 0;
        a.ka = p.ka, a.kb = p.kb, a.kc = p.kc;
        a.comp = out.comp, a.eig = out.eig, a.V = out.V, a.scale = out.scale, a.scale_index = si + 1;
        ProfScope ps(e, masked ? "vessel_z_masked" : "vessel_z", vox * (24.0 + (masked ? 1.0 : 0.0) + (out.V ? 9.0 : 36.0)));
        const long long tiles = (long long)b.h * ((b.n + kVLZ - 1) / kVLZ) * ((b.w + 63) / 64);
        const dim3 grid((unsigned)std::min<long long>(tiles, 1 << 20));
        if (masked) LM_LAUNCH((vessel_z_kernel<true>), grid, dim3(kVT), 0, e->stream, a, axis_taps(sc, 0));
        else LM_LAUNCH((vessel_z_kernel<false>), grid, dim3(kVT), 0, e->stream, a, axis_taps(sc, 0));
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

int vessel_run(lm_engine* e, const void* vol, int dtype, const uint8_t* lab, int n, int h, int w, const lm_vessel_params& p, const VesselOut& out,
               const char* entry) {
    if (n == 0) return LM_OK;
    const size_t nvox = (size_t)n * h * w;
    int32_t bb[6] = {0, n, 0, h, 0, w};
    if (p.flags & LM_VESSEL_MASKED) LM_TRY(roi_plan(e, lab, n, h, w, p.keep, bb, entry));
    // every voxel that is not analysed is 0; V and scale also start from 0 where it is
    if (out.V) LM_HIP(hipMemsetAsync(out.V, 0, nvox * sizeof(float), e->stream));
    if (out.scale) LM_HIP(hipMemsetAsync(out.scale, 0, nvox, e->stream));
    if (p.flags & LM_VESSEL_MASKED) {
        if (out.comp) LM_HIP(hipMemsetAsync(out.comp, 0, 6 * nvox * sizeof(float), e->stream));
        if (out.eig) LM_HIP(hipMemsetAsync(out.eig, 0, 3 * nvox * sizeof(float), e->stream));
    }
    for (int si = 0; si < p.n_scales; ++si) LM_TRY(vessel_scale(e, vol, dtype, lab, n, h, w, p, si, bb, out));
    return LM_OK;
}

}  // namespace

int hessian(lm_engine* e, const void* vol, int dtype, const uint8_t* lab, int n, int h, int w, const lm_vessel_params& p, float* comp, float* eig) {
    return vessel_run(e, vol, dtype, lab, n, h, w, p, VesselOut{comp, eig, nullptr, nullptr}, "lm_hessian_dev");
}

int vesselness(lm_engine* e, const void* vol, int dtype, const uint8_t* lab, int n, int h, int w, const lm_vessel_params& p, float* V, uint8_t* scale) {
    return vessel_run(e, vol, dtype, lab, n, h, w, p, VesselOut{nullptr, nullptr, V, scale}, "lm_vesselness_dev");
}

int vessel_counts(lm_engine* e, const float* V, const uint8_t* scale, const uint8_t* lab, int n, int h, int w, int n_labels, float threshold,
                  int64_t* counts) {
    const size_t nvox = (size_t)n * h * w, cells = (size_t)kCountLabels * kCountScales;
    std::memset(counts, 0, sizeof(int64_t) * (size_t)n_labels * kCountScales);
    if (nvox == 0) return LM_OK;
    VesselWorkspace& ws = e->vessel;
    LM_TRY(ws.cnt.reserve(cells * 8));
    LM_TRY(ws.h_cnt.reserve(cells * 8));
    unsigned long long* cnt = ws.cnt.as<unsigned long long>();
    LM_HIP(hipMemsetAsync(cnt, 0, cells * 8, e->stream));
    {
        ProfScope ps(e, "vessel_counts", (double)nvox * 6.0);
        const unsigned grid = (unsigned)std::min<size_t>((nvox + kVT - 1) / kVT, 2048);
        LM_LAUNCH(vessel_counts_kernel, dim3(grid), dim3(kVT), 0, e->stream, V, scale, lab, nvox, n_labels, threshold, cnt);
        LM_K(hipGetLastError());
    }
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, cells * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* hc = ws.h_cnt.as<unsigned long long>();
    for (int l = 0; l < n_labels; ++l)
        for (int s = 0; s < kCountScales; ++s) counts[l * kCountScales + s] = (int64_t)hc[l * kCountScales + s];
    return LM_OK;
}

}  // namespace lm
