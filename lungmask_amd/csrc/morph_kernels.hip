// Label morphology (lm_nearest_label_dev, lm_morph_dev; include/lungmask_hip.h): the nearest-label transform -- lm_edt_dev's three
// float32 min-plus passes carried out on pairs (squared distance, label), ordered lexicographically -- and on top of it dilation,
// erosion, opening and closing of a label selection by a ball of a radius in millimetres.
//
// Nearest-label transform.
//   x     nl_x_kernel: the search edt_x_kernel runs (volume_common.h: nearest_set_bits on the row's feature bits, 64-bit ballot words
//         in LDS), plus the label at each of the two bits; equal distances take the smaller label.
//   y, z  nl_line_kernel: edt_line_kernel's structure (a tile of whole lines in LDS, threads along x, the tile loaded completely before
//         anything is written, so the pass runs in place) with a u8 label tile beside the float tile.  The outward search stops only
//         when w * r^2 > best.d: fl(g + c) >= c, so nothing beyond that offset can reach best.d, but a candidate AT best.d can still
//         carry a smaller label.  Every candidate the search skips is strictly larger in d: the result is the lexicographic minimum
//         of the header's recursion, whatever the order of the search.
// Operators.  Everything runs inside the box of the selection grown by ceil(radius / s_i) + 1 voxels (exact: DESIGN.md 8h).  The
// distance-only transforms (erosion, the second half of opening and closing) are lm_edt_dev's kernels on a u8 feature volume that
// morph_feat_kernel writes; morph_apply_kernel compares the distance with the radius, writes the labels and counts the changes.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

// ------------------------------------------------------------------------------------------------ nearest-label transform
constexpr int kXT = 256;  // x pass: 4 waves, one row each

// (g1d, g1k)[z][y][x] = lexmin over the features x' of the row of (wx * (float)((x-x')^2), lab[x']); (+inf, 0) for a row without one.
// feature: keep[lab[(z0+z)][(y0+y)][(x0+x)]] != 0 (lab has the strides of the whole volume H x W; the outputs are box-shaped).
__global__ __launch_bounds__(kXT) void nl_x_kernel(const uint8_t* __restrict__ lab, int H, int W, VolBox b, LabelTable kb, float wx,
                                                  float* __restrict__ g1d, uint8_t* __restrict__ g1k) {
    __shared__ unsigned long long bits[kXT / 64][kMaxDim / 64];
    __shared__ uint8_t keep[256];
    stage_table(kb, keep, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrows = b.n * b.h, nwords = (b.w + 63) >> 6;
    for (int base = blockIdx.x * (kXT / 64); base < nrows; base += gridDim.x * (kXT / 64)) {  // (uniform trip count: barriers inside)
        const int row = base + wave;
        const bool live = row < nrows;
        const int z = live ? row / b.h : 0, y = live ? row - z * b.h : 0;
        const uint8_t* s = lab + ((size_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
        for (int c = 0; c < nwords; ++c) {
            const int x = c * 64 + lane;
            int f = 0;
            if (live && x < b.w) f = keep[s[x]];
            const unsigned long long word = __ballot(f);
            if (lane == 0) bits[wave][c] = word;
        }
        __syncthreads();
        if (live) {
            float* od = g1d + (size_t)row * b.w;
            uint8_t* ok = g1k + (size_t)row * b.w;
            for (int x = lane; x < b.w; x += 64) {
                int xl, xr;  // position of the nearest feature at or before x / after x
                nearest_set_bits(bits[wave], nwords, x, xl, xr);
                const int dl = xl >= 0 ? x - xl : INT_MAX, dr = xr >= 0 ? xr - x : INT_MAX;
                const int d = dl < dr ? dl : dr;
                int k = 0;
                if (d != INT_MAX) {
                    const int kl = dl == d ? (int)s[xl] : 256, kr = dr == d ? (int)s[xr] : 256;
                    k = kl < kr ? kl : kr;
                }
                od[x] = d == INT_MAX ? INFINITY : wx * (float)(d * d);
                ok[x] = (uint8_t)k;
            }
        }
        __syncthreads();
    }
}

constexpr int kLT = 512;      // line pass: 8 waves
constexpr int kTile = 16384;  // cells of LDS per workgroup: 64 KiB of distances + 16 KiB of labels (two workgroups = 16 waves per CU)

// In place on pairs: (f, k)[o][l][x] = lexmin over l' of (fl(f[o][l'][x] + fl(wgt * (float)((l - l')^2))), k[o][l'][x]), element
// (o, l, x) at o * so + l * sl + x.  y pass: o = z, so = h * w, sl = w;  z pass: o = y, so = w, sl = h * w.
__global__ __launch_bounds__(kLT) void nl_line_kernel(float* f, uint8_t* k, int n_outer, size_t so, size_t sl, int L, int w, int TX,
                                                     float wgt) {
    __shared__ float tile[kTile];
    __shared__ uint8_t ltile[kTile];
    const int nxt = (w + TX - 1) / TX;
    const long long tiles = (long long)n_outer * nxt;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int o = (int)(t / nxt), xb = (int)(t - (long long)o * nxt) * TX;
        const int tx = w - xb < TX ? w - xb : TX;  // columns of this tile
        const size_t base = (size_t)o * so + xb;
        const int cells = L * tx;
        for (int p = threadIdx.x; p < cells; p += kLT) {
            const int l = p / tx, x = p - l * tx;
            tile[p] = f[base + (size_t)l * sl + x];
            ltile[p] = k[base + (size_t)l * sl + x];
        }
        __syncthreads();
        for (int p = threadIdx.x; p < cells; p += kLT) {
            const int l = p / tx, x = p - l * tx;
            float best = tile[p];
            int bk = ltile[p];
            for (int r = 1; r < L; ++r) {
                const float c = wgt * (float)(r * r);
                if (c > best) break;  // every candidate from here on is >= c > best; one AT best may still carry a smaller label
                const int lo = l - r, hi = l + r;
                if (lo < 0 && hi >= L) break;
                if (lo >= 0) {
                    const float v = tile[lo * tx + x] + c;
                    const int vk = ltile[lo * tx + x];
                    if (v < best || (v == best && vk < bk)) best = v, bk = vk;
                }
                if (hi < L) {
                    const float v = tile[hi * tx + x] + c;
                    const int vk = ltile[hi * tx + x];
                    if (v < best || (v == best && vk < bk)) best = v, bk = vk;
                }
            }
            f[base + (size_t)l * sl + x] = best;
            k[base + (size_t)l * sl + x] = (uint8_t)bk;
        }
        __syncthreads();
    }
}

// the transform of the box `b` of lab (strides H x W) -> d2, near, both box-shaped
int nearest_box(lm_engine* e, const uint8_t* lab, int H, int W, const VolBox& b, const LabelTable& kb, const float wgt[3], float* d2,
                uint8_t* near) {
    const int nrows = b.n * b.h;
    {
        ProfScope ps(e, "nl_x", (double)nrows * b.w * 6.0);
        LM_LAUNCH(nl_x_kernel, dim3((unsigned)std::min((nrows + 3) / 4, 1 << 16)), dim3(kXT), 0, e->stream, lab, H, W, b, kb, wgt[2], d2, near);
        LM_K(hipGetLastError());
    }
    for (int axis = 1; axis >= 0; --axis) {  // y, then z
        const LinePass lp = line_pass_plan(b, axis, kTile);
        if (lp.L == 1) continue;
        ProfScope ps(e, axis == 1 ? "nl_y" : "nl_z", (double)nrows * b.w * 10.0);
        LM_LAUNCH(nl_line_kernel, dim3((unsigned)std::min<long long>(lp.tiles, 1 << 20)), dim3(kLT), 0, e->stream, d2, near, lp.n_outer,
                  lp.so, lp.sl, lp.L, b.w, lp.TX, wgt[axis]);
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------ operators
constexpr int kMT = 256;

enum { FEAT_NOT_KEPT, FEAT_D2_GT, FEAT_KEPT_D2_GT };

// The u8 feature volume of the next distance transform, box-shaped:
//   FEAT_NOT_KEPT     keep[lab] == 0               (the complement of the selection S)
//   FEAT_D2_GT        d2 > r2                      (the complement of D(S))
//   FEAT_KEPT_D2_GT   keep[lab] != 0 and d2 > r2   (E(S), d2 = distance to the complement of S)
__global__ __launch_bounds__(kMT) void morph_feat_kernel(const uint8_t* __restrict__ lab, int H, int W, VolBox b, LabelTable kb, int mode,
                                                        const float* __restrict__ d2, float r2, uint8_t* __restrict__ out) {
    __shared__ uint8_t keep[256];
    stage_table(kb, keep, threadIdx.x);
    __syncthreads();
    const int rows = b.n * b.h;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int z = row / b.h, y = row - z * b.h;
        const uint8_t* src = lab + ((size_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
        const size_t o = (size_t)row * b.w;
        for (int x = threadIdx.x; x < b.w; x += kMT) {
            bool f;
            if (mode == FEAT_NOT_KEPT) f = keep[src[x]] == 0;
            else if (mode == FEAT_D2_GT) f = !(d2[o + x] <= r2);
            else f = keep[src[x]] != 0 && !(d2[o + x] <= r2);
            out[o + x] = f ? (uint8_t)1 : (uint8_t)0;
        }
    }
}

// The last step of every operator, on the box: `hit` = (d2 <= r2) when le, else (d2 > r2).
//   grow   a voxel outside S with into[lab] != 0 and hit takes near            (dilate: le; close: d2 = distance to the complement of D)
//   else   a voxel of S with hit becomes 0                                      (erode: le; open: d2 = distance to E(S))
// Reads lab[v] before it writes out[v] and touches nothing else of either: out may be lab.  cnt[0] += added, cnt[1] += removed.
__global__ __launch_bounds__(kMT) void morph_apply_kernel(const uint8_t* lab, uint8_t* out, int H, int W, VolBox b, LabelTable kb, LabelTable ib,
                                                         int grow, int le, const float* __restrict__ d2, float r2,
                                                         const uint8_t* __restrict__ near, unsigned long long* cnt) {
    __shared__ uint8_t keep[256], into[256];
    __shared__ unsigned changed;
    stage_table(kb, keep, threadIdx.x);
    stage_table(ib, into, threadIdx.x);
    if (threadIdx.x == 0) changed = 0u;
    __syncthreads();
    unsigned mine = 0;
    const int rows = b.n * b.h;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int z = row / b.h, y = row - z * b.h;
        const size_t g = ((size_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
        const size_t o = (size_t)row * b.w;
        for (int x = threadIdx.x; x < b.w; x += kMT) {
            const uint8_t v = lab[g + x];
            const bool in_s = keep[v] != 0;
            const bool can = grow ? (!in_s && into[v] != 0) : in_s;
            if (!can) continue;
            const bool within = d2[o + x] <= r2;
            if (le ? within : !within) {
                out[g + x] = grow ? near[o + x] : (uint8_t)0;
                ++mine;
            }
        }
    }
    if (mine) atomicAdd(&changed, mine);
    __syncthreads();
    if (threadIdx.x == 0 && changed) atomicAdd(&cnt[grow ? 0 : 1], (unsigned long long)changed);
}

unsigned row_grid(const VolBox& b) { return (unsigned)std::max(1, std::min(b.n * b.h, 1 << 16)); }

int feat_pass(lm_engine* e, const uint8_t* lab, int H, int W, const VolBox& b, const LabelTable& kb, int mode, const float* d2, float r2,
              uint8_t* out) {
    ProfScope ps(e, "morph_feat", (double)b.n * b.h * b.w * (mode == FEAT_NOT_KEPT ? 2.0 : 6.0));
    LM_LAUNCH(morph_feat_kernel, dim3(row_grid(b)), dim3(kMT), 0, e->stream, lab, H, W, b, kb, mode, d2, r2, out);
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace

int nearest_label(lm_engine* e, const uint8_t* lab, int n, int h, int w, const uint8_t keep[256], const double* spacing, float* d2,
                  uint8_t* near) {
    if (n == 0) return LM_OK;
    if (!d2) {
        LM_TRY(e->morph.d2.reserve((size_t)n * h * w * sizeof(float)));
        d2 = e->morph.d2.as<float>();
    }
    float wgt[3];
    edt_weights(spacing, wgt);
    const VolBox b{0, 0, 0, n, h, w};
    return nearest_box(e, lab, h, w, b, label_table(keep), wgt, d2, near);
}

int morph(lm_engine* e, const uint8_t* lab, int n, int h, int w, const lm_morph_params& p, uint8_t* out, int64_t changed[2]) {
    changed[0] = changed[1] = 0;
    int32_t bb[6];
    LM_TRY(roi_plan(e, lab, n, h, w, p.keep, bb, "lm_morph_dev"));  // (n == 0: no kept voxel either)
    const size_t nvox = (size_t)n * h * w;
    if (out != lab) LM_HIP(hipMemcpyAsync(out, lab, nvox, hipMemcpyDeviceToDevice, e->stream));
    if (p.radius_mm == 0.0) return LM_OK;
    // the box of S grown by ceil(radius / s_i) + 1 voxels, clipped
    const int dim[3] = {n, h, w};
    double margin[3];
    for (int i = 0; i < 3; ++i) margin[i] = std::ceil(p.radius_mm / p.spacing[i]) + 1.0;  // (+inf for propagation)
    const VolBox b = grown_box(bb, margin, dim);
    const size_t bvox = (size_t)b.n * b.h * b.w;
    MorphWorkspace& ws = e->morph;
    LM_TRY(ws.d2.reserve(bvox * sizeof(float)));
    LM_TRY(ws.feat.reserve(bvox));
    LM_TRY(ws.cnt.reserve(16));
    LM_TRY(ws.h_cnt.reserve(16));
    const bool grow = p.op == LM_MORPH_DILATE || p.op == LM_MORPH_CLOSE;
    if (grow) LM_TRY(ws.near.reserve(bvox));
    float* d2 = ws.d2.as<float>();
    uint8_t *feat = ws.feat.as<uint8_t>(), *near = ws.near.as<uint8_t>();
    unsigned long long* cnt = ws.cnt.as<unsigned long long>();
    LM_HIP(hipMemsetAsync(cnt, 0, 16, e->stream));
    float wgt[3];
    edt_weights(p.spacing, wgt);
    const float r2 = (float)(p.radius_mm * p.radius_mm);
    const LabelTable kb = label_table(p.keep), ib = label_table(p.into);
    int le = 1;
    switch (p.op) {
        case LM_MORPH_DILATE:
            LM_TRY(nearest_box(e, lab, h, w, b, kb, wgt, d2, near));
            break;
        case LM_MORPH_ERODE:
            LM_TRY(feat_pass(e, lab, h, w, b, kb, FEAT_NOT_KEPT, nullptr, 0.f, feat));
            LM_TRY(edt(e, feat, b.n, b.h, b.w, p.spacing, d2));
            break;
        case LM_MORPH_OPEN:  // D(E(S)): distance to the complement of S -> E(S) -> distance to E(S)
            LM_TRY(feat_pass(e, lab, h, w, b, kb, FEAT_NOT_KEPT, nullptr, 0.f, feat));
            LM_TRY(edt(e, feat, b.n, b.h, b.w, p.spacing, d2));
            LM_TRY(feat_pass(e, lab, h, w, b, kb, FEAT_KEPT_D2_GT, d2, r2, feat));
            LM_TRY(edt(e, feat, b.n, b.h, b.w, p.spacing, d2));
            le = 0;
            break;
        default:  // LM_MORPH_CLOSE, E(D(S)): distance to S (and its nearest label) -> complement of D(S) -> distance to that
            LM_TRY(nearest_box(e, lab, h, w, b, kb, wgt, d2, near));
            LM_TRY(feat_pass(e, lab, h, w, b, kb, FEAT_D2_GT, d2, r2, feat));
            LM_TRY(edt(e, feat, b.n, b.h, b.w, p.spacing, d2));
            le = 0;
            break;
    }
    {
        ProfScope ps(e, "morph_apply", (double)bvox * 7.0);
        LM_LAUNCH(morph_apply_kernel, dim3(row_grid(b)), dim3(kMT), 0, e->stream, lab, out, h, w, b, kb, ib, grow ? 1 : 0, le,
                  (const float*)d2, r2, (const uint8_t*)near, cnt);
        LM_K(hipGetLastError());
    }
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, 16, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* hc = ws.h_cnt.as<unsigned long long>();
    changed[0] = (int64_t)hc[0];
    changed[1] = (int64_t)hc[1];
    return LM_OK;
}

}  // namespace lm
