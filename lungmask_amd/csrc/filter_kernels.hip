// Lung-aware image filters (lm_filter_dev; include/lungmask_hip.h has the definitions): the median of a window of 1, 3 or 5 voxels
// per axis and a separable convolution with caller-supplied taps of radius <= 32, each either over the whole volume (indices
// clamped) or confined by the labels to a selection (nothing exists outside it).
//
// Median.
//   median_kernel   a workgroup owns 8 x 8 x 64 voxels and loads them with the window's halo ONCE into an LDS tile of order-preserving
//                   32-bit keys (12 x 12 x 68 cells at most: 39 KB) and a u8 tile of flags (bit 0: the cell contributes -- inside the
//                   volume or clamped into it, selected, not NaN; bit 1: the cell is selected).  The element of rank (cnt - 1) / 2 is
//                   found by a bitwise radix select, most significant bit first: count the live cells whose bit is 0, keep them when
//                   the rank falls among them, otherwise drop them and lower the rank.  No per-thread array, hence no scratch.
//                   3 x 3 x 3 (REG3): the 27 keys are read once into registers (constant indices) and the select runs on a 27-bit
//                   "alive" mask; other windows read the tile in every bit pass.  int16 keys have 16 bits, i.e. 16 passes.
// Separable.  One kernel per pass (x, y, z; a pass with r == 0 and w[0] == 1 is skipped), each from a tile with the halo of the
// filtered axis, out-of-range cells CLAMPED (unmasked) or ZERO (masked), so the tap loop has no bounds check:
//   sep_x_kernel     a wave owns a row and walks it in chunks of 256 outputs (tile: 256 + 2 r floats, lanes along x: coalesced).
//   sep_line_kernel  y and z: a tile of 64 outputs along the line + 2 r of halo, 64 lanes wide along x, so global accesses are runs of
//                    64 consecutive floats and LDS reads are conflict-free.
//   The masked form carries num and den through the same kernel in two tiles and two accumulators; the first pass reads the
//   source and the labels (num = selected ? (float)v : 0, den = selected ? 1 : 0), the last one divides and writes the selected
//   voxels only.  It works inside the box of the selection grown by the radii (exact: DESIGN.md 8j); filter_fill_kernel has written
//   every other voxel before.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kMaxR = 32;

struct Indicator {
    int on, lo, hi;
};

// the source value of voxel v as the separable filter sees it: (float)v, or the indicator of ind.lo <= hu <= ind.hi
__device__ __forceinline__ float load_src(const void* vol, int dtype, size_t v, const Indicator& ind) {
    if (ind.on) {
        bool nan;
        const int hu = load_hu(vol, dtype, v, nan);
        return (!nan && ind.lo <= hu && hu <= ind.hi) ? 1.f : 0.f;
    }
    return load_as<float>(vol, dtype, v);
}

// ------------------------------------------------------------------------------------------------ median
constexpr int kMT = 256;
constexpr int kMBZ = 8, kMBY = 8, kMBX = 64;                          // voxels of a workgroup
constexpr int kMCells = (kMBZ + 4) * (kMBY + 4) * (kMBX + 4);         // with the halo of a window of 5

// order-preserving keys: ascending key == ascending value, -0.0 before +0.0; enc and dec are inverse bijections on the bit patterns
template <class T> struct Key;
template <> struct Key<int16_t> {
    static constexpr int bits = 16;
    static __device__ __forceinline__ unsigned enc(int16_t v) { return (unsigned)(uint16_t)v ^ 0x8000u; }
    static __device__ __forceinline__ int16_t dec(unsigned k) { return (int16_t)(uint16_t)(k ^ 0x8000u); }
    static __device__ __forceinline__ bool nan(int16_t) { return false; }
    static __device__ __forceinline__ int16_t empty(int16_t centre) { return centre; }
    static __device__ __forceinline__ int16_t cast(float f) { return (int16_t)f; }
};
template <> struct Key<int32_t> {
    static constexpr int bits = 32;
    static __device__ __forceinline__ unsigned enc(int32_t v) { return (unsigned)v ^ 0x80000000u; }
    static __device__ __forceinline__ int32_t dec(unsigned k) { return (int32_t)(k ^ 0x80000000u); }
    static __device__ __forceinline__ bool nan(int32_t) { return false; }
    static __device__ __forceinline__ int32_t empty(int32_t centre) { return centre; }
    static __device__ __forceinline__ int32_t cast(float f) { return (int32_t)f; }
};
template <> struct Key<float> {
    static constexpr int bits = 32;
    static __device__ __forceinline__ unsigned enc(float v) {
        unsigned b;
        memcpy(&b, &v, 4);
        return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    }
    static __device__ __forceinline__ float dec(unsigned k) {
        const unsigned b = (k >> 31) ? (k ^ 0x80000000u) : ~k;
        float v;
        memcpy(&v, &b, 4);
        return v;
    }
    static __device__ __forceinline__ bool nan(float v) { return v != v; }
    static __device__ __forceinline__ float empty(float) { return dec(0xffc00000u); }  // cnt == 0: the quiet NaN 0x7fc00000
    static __device__ __forceinline__ float cast(float f) { return f; }
};

struct MedArgs {
    const void* vol;
    void* out;
    const uint8_t* lab;
    int n, h, w;
    int hz, hy, hx;  // half windows: 0, 1 or 2
    int masked, fill_outside;
    float fill;
    LabelTable keep;
};

template <class T, bool REG3>
__global__ __launch_bounds__(kMT) void median_kernel(MedArgs a) {
    __shared__ unsigned tk[kMCells];
    __shared__ uint8_t tv[kMCells];
    __shared__ uint8_t keep[256];
    stage_table(a.keep, keep, threadIdx.x);
    __syncthreads();
    const T* vol = static_cast<const T*>(a.vol);
    T* out = static_cast<T*>(a.out);
    const int TX = kMBX + 2 * a.hx, TY = kMBY + 2 * a.hy, TZ = kMBZ + 2 * a.hz;
    const int cells = TZ * TY * TX;  // <= kMCells: every half window <= 2
    const int nbx = (a.w + kMBX - 1) / kMBX, nby = (a.h + kMBY - 1) / kMBY, nbz = (a.n + kMBZ - 1) / kMBZ;
    const long long blocks = (long long)nbx * nby * nbz;
    const int lx = threadIdx.x & 63, g = threadIdx.x >> 6;
    for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {  // (uniform trip count: barriers inside)
        const int bx = (int)(blk % nbx), by = (int)((blk / nbx) % nby), bz = (int)(blk / ((long long)nbx * nby));
        const int x0 = bx * kMBX, y0 = by * kMBY, z0 = bz * kMBZ;
        for (int c = threadIdx.x; c < cells; c += kMT) {
            const int cx = c % TX, cy = (c / TX) % TY, cz = c / (TX * TY);
            int gz = z0 - a.hz + cz, gy = y0 - a.hy + cy, gx = x0 - a.hx + cx;
            bool in = gz >= 0 && gz < a.n && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
            if (!a.masked) {  // scipy's mode="nearest"
                gz = gz < 0 ? 0 : (gz >= a.n ? a.n - 1 : gz);
                gy = gy < 0 ? 0 : (gy >= a.h ? a.h - 1 : gy);
                gx = gx < 0 ? 0 : (gx >= a.w ? a.w - 1 : gx);
                in = true;
            }
            unsigned key = 0u, flags = 0u;
            if (in) {
                const size_t v = ((size_t)gz * a.h + gy) * a.w + gx;
                const T s = vol[v];
                const bool sel = !a.masked || keep[a.lab[v]] != 0;
                key = Key<T>::enc(s);
                flags = (sel && !Key<T>::nan(s) ? 1u : 0u) | (sel ? 2u : 0u);
            }
            tk[c] = key;
            tv[c] = (uint8_t)flags;
        }
        __syncthreads();
        for (int j = 0; j < kMBZ * kMBY / 4; ++j) {
            const int p = g + 4 * j, zz = p >> 3, yy = p & 7;
            const int z = z0 + zz, y = y0 + yy, x = x0 + lx;
            if (z >= a.n || y >= a.h || x >= a.w) continue;
            const size_t v = ((size_t)z * a.h + y) * a.w + x;
            const int cc = ((zz + a.hz) * TY + (yy + a.hy)) * TX + lx + a.hx;
            const T centre = Key<T>::dec(tk[cc]);
            if (!(tv[cc] & 2u)) {  // not selected (masked mode only)
                out[v] = a.fill_outside ? Key<T>::cast(a.fill) : centre;
                continue;
            }
            unsigned res = 0u;
            int cnt = 0;
            if (REG3) {
                unsigned k[27];
                unsigned alive = 0u;
#pragma unroll
                for (int i = 0; i < 27; ++i) {
                    const int c = ((zz + i / 9) * (kMBY + 2) + (yy + (i / 3) % 3)) * (kMBX + 2) + lx + i % 3;
                    k[i] = tk[c];
                    alive |= (unsigned)(tv[c] & 1u) << i;
                }
                cnt = __popc(alive);
                int rank = (cnt - 1) >> 1;
                for (int b = Key<T>::bits - 1; b >= 0; --b) {
                    unsigned ones = 0u;
#pragma unroll
                    for (int i = 0; i < 27; ++i) ones |= ((k[i] >> b) & 1u) << i;
                    const unsigned zeros = alive & ~ones;
                    const int c0 = __popc(zeros);
                    if (rank < c0) alive = zeros;
                    else {
                        rank -= c0;
                        alive &= ones;
                        res |= 1u << b;
                    }
                }
            } else {
                const int wz = 2 * a.hz + 1, wy = 2 * a.hy + 1, wx = 2 * a.hx + 1;
                const int base = (zz * TY + yy) * TX + lx;  // the window's first cell
                for (int dz = 0; dz < wz; ++dz)
                    for (int dy = 0; dy < wy; ++dy)
                        for (int dx = 0; dx < wx; ++dx) cnt += tv[base + (dz * TY + dy) * TX + dx] & 1u;
                int rank = (cnt - 1) >> 1;
                for (int b = Key<T>::bits - 1; b >= 0; --b) {
                    const unsigned above = ~((2u << b) - 1u);  // the bits above b: a live cell agrees with res there
                    int c0 = 0;
                    for (int dz = 0; dz < wz; ++dz)
                        for (int dy = 0; dy < wy; ++dy)
                            for (int dx = 0; dx < wx; ++dx) {
                                const int c = base + (dz * TY + dy) * TX + dx;
                                const unsigned kc = tk[c];
                                c0 += ((tv[c] & 1u) && ((kc ^ res) & above) == 0u && !((kc >> b) & 1u)) ? 1 : 0;
                            }
                    if (rank >= c0) {
                        rank -= c0;
                        res |= 1u << b;
                    }
                }
            }
            out[v] = cnt > 0 ? Key<T>::dec(res) : Key<T>::empty(centre);
        }
        __syncthreads();
    }
}

template <class T>
int median_launch(lm_engine* e, const MedArgs& a) {
    const long long blocks = (long long)((a.w + kMBX - 1) / kMBX) * ((a.h + kMBY - 1) / kMBY) * ((a.n + kMBZ - 1) / kMBZ);
    const dim3 grid((unsigned)std::min<long long>(blocks, 1 << 16));
    const double bytes = (double)a.n * a.h * a.w * (2.0 * sizeof(T) + (a.masked ? 1.0 : 0.0));
    if (a.hz == 1 && a.hy == 1 && a.hx == 1) {
        ProfScope ps(e, "median_333", bytes);
        LM_LAUNCH((median_kernel<T, true>), grid, dim3(kMT), 0, e->stream, a);
    } else {
        ProfScope ps(e, "median_tile", bytes);
        LM_LAUNCH((median_kernel<T, false>), grid, dim3(kMT), 0, e->stream, a);
    }
    LM_K(hipGetLastError());
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------ separable
struct Taps {
    float w[2 * kMaxR + 1];  // w[k]: the tap at offset k - r
    int r;
};

// One pass over the box (n, h, w).  Element (z, y, x) of an array lies at off + z * sz + y * sy + x of it.
struct SepArgs {
    const void* src;  // first pass: the source volume of `dtype`; otherwise the float32 num of the previous pass
    const float* den_in;
    const uint8_t* lab;  // masked: the labels (first pass: the selection; last pass: which voxels are written)
    float* num_out;      // last pass: the output volume
    float* den_out;
    size_t in_sz, in_sy, in_off;
    size_t lab_sz, lab_sy, lab_off;
    size_t out_sz, out_sy, out_off;
    int n, h, w;
    int dtype, first, last;
    Indicator ind;
    LabelTable keep;
};

template <bool MASKED>
__device__ __forceinline__ void sep_load(const SepArgs& a, const uint8_t* keep, int z, int y, int x, float& num, float& den) {
    const size_t i = a.in_off + (size_t)z * a.in_sz + (size_t)y * a.in_sy + x;
    den = 0.f;
    if (a.first) {
        num = load_src(a.src, a.dtype, i, a.ind);
        if (MASKED) {
            const bool sel = keep[a.lab[a.lab_off + (size_t)z * a.lab_sz + (size_t)y * a.lab_sy + x]] != 0;
            num = sel ? num : 0.f;
            den = sel ? 1.f : 0.f;
        }
    } else {
        num = static_cast<const float*>(a.src)[i];
        if (MASKED) den = a.den_in[i];
    }
}

template <bool MASKED>
__device__ __forceinline__ void sep_store(const SepArgs& a, const uint8_t* keep, int z, int y, int x, float num, float den) {
    const size_t o = a.out_off + (size_t)z * a.out_sz + (size_t)y * a.out_sy + x;
    if (!MASKED) a.num_out[o] = num;
    else if (!a.last) {
        a.num_out[o] = num;
        a.den_out[o] = den;
    } else if (keep[a.lab[a.lab_off + (size_t)z * a.lab_sz + (size_t)y * a.lab_sy + x]] != 0) a.num_out[o] = num / den;
}

constexpr int kST = 256;  // both pass kernels: 4 waves
constexpr int kXC = 256;  // x pass: outputs of one chunk of a row

template <bool MASKED>
__global__ __launch_bounds__(kST) void sep_x_kernel(SepArgs a, Taps t) {
    __shared__ float tn[kST / 64][kXC + 2 * kMaxR];
    __shared__ float td[MASKED ? kST / 64 : 1][MASKED ? kXC + 2 * kMaxR : 1];
    __shared__ uint8_t keep[256];
    stage_table(a.keep, keep, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = a.n * a.h, groups = (rows + kST / 64 - 1) / (kST / 64), r = t.r;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {  // (uniform trip counts: barriers inside)
        const int row = grp * (kST / 64) + wave;
        const bool live = row < rows;
        const int z = live ? row / a.h : 0, y = live ? row - z * a.h : 0;
        for (int c0 = 0; c0 < a.w; c0 += kXC) {
            const int outs = a.w - c0 < kXC ? a.w - c0 : kXC;
            for (int i = lane; i < outs + 2 * r; i += 64) {
                int x = c0 - r + i;
                float num = 0.f, den = 0.f;
                if (live) {
                    if (!MASKED) x = x < 0 ? 0 : (x >= a.w ? a.w - 1 : x);
                    if (x >= 0 && x < a.w) sep_load<MASKED>(a, keep, z, y, x, num, den);
                }
                tn[wave][i] = num;
                if (MASKED) td[wave][i] = den;
            }
            __syncthreads();
            for (int i = lane; i < outs; i += 64) {
                if (!live) break;
                float num = 0.f, den = 0.f;
                for (int k = 0; k <= 2 * r; ++k) {
                    num = num + tn[wave][i + k] * t.w[k];
                    if (MASKED) den = den + td[wave][i + k] * t.w[k];
                }
                sep_store<MASKED>(a, keep, z, y, c0 + i, num, den);
            }
            __syncthreads();
        }
    }
}

constexpr int kLL = 64;  // line passes: outputs of one tile along the line

// axis 1: lines along y (outer index z); axis 0: lines along z (outer index y)
template <bool MASKED>
__global__ __launch_bounds__(kST) void sep_line_kernel(SepArgs a, Taps t, int axis) {
    __shared__ float tn[(kLL + 2 * kMaxR) * 64];
    __shared__ float td[MASKED ? (kLL + 2 * kMaxR) * 64 : 1];
    __shared__ uint8_t keep[256];
    stage_table(a.keep, keep, threadIdx.x);
    __syncthreads();
    const int L = axis == 1 ? a.h : a.n, n_outer = axis == 1 ? a.n : a.h, r = t.r;
    const int nxt = (a.w + 63) / 64, nlt = (L + kLL - 1) / kLL;
    const long long tiles = (long long)n_outer * nlt * nxt;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform trip count: barriers inside)
        const int x0 = (int)(tile % nxt) * 64, l0 = (int)((tile / nxt) % nlt) * kLL, o = (int)(tile / ((long long)nxt * nlt));
        const int outs = L - l0 < kLL ? L - l0 : kLL;
        for (int p = threadIdx.x; p < (outs + 2 * r) * 64; p += kST) {
            int l = l0 - r + (p >> 6);
            const int x = x0 + (p & 63);
            float num = 0.f, den = 0.f;
            if (x < a.w) {
                if (!MASKED) l = l < 0 ? 0 : (l >= L ? L - 1 : l);
                if (l >= 0 && l < L) sep_load<MASKED>(a, keep, axis == 1 ? o : l, axis == 1 ? l : o, x, num, den);
            }
            tn[p] = num;
            if (MASKED) td[p] = den;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < outs * 64; p += kST) {
            const int x = x0 + (p & 63);
            if (x >= a.w) continue;
            float num = 0.f, den = 0.f;
            for (int k = 0; k <= 2 * r; ++k) {
                num = num + tn[p + k * 64] * t.w[k];
                if (MASKED) den = den + td[p + k * 64] * t.w[k];
            }
            const int l = l0 + (p >> 6);
            sep_store<MASKED>(a, keep, axis == 1 ? o : l, axis == 1 ? l : o, x, num, den);
        }
        __syncthreads();
    }
}

// out[v] = (float)v (or its indicator); with fill_outside, `fill` where the voxel is not selected.  The whole volume: the masked
// passes overwrite the selected voxels afterwards, and with every pass skipped this IS the result.
__global__ __launch_bounds__(kST) void filter_fill_kernel(const void* vol, int dtype, const uint8_t* lab, size_t nvox, Indicator ind,
                                                          LabelTable kb, int fill_outside, float fill, float* out) {
    __shared__ uint8_t keep[256];
    stage_table(kb, keep, threadIdx.x);
    __syncthreads();
    for (size_t v = (size_t)blockIdx.x * kST + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kST)
        out[v] = (fill_outside && keep[lab[v]] == 0) ? fill : load_src(vol, dtype, v, ind);
}

template <bool MASKED>
int sep_pass(lm_engine* e, int axis, const SepArgs& a, const Taps& t) {
    static const char* const names[2][3] = {{"sep_z", "sep_y", "sep_x"}, {"sep_z_masked", "sep_y_masked", "sep_x_masked"}};
    const double vox = (double)a.n * a.h * a.w;
    const double in_bytes = a.first ? dtype_bytes(a.dtype) + (MASKED ? 1.0 : 0.0) : (MASKED ? 8.0 : 4.0);
    ProfScope ps(e, names[MASKED ? 1 : 0][axis], vox * (in_bytes + ((MASKED && !a.last) ? 8.0 : 4.0)));
    if (axis == 2) {
        const int groups = (a.n * a.h + kST / 64 - 1) / (kST / 64);
        LM_LAUNCH((sep_x_kernel<MASKED>), dim3((unsigned)std::min(groups, 1 << 16)), dim3(kST), 0, e->stream, a, t);
    } else {
        const int L = axis == 1 ? a.h : a.n, n_outer = axis == 1 ? a.n : a.h;
        const long long tiles = (long long)n_outer * ((L + kLL - 1) / kLL) * ((a.w + 63) / 64);
        LM_LAUNCH((sep_line_kernel<MASKED>), dim3((unsigned)std::min<long long>(tiles, 1 << 20)), dim3(kST), 0, e->stream, a, t, axis);
    }
    LM_K(hipGetLastError());
    return LM_OK;
}

}  // namespace

int filter(lm_engine* e, const void* vol, int dtype, const uint8_t* lab, int n, int h, int w, const lm_filter_params& p, void* out) {
    if (n == 0) return LM_OK;
    const bool masked = (p.flags & LM_FILTER_MASKED) != 0;
    const int fill_outside = masked && (p.flags & LM_FILTER_FILL_OUTSIDE) ? 1 : 0;
    const size_t nvox = (size_t)n * h * w;
    const LabelTable kb = label_table(p.keep);
    int32_t bb[6] = {0, n, 0, h, 0, w};
    if (masked) LM_TRY(roi_plan(e, lab, n, h, w, p.keep, bb, "lm_filter_dev"));
    if (p.kind == LM_FILTER_MEDIAN) {
        MedArgs a;
        a.vol = vol, a.out = out, a.lab = lab;
        a.n = n, a.h = h, a.w = w;
        a.hz = p.size[0] >> 1, a.hy = p.size[1] >> 1, a.hx = p.size[2] >> 1;
        a.masked = masked ? 1 : 0, a.fill_outside = fill_outside, a.fill = p.fill;
        a.keep = kb;
        return dtype == LM_I16 ? median_launch<int16_t>(e, a) : dtype == LM_I32 ? median_launch<int32_t>(e, a) : median_launch<float>(e, a);
    }
    // the passes that run, in the order x, y, z
    int axes[3], npass = 0;
    for (int axis = 2; axis >= 0; --axis)
        if (!(p.radius[axis] == 0 && p.taps[axis][0] == 1.0f)) axes[npass++] = axis;
    const Indicator ind{(p.flags & LM_FILTER_INDICATOR) ? 1 : 0, p.ind_lo, p.ind_hi};
    float* outf = static_cast<float*>(out);
    if (masked || npass == 0) {
        ProfScope ps(e, "filter_fill", (double)nvox * 7.0);
        const unsigned grid = (unsigned)std::min<size_t>((nvox + kST - 1) / kST, 1 << 16);
        LM_LAUNCH(filter_fill_kernel, dim3(grid), dim3(kST), 0, e->stream, vol, dtype, lab, nvox, ind, kb, fill_outside, p.fill, outf);
        LM_K(hipGetLastError());
    }
    if (npass == 0) return LM_OK;
    // the box the passes work in: the selection grown by the radii (masked; exact), otherwise the volume
    const int dim[3] = {n, h, w};
    const double margin[3] = {(double)p.radius[0], (double)p.radius[1], (double)p.radius[2]};
    const VolBox b = grown_box(bb, margin, dim);  // (unmasked: bb is the volume, which no margin grows)
    const size_t bvox = (size_t)b.n * b.h * b.w;
    FilterWorkspace& ws = e->filter;
    const int nbuf = masked ? std::min(npass - 1, 2) : (npass > 1 ? 1 : 0);
    for (int k = 0; k < nbuf; ++k) {
        LM_TRY(ws.num[k].reserve(bvox * sizeof(float)));
        if (masked) LM_TRY(ws.den[k].reserve(bvox * sizeof(float)));
    }
    const size_t vol_sz = (size_t)h * w, vol_sy = (size_t)w, vol_off = ((size_t)b.z0 * h + b.y0) * w + b.x0;
    const size_t box_sz = (size_t)b.h * b.w, box_sy = (size_t)b.w;
    SepArgs a;
    std::memset(&a, 0, sizeof a);
    a.lab = lab;
    a.lab_sz = vol_sz, a.lab_sy = vol_sy, a.lab_off = vol_off;
    a.n = b.n, a.h = b.h, a.w = b.w;
    a.dtype = dtype, a.ind = ind, a.keep = kb;
    const float* prev_num = nullptr;
    const float* prev_den = nullptr;
    for (int i = 0; i < npass; ++i) {
        const int axis = axes[i];
        a.first = i == 0, a.last = i == npass - 1;
        if (a.first) a.src = vol, a.den_in = nullptr, a.in_sz = vol_sz, a.in_sy = vol_sy, a.in_off = vol_off;
        else a.src = prev_num, a.den_in = prev_den, a.in_sz = box_sz, a.in_sy = box_sy, a.in_off = 0;
        // the unmasked passes alternate between `out` and one workspace volume such that the last one lands in `out`
        const int slot = masked ? (i & 1) : 0;
        const bool to_out = a.last || (!masked && ((npass - 1 - i) & 1) == 0);
        if (to_out) a.num_out = outf, a.den_out = nullptr, a.out_sz = vol_sz, a.out_sy = vol_sy, a.out_off = vol_off;
        else a.num_out = ws.num[slot].as<float>(), a.den_out = masked ? ws.den[slot].as<float>() : nullptr, a.out_sz = box_sz, a.out_sy = box_sy, a.out_off = 0;
        Taps t;
        std::memset(&t, 0, sizeof t);
        t.r = p.radius[axis];
        std::memcpy(t.w, p.taps[axis], sizeof(float) * (2 * t.r + 1));
        LM_TRY(masked ? sep_pass<true>(e, axis, a, t) : sep_pass<false>(e, axis, a, t));
        prev_num = a.num_out;
        prev_den = a.den_out;
    }
    return LM_OK;
}

}  // namespace lm
