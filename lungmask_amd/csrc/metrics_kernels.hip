// Label agreement metrics (lm_edt_dev, lm_label_agreement_dev; include/lungmask_hip.h): an exact anisotropic squared Euclidean
// distance transform, and around it the overlap counts, 6-neighbour surfaces and surface-distance reductions of two label volumes.
//
// Distance transform.  Three separable min-plus passes in float32, each the literal definition of the header:
//   x  one wave per row: the row's feature bits as 64-bit ballot words in LDS, every voxel finds the nearest set bit on either side
//      with integer work (volume_common.h: nearest_set_bits) and multiplies once (edt_x_kernel);
//   y, z  a workgroup holds a tile of whole lines in LDS -- threads along x, so global accesses are runs of TX consecutive floats --
//      and every voxel searches outwards from its own position until w * r^2 >= best (edt_line_kernel).  fl(g + c) >= c for g >= 0
//      and float rounding is monotone, so nothing beyond that offset can win: the result is the true minimum of the float32
//      expressions, whatever the order of the search.  A tile is loaded completely before anything is written, so the pass runs in
//      place: the transform needs no buffer besides its output.
// Agreement.  agree_overlap_kernel reads both label volumes once (16-byte chunks, the six neighbours only for chunks with
// foreground), writes the two surface volumes and counts voxels / intersection / surface voxels / union boxes per label in LDS;
// with BIN it binarises the labels first (row 0, "lung").  Per row the two transforms run inside the row's union box; the distances
// at the surface voxels are reduced where they lie (surf_reduce_kernel: count, max, sum of roots in a fixed order), and the order
// statistics come from a 4 x 8-bit radix select over the float bit patterns (select_hist_kernel / select_scan_kernel) -- the
// distance lists never exist, neither on the device nor on the host.  Every result except the sum of roots is integer or a
// selected float: independent of the schedule.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kSlots = 17;     // accumulator slots: labels 0 .. 15 (BIN: slot 0 = lung), 16 = labels >= n_labels
enum { C_A, C_B, C_I, C_SA, C_SB, kCnt };  // counts per slot: voxels of a, of b, intersection, surface voxels of a, of b
constexpr int kMaxQ = 8, kMaxT = 6 * kMaxQ;  // targets of the select: 3 lists (a->b, b->a, pooled) x percentiles x (floor, ceil)

// ------------------------------------------------------------------------------------------------ distance transform
constexpr int kXT = 256;  // x pass: 4 waves, one row each

// g1[z][y][x] = wx * (float)(dx^2), dx = distance to the nearest feature of the row; +inf for a row without one.
// feature: src[(z0+z)][(y0+y)][(x0+x)] == match, or != 0 when match == 0 (src has the strides of the whole volume H x W).
__global__ __launch_bounds__(kXT) void edt_x_kernel(const uint8_t* __restrict__ src, int H, int W, VolBox b, int match, float wx,
                                                   float* __restrict__ g1) {
    __shared__ unsigned long long bits[kXT / 64][kMaxDim / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nrows = b.n * b.h, nwords = (b.w + 63) >> 6;
    for (int base = blockIdx.x * (kXT / 64); base < nrows; base += gridDim.x * (kXT / 64)) {  // (uniform trip count: barriers inside)
        const int row = base + wave;
        const bool live = row < nrows;
        const int z = live ? row / b.h : 0, y = live ? row - z * b.h : 0;
        const uint8_t* s = src + ((size_t)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
        for (int c = 0; c < nwords; ++c) {
            const int x = c * 64 + lane;
            int f = 0;
            if (live && x < b.w) {
                const int v = s[x];
                f = match ? v == match : v != 0;
            }
            const unsigned long long word = __ballot(f);
            if (lane == 0) bits[wave][c] = word;
        }
        __syncthreads();
        if (live) {
            float* out = g1 + (size_t)row * b.w;
            for (int x = lane; x < b.w; x += 64) {
                int xl, xr;  // position of the nearest feature at or before x / after x
                nearest_set_bits(bits[wave], nwords, x, xl, xr);
                const int dl = x - xl, dr = xr - x;  // each a distance only where its side has a feature
                const int d = (xl & xr) < 0 ? INT_MAX : (xr < 0 ? dl : (xl < 0 ? dr : min(dl, dr)));  // (xl & xr) < 0: both are -1
                out[x] = d == INT_MAX ? INFINITY : wx * (float)(d * d);
            }
        }
        __syncthreads();
    }
}

constexpr int kLT = 512;        // line pass: 8 waves
constexpr int kTile = 16384;    // floats of LDS per workgroup (64 KiB: two workgroups = 16 waves per CU)

// In place: f[o][l][x] = min over l' of fl(f[o][l'][x] + fl(wgt * (float)((l - l')^2))), element (o, l, x) at o * so + l * sl + x.
// y pass: o = z, so = h * w, sl = w;  z pass: o = y, so = w, sl = h * w.  A tile = TX consecutive x of one o, all L values of l.
__global__ __launch_bounds__(kLT) void edt_line_kernel(float* f, int n_outer, size_t so, size_t sl, int L, int w, int TX, float wgt) {
    __shared__ float tile[kTile];
    const int nxt = (w + TX - 1) / TX;
    const long long tiles = (long long)n_outer * nxt;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int o = (int)(t / nxt), xb = (int)(t - (long long)o * nxt) * TX;
        const int tx = w - xb < TX ? w - xb : TX;  // columns of this tile
        float* base = f + (size_t)o * so + xb;
        const int cells = L * tx;
        for (int p = threadIdx.x; p < cells; p += kLT) {
            const int l = p / tx, x = p - l * tx;
            tile[p] = base[(size_t)l * sl + x];
        }
        __syncthreads();
        for (int p = threadIdx.x; p < cells; p += kLT) {
            const int l = p / tx, x = p - l * tx;
            float best = tile[p];
            for (int r = 1; r < L; ++r) {
                const float c = wgt * (float)(r * r);
                if (!(c < best)) break;  // every candidate from here on is >= c >= best
                const int lo = l - r, hi = l + r;
                if (lo < 0 && hi >= L) break;
                if (lo >= 0) best = fminf(best, tile[lo * tx + x] + c);
                if (hi < L) best = fminf(best, tile[hi * tx + x] + c);
            }
            base[(size_t)l * sl + x] = best;
        }
        __syncthreads();
    }
}

int edt_box(lm_engine* e, const uint8_t* src, int H, int W, const VolBox& b, int match, const float wgt[3], float* d2) {
    const int nrows = b.n * b.h;
    {
        ProfScope ps(e, "edt_x", (double)nrows * b.w * 5.0);
        LM_LAUNCH(edt_x_kernel, dim3((unsigned)std::min((nrows + 3) / 4, 1 << 16)), dim3(kXT), 0, e->stream, src, H, W, b, match, wgt[2],
                  d2);
        LM_K(hipGetLastError());
    }
    for (int axis = 1; axis >= 0; --axis) {  // y, then z
        const LinePass lp = line_pass_plan(b, axis, kTile);
        if (lp.L == 1) continue;
        ProfScope ps(e, axis == 1 ? "edt_y" : "edt_z", (double)nrows * b.w * 8.0);
        LM_LAUNCH(edt_line_kernel, dim3((unsigned)std::min<long long>(lp.tiles, 1 << 20)), dim3(kLT), 0, e->stream, d2, lp.n_outer, lp.so,
                  lp.sl, lp.L, b.w, lp.TX, wgt[axis]);
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------ overlap and surfaces
constexpr int kOT = 256;

struct OverlapParams {
    const uint8_t *a, *b;
    uint8_t *sa, *sb;
    int n, h, w, n_labels;
    unsigned cpr, nchunks;  // 16-voxel chunks per row, in the volume
    int vec;                // 16-byte accesses (w % 16 == 0, every base 16-byte aligned)
    unsigned long long* cnt;  // [kSlots][kCnt]
    int* box;                 // [kSlots][6]: z0, z1, y0, y1, x0, x1 (inclusive maxima; INT_MAX / -1 when empty)
};

__global__ void agree_init_kernel(unsigned long long* cnt, int* box) {
    const int i = threadIdx.x;
    if (i < kSlots * kCnt) cnt[i] = 0ull;
    if (i < kSlots * 6) box[i] = (i % 6) % 2 == 0 ? INT_MAX : -1;
}

template <bool BIN> __device__ __forceinline__ uint8_t map_label(uint8_t k) { return BIN ? (uint8_t)(k ? 1 : 0) : k; }

// 16 mapped labels at p[0 .. 15]; positions >= nx (beyond the row) and a missing neighbour row (p == nullptr) read as 0
template <bool BIN> __device__ __forceinline__ void load_chunk(const uint8_t* p, int nx, int vec, uint8_t (&l)[16]) {
    if (!p) {
#pragma unroll
        for (int i = 0; i < 16; ++i) l[i] = 0;
    } else if (vec) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned wd = i == 0 ? q.x : (i == 1 ? q.y : (i == 2 ? q.z : q.w));
#pragma unroll
            for (int j = 0; j < 4; ++j) l[4 * i + j] = map_label<BIN>((uint8_t)(wd >> (8 * j)));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) l[i] = i < nx ? map_label<BIN>(p[i]) : (uint8_t)0;
    }
}

__device__ __forceinline__ void store_chunk(uint8_t* p, int nx, int vec, const uint8_t (&l)[16]) {
    if (vec) {
        unsigned wd[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            wd[i] = (unsigned)l[4 * i] | ((unsigned)l[4 * i + 1] << 8) | ((unsigned)l[4 * i + 2] << 16) | ((unsigned)l[4 * i + 3] << 24);
        uint4 q;
        q.x = wd[0], q.y = wd[1], q.z = wd[2], q.w = wd[3];
        *reinterpret_cast<uint4*>(p) = q;
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < nx) p[i] = l[i];
    }
}

template <bool BIN> __device__ __forceinline__ int slot_of(int v, int nl) { return BIN ? 0 : (v < nl ? v : kSlots - 1); }

// The runs of equal non-zero values of one chunk go to the LDS accumulators: count field `fld` of the value's slot, and with
// `boxed` the slot's box (the chunk lies in row y of slice z and starts at x = xb).
template <bool BIN>
__device__ __forceinline__ void count_runs(const uint8_t (&v)[16], int fld, bool boxed, int nl, int z, int y, int xb, unsigned* cnt,
                                           int* box) {
    int cur = 0, len = 0, start = 0;
#pragma unroll
    for (int i = 0; i <= 16; ++i) {
        const int val = i < 16 ? v[i] : 0;
        if (val != cur) {
            if (cur) {
                const int s = slot_of<BIN>(cur, nl);
                atomicAdd(&cnt[s * kCnt + fld], (unsigned)len);
                if (boxed) {
                    atomicMin(&box[s * 6 + 0], z);
                    atomicMax(&box[s * 6 + 1], z);
                    atomicMin(&box[s * 6 + 2], y);
                    atomicMax(&box[s * 6 + 3], y);
                    atomicMin(&box[s * 6 + 4], xb + start);
                    atomicMax(&box[s * 6 + 5], xb + i - 1);
                }
            }
            cur = val;
            len = 0;
            start = i;
        }
        ++len;
    }
}

// surf[i] = c[i] where voxel i has label >= 1 and one of its six face neighbours has another label or lies outside the volume
template <bool BIN>
__device__ __forceinline__ void chunk_surface(const uint8_t* vol, const OverlapParams& p, int z, int y, int xb, int nx, size_t off,
                                              const uint8_t (&c)[16], uint8_t (&surf)[16]) {
    uint8_t zm[16], zp[16], ym[16], yp[16];
    const size_t plane = (size_t)p.h * p.w;
    load_chunk<BIN>(z > 0 ? vol + off - plane : nullptr, nx, p.vec, zm);
    load_chunk<BIN>(z + 1 < p.n ? vol + off + plane : nullptr, nx, p.vec, zp);
    load_chunk<BIN>(y > 0 ? vol + off - p.w : nullptr, nx, p.vec, ym);
    load_chunk<BIN>(y + 1 < p.h ? vol + off + p.w : nullptr, nx, p.vec, yp);
    const uint8_t left = xb > 0 ? map_label<BIN>(vol[off - 1]) : (uint8_t)0;
    const uint8_t right = xb + 16 < p.w ? map_label<BIN>(vol[off + 16]) : (uint8_t)0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint8_t v = c[i];
        const uint8_t l = i > 0 ? c[i - 1] : left, r = i < 15 ? c[i + 1] : right;  // (c is 0 beyond the row's end)
        const bool edge = zm[i] != v || zp[i] != v || ym[i] != v || yp[i] != v || l != v || r != v;
        surf[i] = (v && edge) ? v : (uint8_t)0;
    }
}

template <bool BIN>
__global__ __launch_bounds__(kOT) void agree_overlap_kernel(OverlapParams p) {
    __shared__ unsigned cnt[kSlots * kCnt];
    __shared__ int box[kSlots * 6];
    const int tid = threadIdx.x;
    if (tid < kSlots * kCnt) cnt[tid] = 0u;
    if (tid < kSlots * 6) box[tid] = (tid % 6) % 2 == 0 ? INT_MAX : -1;
    __syncthreads();
    const int nl = p.n_labels;
    for (unsigned ch = blockIdx.x * kOT + tid; ch < p.nchunks; ch += gridDim.x * kOT) {
        const unsigned row = ch / p.cpr;
        const int xb = (int)(ch - row * p.cpr) * 16;
        const int z = (int)(row / (unsigned)p.h), y = (int)(row - (unsigned)z * p.h);
        const size_t off = (size_t)row * p.w + xb;
        const int nx = p.w - xb < 16 ? p.w - xb : 16;
        uint8_t ca[16], cb[16], s[16];
        load_chunk<BIN>(p.a + off, nx, p.vec, ca);
        load_chunk<BIN>(p.b + off, nx, p.vec, cb);
        bool any_a = false, any_b = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            any_a |= ca[i] != 0;
            any_b |= cb[i] != 0;
        }
        if (any_a) {
            chunk_surface<BIN>(p.a, p, z, y, xb, nx, off, ca, s);
            count_runs<BIN>(ca, C_A, true, nl, z, y, xb, cnt, box);
            count_runs<BIN>(s, C_SA, false, nl, z, y, xb, cnt, box);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0;
        }
        store_chunk(p.sa + off, nx, p.vec, s);
        if (any_b) {
            chunk_surface<BIN>(p.b, p, z, y, xb, nx, off, cb, s);
            count_runs<BIN>(cb, C_B, true, nl, z, y, xb, cnt, box);
            count_runs<BIN>(s, C_SB, false, nl, z, y, xb, cnt, box);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0;
        }
        store_chunk(p.sb + off, nx, p.vec, s);
        if (any_a && any_b) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = ca[i] == cb[i] ? ca[i] : (uint8_t)0;
            count_runs<BIN>(s, C_I, false, nl, z, y, xb, cnt, box);
        }
    }
    __syncthreads();
    if (tid < kSlots * kCnt && cnt[tid]) atomicAdd(&p.cnt[tid], (unsigned long long)cnt[tid]);
    if (tid < kSlots * 6) {
        if ((tid % 6) % 2 == 0) {
            if (box[tid] != INT_MAX) atomicMin(&p.box[tid], box[tid]);
        } else if (box[tid] >= 0) {
            atomicMax(&p.box[tid], box[tid]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ surface distances
// What one row's device passes deliver, list 0 = a -> b (d2 of b's surface read at a's surface voxels), list 1 = b -> a.
struct RowRes {
    unsigned long long count[2];
    double sum[2];          // sum of sqrt((double)d2)
    unsigned max_bits[2];   // d2 >= 0: the float bit patterns order like unsigned integers
    unsigned order[kMaxT];  // bit patterns of the selected order statistics, target t = (list * nq + q) * 2 + (0 floor, 1 ceil)
};

struct SurfParams {
    const uint8_t *sa, *sb;  // surface volumes (strides of the whole volume H x W)
    const float *dab, *dba;  // d2 to b's surface / to a's surface, box-shaped
    int H, W, match;
    VolBox b;
};

constexpr int kRT = 256;

__device__ __forceinline__ unsigned float_bits(float f) {
    unsigned u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

__device__ __forceinline__ bool surf_voxel(const SurfParams& p, size_t i, bool& in_a, bool& in_b) {
    const size_t plane = (size_t)p.b.h * p.b.w;
    const int z = (int)(i / plane);
    const int rem = (int)(i - (size_t)z * plane);
    const int y = rem / p.b.w, x = rem - y * p.b.w;
    const size_t g = ((size_t)(p.b.z0 + z) * p.H + (p.b.y0 + y)) * p.W + (p.b.x0 + x);
    in_a = p.sa[g] == p.match;
    in_b = p.sb[g] == p.match;
    return in_a || in_b;
}

// count, max and the workgroup's sum of roots of both lists (part[blockIdx.x][2]; surf_sum_kernel adds the parts in block order)
__global__ __launch_bounds__(kRT) void surf_reduce_kernel(SurfParams p, RowRes* res, double* part) {
    __shared__ double red[2][kRT / 64];
    const size_t total = (size_t)p.b.n * p.b.h * p.b.w;
    unsigned cnt[2] = {0u, 0u}, mx[2] = {0u, 0u};
    double sum[2] = {0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * kRT + threadIdx.x; i < total; i += (size_t)gridDim.x * kRT) {
        bool in_a, in_b;
        if (!surf_voxel(p, i, in_a, in_b)) continue;
        if (in_a) {
            const float d = p.dab[i];
            cnt[0]++;
            mx[0] = max(mx[0], float_bits(d));
            sum[0] += sqrt((double)d);
        }
        if (in_b) {
            const float d = p.dba[i];
            cnt[1]++;
            mx[1] = max(mx[1], float_bits(d));
            sum[1] += sqrt((double)d);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        for (int m = 32; m >= 1; m >>= 1) {
            cnt[k] += __shfl_xor(cnt[k], m);
            mx[k] = max(mx[k], __shfl_xor(mx[k], m));
            sum[k] += __shfl_xor(sum[k], m);
        }
        if (lane == 0) {
            red[k][wave] = sum[k];
            if (cnt[k]) {
                atomicAdd(&res->count[k], (unsigned long long)cnt[k]);
                atomicMax(&res->max_bits[k], mx[k]);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = red[threadIdx.x][0];
        for (int wv = 1; wv < kRT / 64; ++wv) s += red[threadIdx.x][wv];
        part[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

__global__ void surf_sum_kernel(const double* part, int nparts, RowRes* res) {
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int i = 0; i < nparts; ++i) s += part[(size_t)i * 2 + threadIdx.x];
        res->sum[threadIdx.x] = s;
    }
}

// Radix select, 8 bits per pass from the top.  State per target: the bits fixed so far and the rank among the values that share them.
struct SelState {
    unsigned prefix[kMaxT];
    unsigned long long rank[kMaxT];
};
struct SelRanks {
    unsigned long long rank[kMaxT];
};

// hist[t][digit] += 1 for every value of target t's list whose bits above `shift + 8` equal the target's prefix
__global__ __launch_bounds__(kRT) void select_hist_kernel(SurfParams p, const SelState* st, int nq2, int shift, unsigned* hist) {
    __shared__ unsigned h[kMaxT * 256];
    __shared__ unsigned prefix[kMaxT];
    const int T = 3 * nq2;  // nq2 = 2 * percentiles: targets per list
    for (int i = threadIdx.x; i < T * 256; i += kRT) h[i] = 0u;
    if ((int)threadIdx.x < T) prefix[threadIdx.x] = shift == 24 ? 0u : st->prefix[threadIdx.x] >> (shift + 8);
    __syncthreads();
    const size_t total = (size_t)p.b.n * p.b.h * p.b.w;
    for (size_t i = (size_t)blockIdx.x * kRT + threadIdx.x; i < total; i += (size_t)gridDim.x * kRT) {
        bool in[2];
        if (!surf_voxel(p, i, in[0], in[1])) continue;
        for (int k = 0; k < 2; ++k) {
            if (!in[k]) continue;
            const unsigned u = float_bits(k == 0 ? p.dab[i] : p.dba[i]);
            const unsigned hi = shift == 24 ? 0u : u >> (shift + 8), digit = (u >> shift) & 255u;
            for (int j = 0; j < nq2; ++j) {
                if (prefix[k * nq2 + j] == hi) atomicAdd(&h[(k * nq2 + j) * 256 + digit], 1u);
                if (prefix[2 * nq2 + j] == hi) atomicAdd(&h[(2 * nq2 + j) * 256 + digit], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T * 256; i += kRT)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// one thread per target: the digit that holds the target's rank; the histogram row is left zeroed for the next pass
__global__ void select_scan_kernel(SelState* st, SelRanks first, int T, int shift, unsigned* hist, RowRes* res) {
    const int t = threadIdx.x;
    if (t >= T) return;
    unsigned long long rank = shift == 24 ? first.rank[t] : st->rank[t];
    const unsigned prefix = shift == 24 ? 0u : st->prefix[t];
    unsigned* h = hist + t * 256;
    int digit = 255;
    bool found = false;
    for (int d = 0; d < 256; ++d) {
        const unsigned c = h[d];
        h[d] = 0u;
        if (!found) {
            if (rank < c) {
                digit = d;
                found = true;
            } else {
                rank -= c;
            }
        }
    }
    const unsigned np = prefix | ((unsigned)digit << shift);
    st->prefix[t] = np;
    st->rank[t] = rank;
    if (shift == 0) res->order[t] = np;
}

int overlap_pass(lm_engine* e, bool bin, const uint8_t* a, const uint8_t* b, int n, int h, int w, int n_labels, unsigned long long* cnt,
                 int* box) {
    MetricsWorkspace& ws = e->metrics;
    OverlapParams p;
    p.a = a, p.b = b, p.sa = ws.sa.as<uint8_t>(), p.sb = ws.sb.as<uint8_t>();
    p.n = n, p.h = h, p.w = w, p.n_labels = n_labels;
    p.cpr = (unsigned)(w + 15) / 16;
    p.nchunks = (unsigned)((size_t)n * h * p.cpr);
    p.vec = (w % 16 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(p.sa) |
                              reinterpret_cast<uintptr_t>(p.sb)) & 15) == 0) ? 1 : 0;
    p.cnt = ws.acc.as<unsigned long long>();
    p.box = reinterpret_cast<int*>(p.cnt + kSlots * kCnt);
    int cus = 0;
    LM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    const unsigned grid = std::max(1u, std::min((p.nchunks + kOT - 1) / kOT, (unsigned)std::max(cus, 1) * 8u));
    {
        ProfScope ps(e, bin ? "agree_overlap_bin" : "agree_overlap", (double)n * h * w * 4.0);
        LM_LAUNCH(agree_init_kernel, dim3(1), dim3(128), 0, e->stream, p.cnt, p.box);
        LM_K(hipGetLastError());
        if (bin)
            LM_LAUNCH(agree_overlap_kernel<true>, dim3(grid), dim3(kOT), 0, e->stream, p);
        else
            LM_LAUNCH(agree_overlap_kernel<false>, dim3(grid), dim3(kOT), 0, e->stream, p);
        LM_K(hipGetLastError());
    }
    const size_t bytes = kSlots * kCnt * 8 + kSlots * 6 * 4;
    LM_HIP(hipMemcpyAsync(ws.h_acc.p, p.cnt, bytes, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(cnt, ws.h_acc.p, kSlots * kCnt * 8);
    std::memcpy(box, ws.h_acc.as<char>() + kSlots * kCnt * 8, kSlots * 6 * 4);
    return LM_OK;
}

// rank of the lower / upper neighbour of numpy's method="linear" position q / 100 * (count - 1)
void linear_ranks(unsigned long long count, double q, unsigned long long* lo, unsigned long long* hi) {
    const double pos = (q / 100.0) * (double)(count - 1);
    *lo = std::min<unsigned long long>((unsigned long long)std::floor(pos), count - 1);
    *hi = std::min<unsigned long long>((unsigned long long)std::ceil(pos), count - 1);
}

// the device passes of one row, enqueued only: both transforms inside `b`, the reductions and the select -> res_dev
int row_distances(lm_engine* e, int match, const VolBox& b, int H, int W, const float wgt[3], unsigned long long sa_count,
                  unsigned long long sb_count, const double* percentiles, int nq, RowRes* res_dev) {
    MetricsWorkspace& ws = e->metrics;
    float *dab = ws.d2[0].as<float>(), *dba = ws.d2[1].as<float>();
    LM_TRY(edt_box(e, ws.sb.as<uint8_t>(), H, W, b, match, wgt, dab));
    LM_TRY(edt_box(e, ws.sa.as<uint8_t>(), H, W, b, match, wgt, dba));
    SurfParams p;
    p.sa = ws.sa.as<uint8_t>(), p.sb = ws.sb.as<uint8_t>(), p.dab = dab, p.dba = dba;
    p.H = H, p.W = W, p.match = match, p.b = b;
    const size_t total = (size_t)b.n * b.h * b.w;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((total + kRT - 1) / kRT, 1024));
    double* part = ws.part.as<double>();
    {
        ProfScope ps(e, "surf_reduce", (double)total * 2.0);
        LM_LAUNCH(surf_reduce_kernel, dim3(grid), dim3(kRT), 0, e->stream, p, res_dev, part);
        LM_K(hipGetLastError());
        LM_LAUNCH(surf_sum_kernel, dim3(1), dim3(64), 0, e->stream, (const double*)part, grid, res_dev);
        LM_K(hipGetLastError());
    }
    if (nq == 0) return LM_OK;
    SelRanks first;
    std::memset(&first, 0, sizeof first);
    const unsigned long long counts[3] = {sa_count, sb_count, sa_count + sb_count};
    for (int l = 0; l < 3; ++l)
        for (int q = 0; q < nq; ++q) linear_ranks(counts[l], percentiles[q], &first.rank[(l * nq + q) * 2], &first.rank[(l * nq + q) * 2 + 1]);
    SelState* st = reinterpret_cast<SelState*>(ws.sel.as<char>());
    unsigned* hist = reinterpret_cast<unsigned*>(ws.sel.as<char>() + sizeof(SelState));
    ProfScope ps(e, "surf_select", (double)total * 2.0 * 4);
    for (int shift = 24; shift >= 0; shift -= 8) {
        LM_LAUNCH(select_hist_kernel, dim3(grid), dim3(kRT), 0, e->stream, p, (const SelState*)st, 2 * nq, shift, hist);
        LM_K(hipGetLastError());
        LM_LAUNCH(select_scan_kernel, dim3(1), dim3(64), 0, e->stream, st, first, 6 * nq, shift, hist, res_dev);
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

float bits_float(unsigned u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

}  // namespace

int edt(lm_engine* e, const uint8_t* feat, int n, int h, int w, const double* spacing, float* d2) {
    if (n == 0) return LM_OK;
    float wgt[3];
    edt_weights(spacing, wgt);
    const VolBox b{0, 0, 0, n, h, w};
    return edt_box(e, feat, h, w, b, 0, wgt, d2);
}

int label_agreement(lm_engine* e, const uint8_t* a, const uint8_t* b, int n, int h, int w, int n_labels, const double* spacing,
                    const double* percentiles, int nq, lm_label_agreement* rows) {
    for (int k = 0; k < n_labels; ++k) {
        lm_label_agreement& r = rows[k];
        std::memset(&r, 0, sizeof r);
        for (int q = 0; q < 6; ++q) r.bbox[q] = -1;
        r.max_d2_ab = r.max_d2_ba = -1.f;
        for (int q = 0; q < kMaxQ; ++q)
            for (int j = 0; j < 2; ++j) r.order_ab[q][j] = r.order_ba[q][j] = r.order_pooled[q][j] = -1.f;
    }
    if (n == 0) return LM_OK;
    MetricsWorkspace& ws = e->metrics;
    const size_t nvox = (size_t)n * h * w;
    LM_TRY(ws.sa.reserve(nvox));
    LM_TRY(ws.sb.reserve(nvox));
    LM_TRY(ws.acc.reserve(kSlots * kCnt * 8 + kSlots * 6 * 4));
    LM_TRY(ws.h_acc.reserve(std::max<size_t>(kSlots * kCnt * 8 + kSlots * 6 * 4, sizeof(RowRes) * 16)));
    LM_TRY(ws.res.reserve(sizeof(RowRes) * 16));
    LM_TRY(ws.part.reserve(1024 * 2 * 8));
    LM_TRY(ws.sel.reserve(sizeof(SelState) + kMaxT * 256 * 4));
    float wgt[3];
    edt_weights(spacing, wgt);
    RowRes* res = ws.res.as<RowRes>();
    LM_HIP(hipMemsetAsync(res, 0, sizeof(RowRes) * 16, e->stream));
    LM_HIP(hipMemsetAsync(ws.sel.as<char>() + sizeof(SelState), 0, kMaxT * 256 * 4, e->stream));
    unsigned long long cnt[kSlots * kCnt];
    int box[kSlots * 6];
    bool ran[16] = {false};
    auto fill = [&](int k, int slot) -> VolBox {
        lm_label_agreement& r = rows[k];
        r.voxels_a = (int64_t)cnt[slot * kCnt + C_A];
        r.voxels_b = (int64_t)cnt[slot * kCnt + C_B];
        r.intersection = (int64_t)cnt[slot * kCnt + C_I];
        r.surface_a = (int64_t)cnt[slot * kCnt + C_SA];
        r.surface_b = (int64_t)cnt[slot * kCnt + C_SB];
        VolBox bx{0, 0, 0, 0, 0, 0};
        if (r.voxels_a + r.voxels_b > 0) {
            const int* q = box + slot * 6;
            const int bb[6] = {q[0], q[1] + 1, q[2], q[3] + 1, q[4], q[5] + 1};
            for (int i = 0; i < 6; ++i) r.bbox[i] = bb[i];
            bx = VolBox{bb[0], bb[2], bb[4], bb[1] - bb[0], bb[3] - bb[2], bb[5] - bb[4]};
        }
        return bx;
    };
    // row 0 first: its box holds every label's box, so it sizes the two distance volumes once
    LM_TRY(overlap_pass(e, true, a, b, n, h, w, n_labels, cnt, box));
    {
        const VolBox bx = fill(0, 0);
        const size_t bvox = (size_t)bx.n * bx.h * bx.w;
        LM_TRY(ws.d2[0].reserve(std::max<size_t>(bvox, 1) * 4));
        LM_TRY(ws.d2[1].reserve(std::max<size_t>(bvox, 1) * 4));
        if (rows[0].surface_a > 0 && rows[0].surface_b > 0) {
            LM_TRY(row_distances(e, 1, bx, h, w, wgt, (unsigned long long)rows[0].surface_a, (unsigned long long)rows[0].surface_b,
                                 percentiles, nq, res));
            ran[0] = true;
        }
    }
    LM_TRY(overlap_pass(e, false, a, b, n, h, w, n_labels, cnt, box));  // (stream order: behind row 0's reads of the surfaces)
    rows[0].other_a = (int64_t)cnt[(kSlots - 1) * kCnt + C_A];
    rows[0].other_b = (int64_t)cnt[(kSlots - 1) * kCnt + C_B];
    for (int k = 1; k < n_labels; ++k) {
        const VolBox bx = fill(k, k);
        if (rows[k].surface_a > 0 && rows[k].surface_b > 0) {
            LM_TRY(row_distances(e, k, bx, h, w, wgt, (unsigned long long)rows[k].surface_a, (unsigned long long)rows[k].surface_b,
                                 percentiles, nq, res + k));
            ran[k] = true;
        }
    }
    LM_HIP(hipMemcpyAsync(ws.h_acc.p, res, sizeof(RowRes) * 16, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const RowRes* hr = ws.h_acc.as<RowRes>();
    for (int k = 0; k < n_labels; ++k) {
        if (!ran[k]) continue;
        lm_label_agreement& r = rows[k];
        if ((int64_t)hr[k].count[0] != r.surface_a || (int64_t)hr[k].count[1] != r.surface_b) {
            set_error("lm_label_agreement_dev: surface counts of row %d disagree between the passes", k);
            return LM_ERR_DEVICE;
        }
        r.max_d2_ab = bits_float(hr[k].max_bits[0]);
        r.max_d2_ba = bits_float(hr[k].max_bits[1]);
        r.sum_d_ab = hr[k].sum[0];
        r.sum_d_ba = hr[k].sum[1];
        for (int q = 0; q < nq; ++q)
            for (int j = 0; j < 2; ++j) {
                r.order_ab[q][j] = bits_float(hr[k].order[(0 * nq + q) * 2 + j]);
                r.order_ba[q][j] = bits_float(hr[k].order[(1 * nq + q) * 2 + j]);
                r.order_pooled[q][j] = bits_float(hr[k].order[(2 * nq + q) * 2 + j]);
            }
    }
    return LM_OK;
}

}  // namespace lm
