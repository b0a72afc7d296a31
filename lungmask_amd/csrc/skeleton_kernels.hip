// Skeleton, point list and calibre classes (lm_skeleton_dev, lm_skeleton_points_dev, lm_calibre_dev, lm_vessel_mask_dev; include/lungmask_hip.h has the
// definitions).
//   skel_init_kernel     sel, keep -> `work`, one u8 per voxel of the selection's box with a border of ONE voxel that stays 0: every
//                        neighbour of a box voxel has a cell, so the thinning reads without bounds checks, and the border stands for
//                        "background", inside the volume and outside of it alike.  Counts |S|.
//   skel_substep_kernel  one sub-step (direction d, subfield f): one thread per voxel of the subfield (parity of the index IN THE
//                        VOLUME).  A thread leaves unless its voxel is set and its d-neighbour is clear; a candidate gathers its 26
//                        neighbours into one word and tests "end point" and "simple point" in registers: two bit-parallel flood fills
//                        (26-connected object voxels of N26; 6-connected background voxels of N18 from the N6 seeds) with constant
//                        shift masks.  A deleted voxel is cleared in place: no thread of the sub-step reads or writes another
//                        thread's voxel, because two voxels of a subfield are never 26-adjacent.  No LDS but one counter.
//   skel_code_kernel     work -> out over the whole volume: 0, or 1 + the number of set neighbours.
//   points_*_kernel      count per 4096-voxel chunk, one-workgroup scan of the chunk counts, ordered write: ascending raster order
//                        without any atomics on the order.
//   vessel_mask_kernel   V, labels, threshold -> the u8 vessel mask the three entry points above start from.
//   calibre_*_kernel     the complement of the mask (lm_edt_dev's features), the class of the skeleton voxels from d2, and the class
//                        volume with its label x class counts from lm_nearest_label_dev's result.
// LDS: the keep table, one scan buffer or the 16 x 9 counters, under 2 KiB in every kernel; the thinning kernel holds one counter.
// No kernel waits on another workgroup; the pass loop is the host's: 48 launches and one counter read back per pass.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kST = 256;  // every kernel: 4 waves

// ------------------------------------------------------------------------------------------------ 3 x 3 x 3 neighbourhood words
// bit i = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of a word is the voxel at offset (dz, dy, dx); bit 13 is the centre.
constexpr unsigned kAll = 0x7FFFFFFu, kCentre = 1u << 13;
constexpr unsigned kX0 = 0x1249249u, kX2 = kX0 << 2;  // dx = -1, dx = +1
constexpr unsigned kY0 = 0x01C0E07u, kY2 = kY0 << 6;  // dy = -1, dy = +1
constexpr unsigned kCorners = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
constexpr unsigned kN18 = kAll & ~kCorners & ~kCentre;
constexpr unsigned kN6 = (1u << 4) | (1u << 22) | (1u << 10) | (1u << 16) | (1u << 12) | (1u << 14);

// the voxels one step along an axis from a voxel of m (m within kAll; a step out of the cube is dropped)
__device__ __forceinline__ unsigned shift_x(unsigned m) { return ((m << 1) & (kAll & ~kX0)) | ((m >> 1) & ~kX2); }
__device__ __forceinline__ unsigned shift_y(unsigned m) { return ((m << 3) & (kAll & ~kY0)) | ((m >> 3) & ~kY2); }
__device__ __forceinline__ unsigned shift_z(unsigned m) { return ((m << 9) & kAll) | (m >> 9); }

// the voxels of the cube within one 26-step (the box: separable) / one 6-step of a voxel of m, m included
__device__ __forceinline__ unsigned grow26(unsigned m) {
    m |= shift_x(m);
    m |= shift_y(m);
    m |= shift_z(m);
    return m;
}
__device__ __forceinline__ unsigned grow6(unsigned m) { return m | shift_x(m) | shift_y(m) | shift_z(m); }

// obj: the object voxels of N26(v) (bit 13 clear).  Every round of a fill adds a voxel or ends it: at most 26 rounds.
__device__ __forceinline__ bool simple_point(unsigned obj) {
    if (obj == 0u) return false;
    unsigned f = obj & (0u - obj);
    for (;;) {
        const unsigned g = grow26(f) & obj;
        if (g == f) break;
        f = g;
    }
    if (f != obj) return false;
    const unsigned bg = ~obj & kN18, seeds = bg & kN6;
    if (seeds == 0u) return false;
    f = seeds & (0u - seeds);
    for (;;) {
        const unsigned g = grow6(f) & bg;
        if (g == f) break;
        f = g;
    }
    return (seeds & ~f) == 0u;
}

// the padded box: cell (lz, ly, lx) is the volume's voxel (z0 - 1 + lz, y0 - 1 + ly, x0 - 1 + lx); b = the selection's box
struct SkelBox {
    VolBox b;
    int ph, pw;  // padded height and width (b.h + 2, b.w + 2)
};

__device__ __forceinline__ unsigned gather26(const uint8_t* __restrict__ c, size_t plane, int pw) {
    unsigned word = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const uint8_t* r = c + (long long)dz * (long long)plane + dy * pw;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int i = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1);
                if (i != 13 && r[dx] != 0) word |= 1u << i;
            }
        }
    return word;
}

// ------------------------------------------------------------------------------------------------ thinning
__global__ __launch_bounds__(kST) void skel_init_kernel(const uint8_t* __restrict__ sel, int H, int W, SkelBox s, LabelTable kb,
                                                        uint8_t* __restrict__ work, unsigned long long* cnt) {
    __shared__ uint8_t keep[256];
    __shared__ unsigned found;
    stage_table(kb, keep, threadIdx.x);
    if (threadIdx.x == 0) found = 0u;
    __syncthreads();
    unsigned mine = 0;
    const int rows = (s.b.n + 2) * s.ph;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int lz = row / s.ph, ly = row - lz * s.ph;
        const bool inner = lz >= 1 && lz <= s.b.n && ly >= 1 && ly <= s.b.h;
        const uint8_t* src = inner ? sel + ((size_t)(s.b.z0 + lz - 1) * H + (s.b.y0 + ly - 1)) * W + s.b.x0 : sel;  // the row's box voxels
        uint8_t* dst = work + (size_t)row * s.pw;
        for (int lx = threadIdx.x; lx < s.pw; lx += kST) {
            const bool on = inner && lx >= 1 && lx <= s.b.w && keep[src[lx - 1]] != 0;
            dst[lx] = on ? (uint8_t)1 : (uint8_t)0;
            mine += on ? 1u : 0u;
        }
    }
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    if (threadIdx.x == 0 && found) atomicAdd(&cnt[0], (unsigned long long)found);
}

// i0 = first box index of the subfield along each axis, m = number of subfield voxels along it; off_d: from a cell to its d-neighbour
struct SubStep {
    int iz0, iy0, ix0, mz, my, mx;
    long long off_d;
};

__global__ __launch_bounds__(kST) void skel_substep_kernel(uint8_t* work, SkelBox s, SubStep q, unsigned long long* cnt) {
    __shared__ unsigned deleted;
    if (threadIdx.x == 0) deleted = 0u;
    __syncthreads();
    const size_t plane = (size_t)s.ph * s.pw;
    const long long total = (long long)q.mz * q.my * q.mx;
    unsigned mine = 0;
    for (long long t = (long long)blockIdx.x * kST + threadIdx.x; t < total; t += (long long)gridDim.x * kST) {
        const int kx = (int)(t % q.mx);
        const long long r = t / q.mx;
        const int ky = (int)(r % q.my), kz = (int)(r / q.my);
        uint8_t* c = work + (size_t)(q.iz0 + 2 * kz + 1) * plane + (size_t)(q.iy0 + 2 * ky + 1) * s.pw + (q.ix0 + 2 * kx + 1);
        if (c[0] == 0 || c[q.off_d] != 0) continue;
        const unsigned obj = gather26(c, plane, s.pw);
        if (__popc(obj) <= 1) continue;  // end point or isolated voxel
        if (simple_point(obj)) {
            c[0] = 0;
            ++mine;
        }
    }
    if (mine) atomicAdd(&deleted, mine);
    __syncthreads();
    if (threadIdx.x == 0 && deleted) atomicAdd(&cnt[1], (unsigned long long)deleted);
}

__global__ __launch_bounds__(kST) void skel_code_kernel(const uint8_t* __restrict__ work, SkelBox s, int N, int H, int W,
                                                        uint8_t* __restrict__ out) {
    const size_t plane = (size_t)s.ph * s.pw;
    const int rows = N * H;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int z = row / H, y = row - z * H;
        const int lz = z - s.b.z0 + 1, ly = y - s.b.y0 + 1;
        const bool inner = lz >= 1 && lz <= s.b.n && ly >= 1 && ly <= s.b.h;
        uint8_t* dst = out + (size_t)row * W;
        for (int x = threadIdx.x; x < W; x += kST) {
            const int lx = x - s.b.x0 + 1;
            uint8_t code = 0;
            if (inner && lx >= 1 && lx <= s.b.w) {
                const uint8_t* c = work + (size_t)lz * plane + (size_t)ly * s.pw + lx;
                if (c[0] != 0) code = (uint8_t)(1 + __popc(gather26(c, plane, s.pw)));
            }
            dst[x] = code;
        }
    }
}

// ------------------------------------------------------------------------------------------------ point list
constexpr int kPV = 16;              // voxels of one thread, consecutive
constexpr int kPC = kST * kPV;       // voxels of one workgroup

// exclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); *sum = the workgroup's total
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* buf, unsigned* sum) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kST; d <<= 1) {
        const unsigned add = t >= d ? buf[t - d] : 0u;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const unsigned incl = buf[t];
    *sum = buf[kST - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kST) void points_count_kernel(const uint8_t* __restrict__ skel, size_t nvox, unsigned* __restrict__ wgcnt) {
    __shared__ unsigned found;
    if (threadIdx.x == 0) found = 0u;
    __syncthreads();
    const size_t v0 = (size_t)blockIdx.x * kPC + (size_t)threadIdx.x * kPV;
    unsigned mine = 0;
    for (int j = 0; j < kPV; ++j)
        if (v0 + j < nvox && skel[v0 + j] != 0) ++mine;
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    if (threadIdx.x == 0) wgcnt[blockIdx.x] = found;
}

// ONE workgroup: wgcnt[i] (counts) -> the number of points in front of chunk i, in place; cnt[2] = the total
__global__ __launch_bounds__(kST) void points_scan_kernel(unsigned* wgcnt, int chunks, unsigned long long* cnt) {
    __shared__ unsigned buf[kST];
    unsigned carry = 0;  // (the same in every thread)
    for (int i0 = 0; i0 < chunks; i0 += kST) {
        const int i = i0 + (int)threadIdx.x;
        const unsigned v = i < chunks ? wgcnt[i] : 0u;
        unsigned sum;
        const unsigned ex = block_exclusive_scan(v, buf, &sum);
        if (i < chunks) wgcnt[i] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) cnt[2] = carry;  // (fewer than 2^31 voxels)
}

__global__ __launch_bounds__(kST) void points_write_kernel(const uint8_t* __restrict__ skel, const float* __restrict__ d2, size_t nvox,
                                                           const unsigned* __restrict__ wgoff, long long cap, int32_t* __restrict__ index,
                                                           uint8_t* __restrict__ code, float* __restrict__ d2_out) {
    __shared__ unsigned buf[kST];
    const size_t v0 = (size_t)blockIdx.x * kPC + (size_t)threadIdx.x * kPV;
    unsigned mine = 0;
    for (int j = 0; j < kPV; ++j)
        if (v0 + j < nvox && skel[v0 + j] != 0) ++mine;
    unsigned sum;
    long long pos = (long long)wgoff[blockIdx.x] + block_exclusive_scan(mine, buf, &sum);
    if (mine == 0) return;
    for (int j = 0; j < kPV; ++j) {
        const size_t v = v0 + j;
        if (v >= nvox) break;
        const uint8_t c = skel[v];
        if (c == 0) continue;
        if (pos < cap) {
            index[pos] = (int32_t)v;
            code[pos] = c;
            if (d2) d2_out[pos] = d2[v];
        }
        ++pos;
    }
}

// ------------------------------------------------------------------------------------------------ calibre classes
struct Edges2 {
    float e2[LM_CALIBRE_MAX_EDGES];
    int n;
};
constexpr int kCalLabels = 16, kCalCols = LM_CALIBRE_COLUMNS;

// mode 0: out = 1 outside the mask M (lm_edt_dev's features).  mode 1: out = the class of a skeleton voxel of M from d2, else 0.
__global__ __launch_bounds__(kST) void calibre_class_kernel(const uint8_t* __restrict__ sel, const uint8_t* __restrict__ skel,
                                                            const float* __restrict__ d2, size_t nvox, LabelTable kb, Edges2 ed, int mode,
                                                            uint8_t* __restrict__ out) {
    __shared__ uint8_t keep[256];
    stage_table(kb, keep, threadIdx.x);
    __syncthreads();
    for (size_t v = (size_t)blockIdx.x * kST + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kST) {
        const bool in_m = keep[sel[v]] != 0;
        uint8_t r;
        if (mode == 0) {
            r = in_m ? (uint8_t)0 : (uint8_t)1;
        } else {
            r = 0;
            if (in_m && skel[v] != 0) {
                const float d = d2[v];
                int c = 1;
#pragma unroll
                for (int j = 0; j < LM_CALIBRE_MAX_EDGES; ++j) c += (j < ed.n && d >= ed.e2[j]) ? 1 : 0;
                r = (uint8_t)c;
            }
        }
        out[v] = r;
    }
}

__global__ __launch_bounds__(kST) void calibre_out_kernel(const uint8_t* __restrict__ sel, const uint8_t* __restrict__ near,
                                                          const uint8_t* __restrict__ lab, size_t nvox, LabelTable kb, int n_labels,
                                                          uint8_t* __restrict__ out, unsigned long long* cnt) {
    __shared__ uint8_t keep[256];
    __shared__ unsigned hist[kCalLabels * kCalCols];
    stage_table(kb, keep, threadIdx.x);
    for (int i = threadIdx.x; i < kCalLabels * kCalCols; i += kST) hist[i] = 0u;
    __syncthreads();
    // (a workgroup adds fewer than 2^32 voxels: n * h * w < 2^31)
    for (size_t v = (size_t)blockIdx.x * kST + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kST) {
        const bool in_m = keep[sel[v]] != 0;
        const uint8_t c = in_m ? near[v] : (uint8_t)0;
        out[v] = c;
        if (!in_m) continue;
        const int l = lab ? lab[v] : 1;
        if (l >= 1 && l < n_labels && c < kCalCols) atomicAdd(&hist[l * kCalCols + c], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCalLabels * kCalCols; i += kST)
        if (hist[i]) atomicAdd(&cnt[i], (unsigned long long)hist[i]);
}

// out = 1 where V >= threshold inside the labels (a NaN never is), else 0
__global__ __launch_bounds__(kST) void vessel_mask_kernel(const float* __restrict__ V, const uint8_t* __restrict__ lab, size_t nvox, float threshold,
                                                          uint8_t* __restrict__ out) {
    for (size_t v = (size_t)blockIdx.x * kST + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kST)
        out[v] = (lab[v] != 0 && V[v] >= threshold) ? (uint8_t)1 : (uint8_t)0;
}

// ------------------------------------------------------------------------------------------------ host
unsigned flat_grid(size_t nvox) { return (unsigned)std::max<size_t>(1, std::min<size_t>((nvox + kST - 1) / kST, 4096)); }

// the sub-step (d, f) over the box b: the subfield's first index and count per axis from the parity of the box's origin
SubStep sub_step(const SkelBox& s, int d, int f) {
    SubStep q;
    const int par[3] = {(f >> 2) & 1, (f >> 1) & 1, f & 1}, org[3] = {s.b.z0, s.b.y0, s.b.x0}, ext[3] = {s.b.n, s.b.h, s.b.w};
    int i0[3], m[3];
    for (int a = 0; a < 3; ++a) {
        i0[a] = (par[a] ^ org[a]) & 1;
        m[a] = ext[a] > i0[a] ? (ext[a] - i0[a] + 1) / 2 : 0;
    }
    q.iz0 = i0[0], q.iy0 = i0[1], q.ix0 = i0[2];
    q.mz = m[0], q.my = m[1], q.mx = m[2];
    const long long plane = (long long)s.ph * s.pw, step[3] = {plane, (long long)s.pw, 1};
    q.off_d = (d & 1) ? step[d >> 1] : -step[d >> 1];  // -z, +z, -y, +y, -x, +x
    return q;
}

}  // namespace

int skeleton(lm_engine* e, const uint8_t* sel, int n, int h, int w, const uint8_t keep[256], uint8_t* out, int64_t info[4]) {
    info[0] = info[1] = info[2] = info[3] = 0;
    int32_t bb[6];
    LM_TRY(roi_plan(e, sel, n, h, w, keep, bb, "lm_skeleton_dev"));  // (n == 0: no kept voxel either)
    SkelBox s;
    s.b = VolBox{bb[0], bb[2], bb[4], bb[1] - bb[0], bb[3] - bb[2], bb[5] - bb[4]};
    s.ph = s.b.h + 2, s.pw = s.b.w + 2;
    const size_t pvox = (size_t)(s.b.n + 2) * s.ph * s.pw;
    SkeletonWorkspace& ws = e->skel;
    LM_TRY(ws.work.reserve(pvox));
    LM_TRY(ws.cnt.reserve(32));
    LM_TRY(ws.h_cnt.reserve(32));
    uint8_t* work = ws.work.as<uint8_t>();
    unsigned long long* cnt = ws.cnt.as<unsigned long long>();
    const unsigned long long* hc = ws.h_cnt.as<unsigned long long>();
    LM_HIP(hipMemsetAsync(cnt, 0, 32, e->stream));
    {
        ProfScope ps(e, "skeleton_init", (double)pvox * 2.0);
        LM_LAUNCH(skel_init_kernel, dim3((unsigned)std::min((s.b.n + 2) * s.ph, 1 << 16)), dim3(kST), 0, e->stream, sel, h, w, s, label_table(keep),
                  work, cnt);
        LM_K(hipGetLastError());
    }
    long long selected = 0, deleted = 0, passes = 0;
    for (;;) {
        LM_HIP(hipMemsetAsync(cnt + 1, 0, 8, e->stream));
        {
            ProfScope ps(e, "skeleton_pass", (double)pvox * 6.0);
            for (int d = 0; d < 6; ++d)
                for (int f = 0; f < 8; ++f) {
                    const SubStep q = sub_step(s, d, f);
                    const long long total = (long long)q.mz * q.my * q.mx;
                    if (total == 0) continue;
                    const unsigned grid = (unsigned)std::min<long long>((total + kST - 1) / kST, 1 << 20);
                    LM_LAUNCH(skel_substep_kernel, dim3(grid), dim3(kST), 0, e->stream, work, s, q, cnt);
                    LM_K(hipGetLastError());
                }
        }
        LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, 16, hipMemcpyDeviceToHost, e->stream));
        LM_HIP(hipStreamSynchronize(e->stream));
        selected = (long long)hc[0];
        ++passes;
        if (hc[1] == 0) break;
        deleted += (long long)hc[1];
        if (passes > selected + 1) {  // every pass but the last deletes a voxel
            set_error("lm_skeleton_dev: internal: %lld passes over %lld voxels", passes, selected);
            return LM_ERR_DEVICE;
        }
    }
    {
        ProfScope ps(e, "skeleton_code", (double)n * h * w + (double)pvox);
        LM_LAUNCH(skel_code_kernel, dim3((unsigned)std::min(n * h, 1 << 16)), dim3(kST), 0, e->stream, (const uint8_t*)work, s, n, h, w, out);
        LM_K(hipGetLastError());
    }
    info[0] = selected, info[1] = selected - deleted, info[2] = passes;
    return LM_OK;
}

int skeleton_points(lm_engine* e, const uint8_t* skel, const float* d2, int n, int h, int w, int64_t cap, int32_t* index, uint8_t* code,
                    float* d2_out, int64_t* total) {
    *total = 0;
    const size_t nvox = (size_t)n * h * w;
    if (nvox == 0) return LM_OK;
    const int chunks = (int)((nvox + kPC - 1) / kPC);
    SkeletonWorkspace& ws = e->skel;
    LM_TRY(ws.wgcnt.reserve((size_t)chunks * sizeof(unsigned)));
    LM_TRY(ws.cnt.reserve(32));
    LM_TRY(ws.h_cnt.reserve(32));
    unsigned* wgcnt = ws.wgcnt.as<unsigned>();
    unsigned long long* cnt = ws.cnt.as<unsigned long long>();
    {
        ProfScope ps(e, "skeleton_points", (double)nvox * 2.0);
        LM_LAUNCH(points_count_kernel, dim3((unsigned)chunks), dim3(kST), 0, e->stream, skel, nvox, wgcnt);
        LM_K(hipGetLastError());
        LM_LAUNCH(points_scan_kernel, dim3(1), dim3(kST), 0, e->stream, wgcnt, chunks, cnt);
        LM_K(hipGetLastError());
        if (cap > 0) {
            LM_LAUNCH(points_write_kernel, dim3((unsigned)chunks), dim3(kST), 0, e->stream, skel, d2, nvox, (const unsigned*)wgcnt, (long long)cap,
                      index, code, d2_out);
            LM_K(hipGetLastError());
        }
    }
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, 32, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    *total = (int64_t)ws.h_cnt.as<unsigned long long>()[2];
    return LM_OK;
}

int vessel_mask(lm_engine* e, const float* V, const uint8_t* lab, int n, int h, int w, float threshold, uint8_t* out) {
    const size_t nvox = (size_t)n * h * w;
    if (nvox == 0) return LM_OK;
    ProfScope ps(e, "vessel_mask", (double)nvox * 6.0);
    LM_LAUNCH(vessel_mask_kernel, dim3(flat_grid(nvox)), dim3(kST), 0, e->stream, V, lab, nvox, threshold, out);
    LM_K(hipGetLastError());
    return LM_OK;
}

int calibre(lm_engine* e, const uint8_t* skel, const uint8_t* sel, const uint8_t keep[256], const uint8_t* lab, int n, int h, int w,
            const double* spacing, const double* edges_mm, int n_edges, int n_labels, uint8_t* class_out, float* d2_out, int64_t* counts) {
    const size_t nvox = (size_t)n * h * w, cells = (size_t)kCalLabels * kCalCols;
    std::memset(counts, 0, sizeof(int64_t) * (size_t)n_labels * kCalCols);
    if (nvox == 0) return LM_OK;
    SkeletonWorkspace& ws = e->skel;
    LM_TRY(ws.feat.reserve(nvox));
    LM_TRY(ws.cls.reserve(nvox));
    if (!d2_out) LM_TRY(ws.d2.reserve(nvox * sizeof(float)));
    LM_TRY(ws.cnt.reserve(cells * 8));
    LM_TRY(ws.h_cnt.reserve(cells * 8));
    uint8_t *feat = ws.feat.as<uint8_t>(), *cls = ws.cls.as<uint8_t>();
    float* d2 = d2_out ? d2_out : ws.d2.as<float>();
    unsigned long long* cnt = ws.cnt.as<unsigned long long>();
    Edges2 ed;
    std::memset(&ed, 0, sizeof ed);
    ed.n = n_edges;
    for (int j = 0; j < n_edges; ++j) ed.e2[j] = (float)(edges_mm[j] * edges_mm[j]);
    const LabelTable kb = label_table(keep);
    const unsigned grid = flat_grid(nvox);
    {
        ProfScope ps(e, "calibre_feat", (double)nvox * 2.0);
        LM_LAUNCH(calibre_class_kernel, dim3(grid), dim3(kST), 0, e->stream, sel, skel, (const float*)nullptr, nvox, kb, ed, 0, feat);
        LM_K(hipGetLastError());
    }
    LM_TRY(edt(e, feat, n, h, w, spacing, d2));
    {
        ProfScope ps(e, "calibre_class", (double)nvox * 7.0);
        LM_LAUNCH(calibre_class_kernel, dim3(grid), dim3(kST), 0, e->stream, sel, skel, (const float*)d2, nvox, kb, ed, 1, cls);
        LM_K(hipGetLastError());
    }
    uint8_t every[256];
    every[0] = 0;
    std::memset(every + 1, 1, 255);
    uint8_t* near = feat;  // (the features are spent)
    LM_TRY(nearest_label(e, cls, n, h, w, every, spacing, nullptr, near));
    LM_HIP(hipMemsetAsync(cnt, 0, cells * 8, e->stream));
    {
        ProfScope ps(e, "calibre_out", (double)nvox * (lab ? 4.0 : 3.0));
        LM_LAUNCH(calibre_out_kernel, dim3(grid), dim3(kST), 0, e->stream, sel, (const uint8_t*)near, lab, nvox, kb, n_labels, class_out, cnt);
        LM_K(hipGetLastError());
    }
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, cells * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* hc = ws.h_cnt.as<unsigned long long>();
    for (int l = 0; l < n_labels; ++l)
        for (int c = 0; c < kCalCols; ++c) counts[l * kCalCols + c] = (int64_t)hc[l * kCalCols + c];
    return LM_OK;
}

}  // namespace lm
