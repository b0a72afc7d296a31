// Connected components of a selection inside the labels and their per-component table (lm_components_dev, lm_component_table_dev,
// lm_relabel_dev; include/lungmask_hip.h has the definitions).
//
//   comp_select_kernel   one read of the labels (and of the image): the u8 key volume that ccl_label consumes -- 0 where a voxel is not
//                        selected, its label (per_label) or 1 otherwise -- and the per-label counts voxels / nonfinite / selected,
//                        counted in LDS and flushed once per workgroup.
//   ccl_label, ccl_rank  the engine's union-find labelling and its dense raster-order numbering (post_kernels.hip), unchanged.
//   comp_table_kernel    one row of 16 accumulators per component.  Lanes are voxels and each workgroup walks a CONTIGUOUS range, as
//                        block_run_histogram does for its one counter: inside a wave the voxels of a run of equal ids are combined by a
//                        segmented reduction over the lanes (add for the sums and the faces, min / max for the box and the HU extremes),
//                        the head of the run puts ONE record into a per-workgroup LDS hash keyed by id, and the occupied slots are
//                        flushed with global atomics at the end.  A component of 10^7 voxels therefore costs one set of global atomics
//                        per workgroup it touches instead of one per voxel on one address, and 10^6 components of one voxel cost one set
//                        each: a record that finds no slot within kProbes probes goes straight to memory, so the table is exact
//                        whatever the hash holds.  The device table has `cap` rows, never one per voxel.
//   comp_relabel_kernel  out[v] = lut[ids[v]], bounds-checked.
// Integer arithmetic throughout: no result depends on the schedule.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#include "volume_common.h"
#include "post_kernels.h"

namespace lm {
namespace {

constexpr int kTPB = 256;
constexpr int kSlots = 256;   // LDS hash slots per workgroup (26 KiB with the 17 accumulators of a slot)
constexpr int kProbes = 4;    // probes before a record bypasses the hash
constexpr int kSegsMin = 64;  // 64-voxel segments per workgroup at least (4096 voxels, region_stats' geometry)
constexpr unsigned kMaxGrid = 2048;

struct SelectParams {
    const uint8_t* lab;
    const void* vol;  // nullptr: no image
    const uint8_t* keep;  // device, 256 entries
    uint8_t* key;
    unsigned long long* counts;  // device [3][256], zeroed
    unsigned nvox;
    int dtype, lo, hi, has_lo, has_hi, per_label;
};

__global__ __launch_bounds__(kTPB) void comp_select_kernel(SelectParams p) {
    __shared__ unsigned cnt[3 * 256];
    __shared__ uint8_t keep[256];
    for (int i = threadIdx.x; i < 3 * 256; i += kTPB) cnt[i] = 0u;
    if (threadIdx.x < 256) keep[threadIdx.x] = p.keep[threadIdx.x];
    __syncthreads();
    const unsigned nseg = (p.nvox + 63u) / 64u;
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * (unsigned)kTPB + threadIdx.x) >> 6, nwaves = (gridDim.x * (unsigned)kTPB) >> 6;
    for (unsigned seg = wave; seg < nseg; seg += nwaves) {
        const unsigned v = seg * 64u + lane;
        const bool valid = v < p.nvox;
        const int L = valid ? (int)p.lab[v] : 0;
        bool nan = false;
        int hu = 0;
        if (valid && p.vol) hu = load_hu(p.vol, p.dtype, v, nan);
        const bool sel = valid && keep[L] != 0 && !nan && (!p.vol || ((!p.has_lo || hu >= p.lo) && (!p.has_hi || hu <= p.hi)));
        if (valid) p.key[v] = sel ? (uint8_t)(p.per_label ? L : 1) : (uint8_t)0;
        // a wave of one label (nearly all of them) counts with three LDS atomics, not 3 x 64 on one address
        const int L0 = __shfl(L, 0);
        const unsigned long long bv = __ballot(valid), bn = __ballot(valid && nan), bs = __ballot(sel);
        if (__all(!valid || L == L0)) {
            if (lane == 0) {
                atomicAdd(&cnt[L0], (unsigned)__popcll(bv));
                if (bn) atomicAdd(&cnt[256 + L0], (unsigned)__popcll(bn));
                if (bs) atomicAdd(&cnt[512 + L0], (unsigned)__popcll(bs));
            }
        } else if (valid) {
            atomicAdd(&cnt[L], 1u);
            if (nan) atomicAdd(&cnt[256 + L], 1u);
            if (sel) atomicAdd(&cnt[512 + L], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256; i += kTPB)
        if (cnt[i]) atomicAdd(&p.counts[i], (unsigned long long)cnt[i]);
}

// ---- the per-component table ----------------------------------------------------------------------------------------------------
// the 8 sums and 9 extremes of a row; S_* index hsum, E_* index hext
enum { S_VOX, S_SZ, S_SY, S_SX, S_HU, S_FZ, S_FY, S_FX, kSums };
enum { E_FIRST, E_Z0, E_Y0, E_X0, E_HMIN, E_Z1, E_Y1, E_X1, E_HMAX, kExts };  // the first five are minima

struct Rec {
    long long s[kSums];
    int e[kExts];
};

__device__ __forceinline__ void row_commit(lm_component* row, const Rec& r) {
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->voxels), (unsigned long long)r.s[S_VOX]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->index_sum[0]), (unsigned long long)r.s[S_SZ]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->index_sum[1]), (unsigned long long)r.s[S_SY]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->index_sum[2]), (unsigned long long)r.s[S_SX]);
    if (r.s[S_HU]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->hu_sum), (unsigned long long)r.s[S_HU]);
    if (r.s[S_FZ]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->faces[0]), (unsigned long long)r.s[S_FZ]);
    if (r.s[S_FY]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->faces[1]), (unsigned long long)r.s[S_FY]);
    if (r.s[S_FX]) atomicAdd(reinterpret_cast<unsigned long long*>(&row->faces[2]), (unsigned long long)r.s[S_FX]);
    atomicMin(&row->first, r.e[E_FIRST]);
    atomicMin(&row->bbox[0], r.e[E_Z0]);
    atomicMax(&row->bbox[1], r.e[E_Z1]);
    atomicMin(&row->bbox[2], r.e[E_Y0]);
    atomicMax(&row->bbox[3], r.e[E_Y1]);
    atomicMin(&row->bbox[4], r.e[E_X0]);
    atomicMax(&row->bbox[5], r.e[E_X1]);
    if (r.e[E_HMIN] <= r.e[E_HMAX]) {
        atomicMin(&row->hu_min, r.e[E_HMIN]);
        atomicMax(&row->hu_max, r.e[E_HMAX]);
    }
}

struct TableParams {
    const int* ids;
    const void* vol;  // nullptr: no image
    lm_component* rows;  // [cap], preset by comp_table_init_kernel
    int* maxid;       // device, zeroed
    unsigned nvox, segs_per_wg;
    int dtype, N, H, W, cap;
};

// rows preset for the atomics: sums 0, minima INT_MAX, maxima (inclusive here) INT_MIN
__global__ __launch_bounds__(kTPB) void comp_table_init_kernel(lm_component* rows, int cap) {
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= cap) return;
    lm_component r;
    r.voxels = r.hu_sum = 0;
    for (int k = 0; k < 3; ++k) r.index_sum[k] = r.faces[k] = 0;
    for (int k = 0; k < 3; ++k) {
        r.bbox[2 * k] = INT_MAX;
        r.bbox[2 * k + 1] = INT_MIN;
    }
    r.hu_min = INT_MAX;
    r.hu_max = INT_MIN;
    r.label = 0;
    r.first = INT_MAX;
    rows[i] = r;
}

// exclusive maxima, the label of the first voxel, and the values of the fields nothing contributed to
__global__ __launch_bounds__(kTPB) void comp_table_finish_kernel(lm_component* rows, const uint8_t* __restrict__ lab, int cap) {
    const int i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= cap) return;
    lm_component r = rows[i];
    if (r.voxels == 0) {
        for (int k = 0; k < 6; ++k) r.bbox[k] = -1;
        r.first = -1;
    } else {
        for (int k = 0; k < 3; ++k) r.bbox[2 * k + 1] += 1;
        r.label = lab[r.first];
    }
    if (r.hu_min > r.hu_max) r.hu_min = r.hu_max = 0;
    rows[i] = r;
}

__global__ __launch_bounds__(kTPB) void comp_table_kernel(TableParams p) {
    __shared__ int hkey[kSlots];  // 0: empty (ids are >= 1)
    __shared__ unsigned long long hsum[kSums][kSlots];
    __shared__ int hext[kExts][kSlots];
    for (int i = threadIdx.x; i < kSlots; i += kTPB) {
        hkey[i] = 0;
#pragma unroll
        for (int k = 0; k < kSums; ++k) hsum[k][i] = 0ull;
#pragma unroll
        for (int k = 0; k < kExts; ++k) hext[k][i] = k <= E_HMIN ? INT_MAX : INT_MIN;
    }
    __syncthreads();
    const unsigned nseg = (p.nvox + 63u) / 64u;
    const unsigned seg0 = blockIdx.x * p.segs_per_wg;
    const unsigned seg1 = seg0 + p.segs_per_wg < nseg ? seg0 + p.segs_per_wg : nseg;  // (seg0 + segs_per_wg < 2^26: no wrap)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = p.W, HW = p.H * p.W;
    int mx = 0;
    for (unsigned seg = seg0 + wave; seg < seg1; seg += kTPB / 64) {
        const unsigned v = seg * 64u + lane;
        const int raw = v < p.nvox ? p.ids[v] : 0;
        mx = max(mx, raw);
        const int id = (raw > 0 && raw <= p.cap) ? raw : 0;
        if (__ballot(id != 0) == 0ull) continue;  // (wave-uniform)
        Rec r;
#pragma unroll
        for (int k = 0; k < kSums; ++k) r.s[k] = 0;
#pragma unroll
        for (int k = 0; k < kExts; ++k) r.e[k] = k <= E_HMIN ? INT_MAX : INT_MIN;
        if (id) {
            const unsigned q = v / (unsigned)W;
            const int x = (int)(v - q * (unsigned)W), z = (int)(q / (unsigned)p.H), y = (int)(q - (unsigned)z * (unsigned)p.H);
            r.s[S_VOX] = 1;
            r.s[S_SZ] = z;
            r.s[S_SY] = y;
            r.s[S_SX] = x;
            // faces whose other side is outside the volume or carries another id (the RAW id: a component beyond cap is still another)
            r.s[S_FZ] = ((z == 0 || p.ids[v - HW] != raw) ? 1 : 0) + ((z == p.N - 1 || p.ids[v + HW] != raw) ? 1 : 0);
            r.s[S_FY] = ((y == 0 || p.ids[v - W] != raw) ? 1 : 0) + ((y == p.H - 1 || p.ids[v + W] != raw) ? 1 : 0);
            r.s[S_FX] = ((x == 0 || p.ids[v - 1] != raw) ? 1 : 0) + ((x == W - 1 || p.ids[v + 1] != raw) ? 1 : 0);
            r.e[E_FIRST] = (int)v;
            r.e[E_Z0] = r.e[E_Z1] = z;
            r.e[E_Y0] = r.e[E_Y1] = y;
            r.e[E_X0] = r.e[E_X1] = x;
            if (p.vol) {
                bool nan;
                const int hu = load_hu(p.vol, p.dtype, v, nan);
                if (!nan) {
                    r.s[S_HU] = hu;
                    r.e[E_HMIN] = r.e[E_HMAX] = hu;
                }
            }
        }
        // runs of equal ids inside the wave: `end` = the lane after this lane's run
        const int prev = __shfl_up(id, 1);
        const bool head = lane == 0 || prev != id;
        const unsigned long long heads = __ballot(head);
        const unsigned long long higher = lane == 63 ? 0ull : (heads >> (lane + 1));
        const int end = higher ? lane + __ffsll((long long)higher) : 64;
        // segmented reduction towards the head: after the step `off` a lane holds its run's lanes [lane, min(lane + 2 off, end))
        // (the voxel count is the run's length; the index and face sums of 64 lanes fit 32 bits, the HU sum does not)
        for (int off = 1; off < 64; off <<= 1) {
            const bool take = lane + off < end;
#pragma unroll
            for (int k = S_SZ; k < kSums; ++k) {
                if (k == S_HU) {
                    const long long o = __shfl_down(r.s[k], off);
                    if (take) r.s[k] += o;
                } else {
                    const int o = __shfl_down((int)r.s[k], off);
                    if (take) r.s[k] += o;
                }
            }
#pragma unroll
            for (int k = 0; k < kExts; ++k) {
                const int o = __shfl_down(r.e[k], off);
                if (take) r.e[k] = k <= E_HMIN ? min(r.e[k], o) : max(r.e[k], o);
            }
        }
        if (head && id) {
            r.s[S_VOX] = end - lane;
            unsigned h =((unsigned)id * 2654435761u) >> 24;  // 8 bits
            bool placed = false;
            for (int probe = 0; probe < kProbes && !placed; ++probe) {
                const int old = atomicCAS(&hkey[h], 0, id);
                if (old == 0 || old == id) placed = true;
                else h = (h + 1) & (kSlots - 1);
            }
            if (placed) {
#pragma unroll
                for (int k = 0; k < kSums; ++k)
                    if (r.s[k]) atomicAdd(&hsum[k][h], (unsigned long long)r.s[k]);
#pragma unroll
                for (int k = 0; k < kExts; ++k) {
                    if (k <= E_HMIN) atomicMin(&hext[k][h], r.e[k]);
                    else atomicMax(&hext[k][h], r.e[k]);
                }
            } else {
                row_commit(p.rows + (id - 1), r);  // no slot within kProbes: straight to memory
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSlots; i += kTPB) {
        const int id = hkey[i];
        if (!id) continue;
        Rec r;
#pragma unroll
        for (int k = 0; k < kSums; ++k) r.s[k] = (long long)hsum[k][i];
#pragma unroll
        for (int k = 0; k < kExts; ++k) r.e[k] = hext[k][i];
        row_commit(p.rows + (id - 1), r);
    }
    // the largest id this workgroup saw
    for (int m = 32; m >= 1; m >>= 1) mx = max(mx, __shfl_xor(mx, m));
    if (lane == 0 && mx > 0) atomicMax(p.maxid, mx);
}

__global__ __launch_bounds__(kTPB) void comp_relabel_kernel(const int* ids, const int* __restrict__ lut, unsigned lut_len, unsigned nvox, int* out,
                                                            int* flag) {
    bool bad = false;
    for (unsigned v = blockIdx.x * (unsigned)kTPB + threadIdx.x; v < nvox; v += gridDim.x * (unsigned)kTPB) {
        const int id = ids[v];
        const bool in = (unsigned)id < lut_len;  // (a negative id is a large unsigned one)
        bad |= !in;
        out[v] = in ? lut[id] : 0;
    }
    if (bad) atomicOr(flag, 1);
}

void table_geometry(size_t nvox, unsigned* grid, unsigned* segs_per_wg) {
    const size_t nseg = (nvox + 63) / 64;
    size_t g = std::max<size_t>(1, std::min<size_t>((nseg + kSegsMin - 1) / kSegsMin, kMaxGrid));
    const size_t per = std::max<size_t>(1, (nseg + g - 1) / g);
    g = std::max<size_t>(1, (nseg + per - 1) / per);  // no workgroup without a range
    *grid = (unsigned)g;
    *segs_per_wg = (unsigned)per;
}

}  // namespace

void component_table_launch(size_t nvox, long long* workgroups, long long* voxels_per_workgroup) {
    unsigned grid, per;
    table_geometry(nvox, &grid, &per);
    *workgroups = nvox ? grid : 0;
    *voxels_per_workgroup = (long long)per * 64;
}

int components(lm_engine* e, const uint8_t* lab, const void* vol, int dtype, int n, int h, int w, const lm_components_params& p, int32_t* ids,
               int64_t* total_out, int64_t* counts_host) {
    const size_t nvox = (size_t)n * h * w;
    *total_out = 0;
    std::memset(counts_host, 0, 3 * 256 * sizeof(int64_t));
    if (nvox == 0) return LM_OK;
    ComponentsWorkspace& ws = e->comp;
    const size_t scal_bytes = 3 * 256 * 8 + 256 + 16;  // counts | keep table | total
    LM_TRY(ws.key.reserve(nvox));
    LM_TRY(ws.parent.reserve(nvox * 4));
    LM_TRY(ws.rank.reserve(nvox * 4));
    LM_TRY(ws.blockcnt.reserve((rank_blocks(nvox) + 1) * 4));
    LM_TRY(ws.scal.reserve(scal_bytes));
    LM_TRY(ws.h_scal.reserve(scal_bytes));
    char* scal = ws.scal.as<char>();
    char* h_scal = ws.h_scal.as<char>();
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(scal);
    uint8_t* keep_dev = reinterpret_cast<uint8_t*>(scal + 3 * 256 * 8);
    int* total_dev = reinterpret_cast<int*>(scal + 3 * 256 * 8 + 256);
    std::memset(h_scal, 0, scal_bytes);
    std::memcpy(h_scal + 3 * 256 * 8, p.keep, 256);
    LM_HIP(hipMemcpyAsync(scal, h_scal, scal_bytes, hipMemcpyHostToDevice, e->stream));
    const Dims d{n, h, w};
    {
        ProfScope ps(e, "comp_select", (double)nvox * (2.0 + (vol ? dtype_bytes(dtype) : 0)));
        SelectParams sp{lab, vol, keep_dev, ws.key.as<uint8_t>(), counts, (unsigned)nvox, dtype, p.lo, p.hi, p.has_lo, p.has_hi, p.per_label};
        const size_t nseg = (nvox + 63) / 64;
        const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((nseg + 15) / 16, kMaxGrid));
        LM_LAUNCH(comp_select_kernel, dim3(grid), dim3(kTPB), 0, e->stream, sp);
        LM_K(hipGetLastError());
    }
    {
        ProfScope ps(e, "ccl_label", (double)nvox * 5.0);
        LM_K(ccl_label(ws.key.as<uint8_t>(), ws.parent.as<int>(), d, p.connectivity == 26, e->stream, false));
    }
    {
        ProfScope ps(e, "ccl_rank", (double)nvox * 16.0);
        LM_K(ccl_rank(ws.parent.as<int>(), ws.rank.as<int>(), ids, ws.blockcnt.as<int>(), total_dev, nvox, e->stream, false));
    }
    LM_HIP(hipMemcpyAsync(h_scal, scal, scal_bytes, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(counts_host, h_scal, 3 * 256 * 8);
    int total;
    std::memcpy(&total, h_scal + 3 * 256 * 8 + 256, 4);
    *total_out = total;
    return LM_OK;
}

int component_table(lm_engine* e, const int32_t* ids, const uint8_t* lab, const void* vol, int dtype, int n, int h, int w,
                    lm_component* table_host, int64_t cap64, int64_t* total_out) {
    const size_t nvox = (size_t)n * h * w;
    *total_out = 0;
    if (nvox == 0) return LM_OK;
    const int cap = (int)cap64;
    ComponentsWorkspace& ws = e->comp;
    LM_TRY(ws.rows.reserve(std::max<size_t>(1, (size_t)cap) * sizeof(lm_component)));
    LM_TRY(ws.scal.reserve(3 * 256 * 8 + 256 + 16));
    LM_TRY(ws.h_scal.reserve(3 * 256 * 8 + 256 + 16));
    lm_component* rows = ws.rows.as<lm_component>();
    int* maxid = ws.scal.as<int>();
    LM_HIP(hipMemsetAsync(maxid, 0, 4, e->stream));
    unsigned grid, per;
    table_geometry(nvox, &grid, &per);
    {
        ProfScope ps(e, "comp_table", (double)nvox * (4.0 + (vol ? dtype_bytes(dtype) : 0)) + (double)cap * 2.0 * sizeof(lm_component));
        if (cap > 0) {
            LM_LAUNCH(comp_table_init_kernel, dim3((cap + kTPB - 1) / kTPB), dim3(kTPB), 0, e->stream, rows, cap);
            LM_K(hipGetLastError());
        }
        TableParams tp{ids, vol, rows, maxid, (unsigned)nvox, per, dtype, n, h, w, cap};
        LM_LAUNCH(comp_table_kernel, dim3(grid), dim3(kTPB), 0, e->stream, tp);
        LM_K(hipGetLastError());
        if (cap > 0) {
            LM_LAUNCH(comp_table_finish_kernel, dim3((cap + kTPB - 1) / kTPB), dim3(kTPB), 0, e->stream, rows, lab, cap);
            LM_K(hipGetLastError());
        }
    }
    LM_HIP(hipMemcpyAsync(ws.h_scal.p, maxid, 4, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const int total = *ws.h_scal.as<int>();
    *total_out = total;
    const int nrows = std::min(total, cap);
    if (nrows > 0) {
        LM_HIP(hipMemcpyAsync(table_host, rows, (size_t)nrows * sizeof(lm_component), hipMemcpyDeviceToHost, e->stream));
        LM_HIP(hipStreamSynchronize(e->stream));
    }
    return LM_OK;
}

int relabel(lm_engine* e, const int32_t* ids, const int32_t* lut, int64_t lut_len, int64_t nvox, int32_t* out) {
    if (nvox == 0) return LM_OK;
    ComponentsWorkspace& ws = e->comp;
    LM_TRY(ws.scal.reserve(3 * 256 * 8 + 256 + 16));
    LM_TRY(ws.h_scal.reserve(3 * 256 * 8 + 256 + 16));
    int* flag = ws.scal.as<int>();
    LM_HIP(hipMemsetAsync(flag, 0, 4, e->stream));
    {
        ProfScope ps(e, "comp_relabel", (double)nvox * 8.0);
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nvox + kTPB - 1) / kTPB, 8192));
        LM_LAUNCH(comp_relabel_kernel, dim3(grid), dim3(kTPB), 0, e->stream, ids, lut, (unsigned)lut_len, (unsigned)nvox, out, flag);
        LM_K(hipGetLastError());
    }
    LM_HIP(hipMemcpyAsync(ws.h_scal.p, flag, 4, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    if (*ws.h_scal.as<int>()) {
        set_error("lm_relabel_dev: id outside the table (an id is negative or >= lut_len = %lld); such voxels were written as 0", (long long)lut_len);
        return LM_ERR_INVALID;
    }
    return LM_OK;
}

}  // namespace lm
