// Seeded minimax flood and the airway mask (lm_seed_cost_dev, lm_airway_mask_dev; include/lungmask_hip.h has the definitions).
//   seed_init_kernel    vol -> xenc int16 (workspace): max(hu, -1024) of a passable voxel, 32767 of an impassable one (NaN or
//                       hu > cap_hu), so "impassable" needs no flag: max(32767, .) never goes below 32767.  cost = 32767 everywhere.
//   seed_plant_kernel   ONE workgroup: cost[s] = xenc[s] at every passable seed; the seed's brick AND its six face neighbours enter the
//                       first work-list (a seed's own value never "changes", so the neighbours would not learn of it otherwise).
//   seed_round_kernel   one workgroup per brick of the round's work-list.  Loads the brick's (xenc, cost) and the six FACE halos (edge
//                       and corner cells are never read: the relation is 6-connected) as one packed dword per cell, relaxes to the
//                       local fixed point, writes back the own voxels that fell, and puts the face neighbour behind every face on
//                       which a voxel fell into the next work-list.
//   seed_hist_kernel    cost -> the curve: a histogram of cap_hu + 1025 bins in LDS (16384 bytes for the largest cap), flushed once per workgroup.
//   airway_mask_kernel  cost, labels, threshold -> the u8 mask and its per-label counts in LDS (comp_select_kernel's pattern).
// CHOICES.
//   Brick 8 x 8 x 32 (z, y, x), 2048 voxels, 256 threads.  32 along x: a row of a brick is one 64-byte run of int16 and 32 lanes of
//     a y or z sweep read 32 consecutive LDS dwords.  8 x 8 across: the halo is 1152 cells on 2048, 56 % more loads than voxels,
//     and LDS stays small enough for occupancy not to be bounded by it.
//   LDS cell = (xenc << 16) | (cost & 0xffff), one dword: one ds_read_b32 brings both, and a relaxation rewrites the whole dword (the
//     xenc half never changes).  Layout [10][10][35]: rows of 34 cells padded to 35.  ds_read_b32 / ds_write_b32 bank = dword mod 32
//     within each half wave: the y and z sweeps give a half wave 32 consecutive dwords of one row (conflict-free whatever the
//     stride); the x sweep gives it (y = lane & 7, segment = lane >> 3), dword 35 y + 8 segment + i = 3 y + 8 segment (mod 32), and
//     3 y mod 8 takes every residue once: conflict-free as well.  LDS per workgroup of a round: 10 * 10 * 35 * 4 + 16 (flags) = 14016 bytes.
//   Local relaxation: directional sweeps.  The brick is cut into lines of 8 cells along an axis (x: four segments per row), 256 lines
//     per axis, one thread each: the thread carries the running value forward from the cell in front of its line and backward from
//     the cell behind it, c = max(xenc, min(c, carried)).  One x, y, z triple of sweeps moves a value along any monotone staircase;
//     the triples repeat until one changes nothing (a flag in LDS, three flags in rotation so that resetting one never races
//     with reading it).  A line reads cells that other lines write in the same sweep: whatever it sees is a path's cost.
//   Work-list: compacted.  list[r & 1] holds the bricks of round r; a brick is appended when atomicExch(stamp[brick], r + 1) returns
//     another value, so it appears once.  The host reads back ONE counter per round (the length of the next list, which is also the
//     next grid) and stops on zero.  A brick that changed does not re-run by itself: it is at its local fixed point for the halo it
//     read, and a halo cell that falls later brings the brick back through that neighbour's append.
//   In place.  cost is read (halo) by one workgroup while its owner writes it.  int16 stores are single; every value ever stored is
//     the cost of a real path, so a reader sees an upper bound, and the append made behind the store runs the reader again in the
//     next round, which starts behind a kernel boundary.  The fixed point is unique, so the result does not depend on the schedule.
// No kernel waits on another workgroup; the round loop is the host's, bounded by max_rounds.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kAT = 256;                      // every kernel: 4 waves
constexpr int kBZ = 8, kBY = 8, kBX = 32;     // the brick
constexpr int kRow = kBX + 3;                 // LDS row: 34 cells + 1 of padding
constexpr int kPlane = (kBY + 2) * kRow;
constexpr int kCells = (kBZ + 2) * kPlane;    // 3500 dwords
constexpr int kUnreached = 32767;
constexpr int kMaxSeeds = 64;
constexpr int kHistMax = 3071 + 1025;         // bins of the largest cap_hu

struct Bricks {
    int N, H, W;     // the volume
    int nz, ny, nx;  // bricks per axis
};

struct SeedList {
    long long v[kMaxSeeds];
    int n;
};

__device__ __forceinline__ unsigned pack_cell(int xenc, int cost) { return ((unsigned)xenc << 16) | ((unsigned)cost & 0xffffu); }
__device__ __forceinline__ int cell_cost(unsigned c) { return (int)(short)(c & 0xffffu); }
__device__ __forceinline__ int cell_x(unsigned c) { return (int)c >> 16; }

// brick (bz, by, bx) enters the list of round `round` unless it is there already
__device__ __forceinline__ void append_brick(const Bricks& g, int bz, int by, int bx, unsigned round, unsigned* stamp, unsigned* list,
                                             unsigned* count) {
    if (bz < 0 || by < 0 || bx < 0 || bz >= g.nz || by >= g.ny || bx >= g.nx) return;
    const unsigned b = ((unsigned)bz * g.ny + by) * g.nx + bx;
    if (atomicExch(&stamp[b], round) != round) list[atomicAdd(count, 1u)] = b;
}

__global__ __launch_bounds__(kAT) void seed_init_kernel(const void* __restrict__ vol, int dtype, size_t nvox, int cap_hu,
                                                        int16_t* __restrict__ xenc, int16_t* __restrict__ cost) {
    for (size_t v = (size_t)blockIdx.x * kAT + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kAT) {
        bool nan;
        const int hu = load_hu(vol, dtype, v, nan);
        xenc[v] = (int16_t)((nan || hu > cap_hu) ? kUnreached : (hu < -1024 ? -1024 : hu));
        cost[v] = (int16_t)kUnreached;
    }
}

// cnt[0], cnt[1]: the lengths of the two work-lists; cnt[2]: passable seeds
__global__ __launch_bounds__(kAT) void seed_plant_kernel(SeedList seeds, Bricks g, const int16_t* __restrict__ xenc, int16_t* cost,
                                                         unsigned* stamp, unsigned* list, unsigned* cnt) {
    const int t = threadIdx.x;
    if (t >= seeds.n) return;
    const long long v = seeds.v[t];
    const int x = xenc[v];
    if (x == kUnreached) return;
    atomicAdd(&cnt[2], 1u);
    cost[v] = (int16_t)x;  // (a duplicate stores the same value)
    const int vx = (int)(v % g.W), vy = (int)((v / g.W) % g.H), vz = (int)(v / ((long long)g.W * g.H));
    const int bz = vz / kBZ, by = vy / kBY, bx = vx / kBX;
    append_brick(g, bz, by, bx, 1u, stamp, list, &cnt[1]);
    append_brick(g, bz - 1, by, bx, 1u, stamp, list, &cnt[1]);
    append_brick(g, bz + 1, by, bx, 1u, stamp, list, &cnt[1]);
    append_brick(g, bz, by - 1, bx, 1u, stamp, list, &cnt[1]);
    append_brick(g, bz, by + 1, bx, 1u, stamp, list, &cnt[1]);
    append_brick(g, bz, by, bx - 1, 1u, stamp, list, &cnt[1]);
    append_brick(g, bz, by, bx + 1, 1u, stamp, list, &cnt[1]);
}

// One line of 8 cells, `step` dwords apart, first cell at p: forward from the cell in front, backward from the cell behind.
__device__ __forceinline__ bool sweep_line(unsigned* p, int step) {
    bool changed = false;
    int carry = cell_cost(p[-step]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned c = p[i * step];
        const int x = cell_x(c), old = cell_cost(c);
        const int nc = max(x, min(old, carry));
        if (nc < old) {
            p[i * step] = pack_cell(x, nc);
            changed = true;
        }
        carry = nc;
    }
    carry = cell_cost(p[8 * step]);
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        const unsigned c = p[i * step];
        const int x = cell_x(c), old = cell_cost(c);
        const int nc = max(x, min(old, carry));
        if (nc < old) {
            p[i * step] = pack_cell(x, nc);
            changed = true;
        }
        carry = nc;
    }
    return changed;
}

// cell (lz, ly, lx), each from -1 (halo) to the brick's extent (halo)
__device__ __forceinline__ int cell_index(int lz, int ly, int lx) { return (lz + 1) * kPlane + (ly + 1) * kRow + (lx + 1); }

__global__ __launch_bounds__(kAT) void seed_round_kernel(Bricks g, const int16_t* __restrict__ xenc, int16_t* cost, unsigned round,
                                                         unsigned* stamp, const unsigned* __restrict__ list_now, unsigned* list_next,
                                                         unsigned* count_next) {
    __shared__ unsigned cells[kCells];
    __shared__ unsigned flag[3];
    __shared__ unsigned faces;
    const int t = threadIdx.x;
    const unsigned b = list_now[blockIdx.x];
    const int bx = (int)(b % g.nx), by = (int)((b / g.nx) % g.ny), bz = (int)(b / ((unsigned)g.nx * g.ny));
    const int z0 = bz * kBZ, y0 = by * kBY, x0 = bx * kBX;
    if (t < 3) flag[t] = 0u;
    if (t == 3) faces = 0u;

    // a cell of the volume, or "impassable" outside of it (nothing exists there)
    auto load_cell = [&](int lz, int ly, int lx) {
        const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
        unsigned c = pack_cell(kUnreached, kUnreached);
        if (z >= 0 && y >= 0 && x >= 0 && z < g.N && y < g.H && x < g.W) {
            const size_t v = ((size_t)z * g.H + y) * g.W + x;
            c = pack_cell(xenc[v], cost[v]);
        }
        cells[cell_index(lz, ly, lx)] = c;
    };
    // own voxels: thread t holds (lz = j, ly = t >> 5, lx = t & 31), j = 0 .. 7
    const int ox = t & 31, oy = t >> 5;
    int old[kBZ];
#pragma unroll
    for (int j = 0; j < kBZ; ++j) {
        load_cell(j, oy, ox);
        old[j] = cell_cost(cells[cell_index(j, oy, ox)]);
    }
    // halos: the z faces (2 x 256 cells), the y faces (2 x 256), the x faces (2 x 64)
    load_cell(-1, oy, ox);
    load_cell(kBZ, oy, ox);
    load_cell(oy, -1, ox);
    load_cell(oy, kBY, ox);
    if (t < 128) load_cell((t >> 3) & 7, t & 7, (t >> 6) ? kBX : -1);
    __syncthreads();

    // the three line families (see the head comment for the banks)
    unsigned* const px = cells + cell_index(t >> 5, t & 7, ((t >> 3) & 3) * 8);
    unsigned* const py = cells + cell_index(t >> 5, 0, t & 31);
    unsigned* const pz = cells + cell_index(0, t >> 5, t & 31);
    for (int it = 0;; ++it) {
        bool ch = sweep_line(px, 1);
        __syncthreads();
        ch |= sweep_line(py, kRow);
        __syncthreads();
        ch |= sweep_line(pz, kPlane);
        if (t == 0) flag[(it + 1) % 3] = 0u;
        if (ch) flag[it % 3] = 1u;
        __syncthreads();
        if (flag[it % 3] == 0u) break;
    }

    unsigned mine = 0u;  // bit d: a voxel on face d (-z, +z, -y, +y, -x, +x) fell
#pragma unroll
    for (int j = 0; j < kBZ; ++j) {
        const int z = z0 + j, y = y0 + oy, x = x0 + ox;
        if (z >= g.N || y >= g.H || x >= g.W) continue;
        const int nc = cell_cost(cells[cell_index(j, oy, ox)]);
        if (nc >= old[j]) continue;
        cost[((size_t)z * g.H + y) * g.W + x] = (int16_t)nc;
        mine |= (j == 0 ? 1u : 0u) | (j == kBZ - 1 ? 2u : 0u) | (oy == 0 ? 4u : 0u) | (oy == kBY - 1 ? 8u : 0u) | (ox == 0 ? 16u : 0u) |
                (ox == kBX - 1 ? 32u : 0u);
    }
    if (mine) atomicOr(&faces, mine);
    __syncthreads();
    if (t < 6 && ((faces >> t) & 1u)) {
        const int d = (t & 1) ? 1 : -1, a = t >> 1;
        append_brick(g, bz + (a == 0 ? d : 0), by + (a == 1 ? d : 0), bx + (a == 2 ? d : 0), round + 1u, stamp, list_next, count_next);
    }
}

__global__ __launch_bounds__(kAT) void seed_hist_kernel(const int16_t* __restrict__ cost, size_t nvox, int bins,
                                                        unsigned long long* __restrict__ curve) {
    __shared__ unsigned hist[kHistMax];
    for (int i = threadIdx.x; i < bins; i += kAT) hist[i] = 0u;
    __syncthreads();
    // (a workgroup adds fewer than 2^32 voxels: n * h * w < 2^31)
    for (size_t v = (size_t)blockIdx.x * kAT + threadIdx.x; v < nvox; v += (size_t)gridDim.x * kAT) {
        const int k = (int)cost[v] + 1024;
        if (k >= 0 && k < bins) atomicAdd(&hist[k], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += kAT)
        if (hist[i]) atomicAdd(&curve[i], (unsigned long long)hist[i]);
}

__global__ __launch_bounds__(kAT) void airway_mask_kernel(const int16_t* __restrict__ cost, const uint8_t* __restrict__ lab, unsigned nvox,
                                                          int threshold, uint8_t* __restrict__ mask, unsigned long long* __restrict__ counts) {
    __shared__ unsigned cnt[256];
    for (int i = threadIdx.x; i < 256; i += kAT) cnt[i] = 0u;
    __syncthreads();
    const unsigned nseg = (nvox + 63u) / 64u;
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * (unsigned)kAT + threadIdx.x) >> 6, nwaves = (gridDim.x * (unsigned)kAT) >> 6;
    for (unsigned seg = wave; seg < nseg; seg += nwaves) {
        const unsigned v = seg * 64u + lane;
        const bool valid = v < nvox;
        const bool in = valid && (int)cost[v] <= threshold;
        if (valid) mask[v] = in ? (uint8_t)1 : (uint8_t)0;
        const int L = (in && lab) ? (int)lab[v] : 0;
        // a wave of one label (nearly all of them) counts with one LDS atomic
        const unsigned long long bi = __ballot(in);
        if (bi == 0ull) continue;
        const int L0 = __shfl(L, __ffsll((long long)bi) - 1);
        if (__all(!in || L == L0)) {
            if (lane == 0) atomicAdd(&cnt[L0], (unsigned)__popcll(bi));
        } else if (in) {
            atomicAdd(&cnt[L], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += kAT)
        if (cnt[i]) atomicAdd(&counts[i], (unsigned long long)cnt[i]);
}

unsigned flat_grid(size_t nvox) { return (unsigned)std::max<size_t>(1, std::min<size_t>((nvox + kAT - 1) / kAT, 4096)); }

}  // namespace

void seed_cost_bricks(int n, int h, int w, long long* bricks, int brick[3]) {
    *bricks = (long long)((n + kBZ - 1) / kBZ) * ((h + kBY - 1) / kBY) * ((w + kBX - 1) / kBX);
    brick[0] = kBZ, brick[1] = kBY, brick[2] = kBX;
}

int seed_cost(lm_engine* e, const void* vol, int dtype, int n, int h, int w, const int64_t* seeds, int n_seeds, int cap_hu, int64_t max_rounds,
              int16_t* cost, int64_t* curve, int64_t info[4]) {
    const int bins = cap_hu + 1025;
    std::memset(curve, 0, sizeof(int64_t) * (size_t)bins);
    info[0] = info[1] = info[2] = 0;
    info[3] = 1;
    const size_t nvox = (size_t)n * h * w;
    if (nvox == 0) return LM_OK;
    Bricks g{n, h, w, (n + kBZ - 1) / kBZ, (h + kBY - 1) / kBY, (w + kBX - 1) / kBX};
    const size_t nbricks = (size_t)g.nz * g.ny * g.nx;
    AirwayWorkspace& ws = e->airway;
    LM_TRY(ws.xenc.reserve(nvox * sizeof(int16_t)));
    LM_TRY(ws.stamp.reserve(nbricks * sizeof(unsigned)));
    LM_TRY(ws.list.reserve(2 * nbricks * sizeof(unsigned)));
    LM_TRY(ws.cnt.reserve(kHistMax * 8));
    LM_TRY(ws.h_cnt.reserve(kHistMax * 8));
    int16_t* xenc = ws.xenc.as<int16_t>();
    unsigned *stamp = ws.stamp.as<unsigned>(), *list = ws.list.as<unsigned>(), *cnt = ws.cnt.as<unsigned>();
    SeedList sl;
    std::memset(&sl, 0, sizeof sl);
    sl.n = n_seeds;
    for (int i = 0; i < n_seeds; ++i) sl.v[i] = seeds[i];
    LM_HIP(hipMemsetAsync(stamp, 0, nbricks * sizeof(unsigned), e->stream));
    LM_HIP(hipMemsetAsync(cnt, 0, 16, e->stream));
    {
        ProfScope ps(e, "seed_init", (double)nvox * (dtype_bytes(dtype) + 4.0));
        LM_LAUNCH(seed_init_kernel, dim3(flat_grid(nvox)), dim3(kAT), 0, e->stream, vol, dtype, nvox, cap_hu, xenc, cost);
        LM_K(hipGetLastError());
        LM_LAUNCH(seed_plant_kernel, dim3(1), dim3(kAT), 0, e->stream, sl, g, (const int16_t*)xenc, cost, stamp, list + nbricks, cnt);
        LM_K(hipGetLastError());
    }
    const unsigned* hc = ws.h_cnt.as<unsigned>();
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, 16, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    info[2] = hc[2];
    unsigned active = hc[1];  // the length of list[round & 1], round = 1
    long long rounds = 0;
    while (active != 0) {
        if (rounds >= max_rounds) {
            info[0] = rounds, info[3] = 0;
            set_error("lm_seed_cost_dev: max_rounds (%lld) spent before the fixed point: %u bricks still to run", (long long)max_rounds, active);
            return LM_ERR_INVALID;
        }
        const unsigned r = (unsigned)(rounds + 1);  // (rounds < n * h * w + 2 < 2^32 for any run that converges)
        unsigned *now = list + (size_t)(r & 1u) * nbricks, *next = list + (size_t)((r + 1u) & 1u) * nbricks;
        LM_HIP(hipMemsetAsync(cnt + ((r + 1u) & 1u), 0, 4, e->stream));
        {
            ProfScope ps(e, "seed_round", (double)active * (2048.0 + 1152.0) * 4.0);
            LM_LAUNCH(seed_round_kernel, dim3(active), dim3(kAT), 0, e->stream, g, (const int16_t*)xenc, cost, r, stamp, (const unsigned*)now, next,
                      cnt + ((r + 1u) & 1u));
            LM_K(hipGetLastError());
        }
        LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, 8, hipMemcpyDeviceToHost, e->stream));
        LM_HIP(hipStreamSynchronize(e->stream));
        active = hc[(r + 1u) & 1u];
        ++rounds;
    }
    unsigned long long* dcurve = ws.cnt.as<unsigned long long>();
    LM_HIP(hipMemsetAsync(dcurve, 0, (size_t)bins * 8, e->stream));
    {
        ProfScope ps(e, "seed_hist", (double)nvox * 2.0);
        LM_LAUNCH(seed_hist_kernel, dim3(flat_grid(nvox)), dim3(kAT), 0, e->stream, (const int16_t*)cost, nvox, bins, dcurve);
        LM_K(hipGetLastError());
    }
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, dcurve, (size_t)bins * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* hcurve = ws.h_cnt.as<unsigned long long>();
    long long reached = 0;
    for (int k = 0; k < bins; ++k) {
        curve[k] = (int64_t)hcurve[k];
        reached += (long long)hcurve[k];
    }
    info[0] = rounds, info[1] = reached;
    return LM_OK;
}

int airway_mask(lm_engine* e, const int16_t* cost, const uint8_t* lab, int n, int h, int w, int threshold, uint8_t* mask, int64_t counts[256]) {
    std::memset(counts, 0, sizeof(int64_t) * 256);
    const size_t nvox = (size_t)n * h * w;
    if (nvox == 0) return LM_OK;
    AirwayWorkspace& ws = e->airway;
    LM_TRY(ws.cnt.reserve(kHistMax * 8));
    LM_TRY(ws.h_cnt.reserve(kHistMax * 8));
    unsigned long long* cnt = ws.cnt.as<unsigned long long>();
    LM_HIP(hipMemsetAsync(cnt, 0, 256 * 8, e->stream));
    {
        ProfScope ps(e, "airway_mask", (double)nvox * (lab ? 4.0 : 3.0));
        LM_LAUNCH(airway_mask_kernel, dim3(std::min(flat_grid(nvox), 2048u)), dim3(kAT), 0, e->stream, cost, lab, (unsigned)nvox, threshold, mask, cnt);
        LM_K(hipGetLastError());
    }
    LM_HIP(hipMemcpyAsync(ws.h_cnt.p, cnt, 256 * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* hc = ws.h_cnt.as<unsigned long long>();
    for (int l = 0; l < 256; ++l) counts[l] = (int64_t)hc[l];
    return LM_OK;
}

}  // namespace lm
