// Surface nets of a label selection (lm_mesh_plan_dev, lm_mesh_dev; include/lungmask_hip.h): one vertex per cell whose eight corner
// voxels are not all equal, one quad per pair of axis neighbours whose selection differs.
//
// All work runs on the box of the selection grown by one cell: C_i = e_i + 1 cells and e_i + 2 voxels per axis (the box's voxels and a
// border of unselected ones on either side, which is what the volume's outside and every voxel beyond the box are).  Local cell
// (kk, jj, ii) is the header's cell (z0 - 1 + kk, y0 - 1 + jj, x0 - 1 + ii); its corner (a, b, c) is the local voxel (kk + a, jj + b,
// ii + c).  The lower voxel of a quad is corner 0 of the cell with the same index, so a cell owns its vertex and the up to three quads
// of its edges 0-4 (z), 0-2 (y), 0-1 (x), and both are numbered by one raster walk over the cells.
//
// mesh_pass_kernel<false> (pass 1, "mesh_count") and <true> (pass 2, "mesh_emit").  A workgroup (256 threads) owns kRows consecutive
// cell rows of one cell slice over their whole width, i.e. one contiguous piece of the raster order.  It first turns the 2 x (kRows + 1)
// voxel rows it needs into bit rows in LDS: a lane loads one label, the wave's ballot is 64 voxels of keep[label] (edt_x's form), so
// a voxel is fetched once per workgroup instead of once per corner; the rows it shares with the workgroups above and below (1 / kRows
// of them, and the second slice) come from L2.  A cell's 8-bit corner mask is then eight bits picked from four LDS words.  Pass 1 only
// adds up the workgroup's vertices and quads.  mesh_scan_kernel turns the per-workgroup counts into offsets (one workgroup: a serial
// run per thread, a wave-shuffle scan over the threads -- rank_blocks' form; there are cells / (kRows * C_2) entries).  Pass 2
// repeats the classification, scans the (row, 64-cell chunk) counts of the workgroup in LDS, and writes the vertex positions, the
// dense cell -> vertex id map (-1: no vertex) and the quads; a quad's corners are cells with a smaller raster index, whose ids other
// workgroups are still writing, so pass 2 stores the corners' CELL indices and mesh_quad_ids_kernel replaces them through the finished
// map (4 Q gathers).  mesh_smooth_kernel is one Jacobi pass over the vertices: per vertex its cell and corner mask (kept by pass 2
// when smooth > 0), the map entries of the up to six cells across a face whose four voxels are not all equal, their positions.
// Arithmetic is the header's, float32 without contraction.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kMT = 256, kWaves = kMT / 64, kRows = 8, kRowsPerWave = kRows / kWaves;
constexpr int kMaxChunks = (4096 + 2 + 63) / 64;  // 64-voxel words of a bit row: e_2 + 2 <= 4098 voxels
constexpr int kScanT = 256;

struct MeshParams {
    const uint8_t* lab;
    int H, W;                    // rows per slice / voxels per row of the label volume
    int z0, y0, x0, e0, e1, e2;  // the box
    int C0, C1, C2;              // cells: e_i + 1
    int ytiles, chunks;          // workgroups per cell slice; 64-cell chunks of a cell row
    LabelTable kb;
    unsigned* wgcnt;        // [workgroups][2]: vertices, quads
    const unsigned* wgoff;  // [workgroups][2]: exclusive sums of wgcnt
    float* verts;
    int* map;
    unsigned* quads;
    unsigned* vcell;  // smooth > 0: the cell of each vertex ...
    uint8_t* vmask;   // ... and its corner mask
    unsigned vcap, qcap;
};

// the two voxels ii, ii + 1 of a bit row for lane ii & 63 of chunk c (row[chunks + 1] is a zero word)
__device__ __forceinline__ unsigned two_bits(const unsigned long long* row, int c, int lane) {
    const unsigned long long lo = row[c], hi = row[c + 1];
    return lane < 63 ? (unsigned)(lo >> lane) & 3u : (unsigned)(lo >> 63) | ((unsigned)(hi & 1ull) << 1);
}

// corner mask of cell (r, c * 64 + lane) of the tile: bit 4 a + 2 b + c = voxel (kk + a, jj + b, ii + c) is selected
__device__ __forceinline__ unsigned corner_mask(const unsigned long long (*bits)[kRows + 1][kMaxChunks + 1], int r, int c, int lane) {
    return two_bits(bits[0][r], c, lane) | (two_bits(bits[0][r + 1], c, lane) << 2) | (two_bits(bits[1][r], c, lane) << 4) |
           (two_bits(bits[1][r + 1], c, lane) << 6);
}

template <bool EMIT>
__global__ __launch_bounds__(kMT) void mesh_pass_kernel(MeshParams p) {
    __shared__ uint8_t keep[256];
    __shared__ unsigned long long bits[2][kRows + 1][kMaxChunks + 1];
    __shared__ unsigned cnt[2][kRows * kMaxChunks + 1];  // EMIT: exclusive sums over (row, chunk) in raster order
    __shared__ unsigned wtot[2][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = (int)(blockIdx.x / (unsigned)p.ytiles), jb = (int)(blockIdx.x - (unsigned)kk * (unsigned)p.ytiles) * kRows;
    const int rows = min(kRows, p.C1 - jb);
    const int vchunks = p.chunks + 1;  // words written per bit row: voxels 0 .. e2 + 1, then zeros up to the word after the last chunk
    stage_table(p.kb, keep, tid);
    __syncthreads();
    // voxel rows (a, r): local z = kk + a, local y = jb + r, r <= rows; local voxel l is global l - 1 + box start, selected only inside the box
    for (int vr = wave; vr < 2 * (kRows + 1); vr += kWaves) {
        const int a = vr / (kRows + 1), r = vr - a * (kRows + 1);
        const int zl = kk + a, yl = jb + r;
        const bool inside = r <= rows && zl >= 1 && zl <= p.e0 && yl >= 1 && yl <= p.e1;  // (wave-uniform)
        const uint8_t* __restrict__ src = p.lab + ((size_t)(p.z0 + zl - 1) * p.H + (size_t)(p.y0 + yl - 1)) * p.W + (p.x0 - 1);
        for (int c = 0; c < vchunks; ++c) {
            const int xl = c * 64 + lane;
            int f = 0;
            if (inside && xl >= 1 && xl <= p.e2) f = keep[src[xl]];
            const unsigned long long word = __ballot(f);
            if (lane == 0) bits[a][r][c] = word;
        }
    }
    __syncthreads();
    // classification: wave w owns rows w * kRowsPerWave ..., so that (wave, row, chunk, lane) is the raster order
    unsigned nv = 0, nq = 0;
    for (int rr = 0; rr < kRowsPerWave; ++rr) {
        const int r = wave * kRowsPerWave + rr;
        if (r >= rows) break;  // (wave-uniform)
        for (int c = 0; c < p.chunks; ++c) {
            const int ii = c * 64 + lane;
            const unsigned m = ii < p.C2 ? corner_mask(bits, r, c, lane) : 0u;
            const unsigned s = m & 1u;
            const unsigned cv = (unsigned)__popcll(__ballot(m != 0u && m != 0xffu));
            const unsigned cq = (unsigned)(__popcll(__ballot(((m >> 4) & 1u) != s)) + __popcll(__ballot(((m >> 2) & 1u) != s)) +
                                           __popcll(__ballot(((m >> 1) & 1u) != s)));
            if (EMIT) {
                if (lane == 0) {
                    cnt[0][r * p.chunks + c] = cv;
                    cnt[1][r * p.chunks + c] = cq;
                }
            } else {
                nv += cv;
                nq += cq;
            }
        }
    }
    if (!EMIT) {
        if (lane == 0) {
            wtot[0][wave] = nv;
            wtot[1][wave] = nq;
        }
        __syncthreads();
        if (tid < 2) {
            unsigned t = 0;
            for (int k = 0; k < kWaves; ++k) t += wtot[tid][k];
            p.wgcnt[2 * (size_t)blockIdx.x + tid] = t;
        }
        return;
    }
    __syncthreads();
    // exclusive scan of the (row, chunk) counts: wave 0 the vertices, wave 1 the quads, 64 entries per step
    if (wave < 2) {
        const int total = rows * p.chunks;
        unsigned carry = 0;
        for (int b = 0; b < total; b += 64) {
            const int i = b + lane;
            const unsigned v = i < total ? cnt[wave][i] : 0u;
            unsigned incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            if (i < total) cnt[wave][i] = carry + incl - v;
            carry += __shfl(incl, 63);
        }
    }
    __syncthreads();
    const unsigned vbase = p.wgoff[2 * (size_t)blockIdx.x], qbase = p.wgoff[2 * (size_t)blockIdx.x + 1];
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned sY = (unsigned)p.C2, sZ = (unsigned)p.C1 * (unsigned)p.C2;  // (cells < 2^32: every C_i <= 4097, voxels < 2^31)
    for (int rr = 0; rr < kRowsPerWave; ++rr) {
        const int r = wave * kRowsPerWave + rr;
        if (r >= rows) break;
        const int jj = jb + r;
        const unsigned rowcell = ((unsigned)kk * (unsigned)p.C1 + (unsigned)jj) * (unsigned)p.C2;
        for (int c = 0; c < p.chunks; ++c) {
            const int ii = c * 64 + lane;
            const bool valid = ii < p.C2;
            const unsigned m = valid ? corner_mask(bits, r, c, lane) : 0u;
            const unsigned s = m & 1u;
            const bool act = m != 0u && m != 0xffu;
            const bool qz = ((m >> 4) & 1u) != s, qy = ((m >> 2) & 1u) != s, qx = ((m >> 1) & 1u) != s;
            const unsigned long long bv = __ballot(act), bz = __ballot(qz), by = __ballot(qy), bx = __ballot(qx);
            const unsigned cell = rowcell + (unsigned)ii;
            const unsigned vid = vbase + cnt[0][r * p.chunks + c] + (unsigned)__popcll(bv & below);
            if (valid) p.map[cell] = act ? (int)vid : -1;
            if (act && vid < p.vcap) {
                const unsigned dx = (m ^ (m >> 1)) & 0x55u, dy = (m ^ (m >> 2)) & 0x33u, dz = (m ^ (m >> 4)) & 0x0fu;
                const int nx = __popc(dx), ny = __popc(dy), nz = __popc(dz);
                const float den = (float)(2 * (nx + ny + nz));
                const int s2z = nz + 2 * (__popc(dx & 0x50u) + __popc(dy & 0x30u));
                const int s2y = ny + 2 * (__popc(dx & 0x44u) + __popc(dz & 0x0cu));
                const int s2x = nx + 2 * (__popc(dy & 0x22u) + __popc(dz & 0x0au));
                float* v = p.verts + 3 * (size_t)vid;
                v[0] = (float)(p.z0 - 1 + kk) + (float)s2z / den;
                v[1] = (float)(p.y0 - 1 + jj) + (float)s2y / den;
                v[2] = (float)(p.x0 - 1 + ii) + (float)s2x / den;
                if (p.vcell) {
                    p.vcell[vid] = cell;
                    p.vmask[vid] = (uint8_t)m;
                }
            }
            // quads in z, y, x order; first corner the smallest cell, then round the edge so that the right-hand normal (components
            // in z, y, x order) points from the selected voxel to the unselected one
            unsigned q = qbase + cnt[1][r * p.chunks + c] + (unsigned)(__popcll(bz & below) + __popcll(by & below) + __popcll(bx & below));
            if (qz) {
                if (q < p.qcap) {  // the cells around a z edge: (jj - 1, ii - 1), (jj, ii - 1), (jj, ii), (jj - 1, ii)
                    unsigned* o = p.quads + 4 * (size_t)q;
                    o[0] = cell - sY - 1u;
                    o[1] = s ? cell - 1u : cell - sY;
                    o[2] = cell;
                    o[3] = s ? cell - sY : cell - 1u;
                }
                ++q;
            }
            if (qy) {
                if (q < p.qcap) {  // a y edge: (kk - 1, ii - 1), (kk - 1, ii), (kk, ii), (kk, ii - 1)
                    unsigned* o = p.quads + 4 * (size_t)q;
                    o[0] = cell - sZ - 1u;
                    o[1] = s ? cell - sZ : cell - 1u;
                    o[2] = cell;
                    o[3] = s ? cell - 1u : cell - sZ;
                }
                ++q;
            }
            if (qx && q < p.qcap) {  // an x edge: (kk - 1, jj - 1), (kk, jj - 1), (kk, jj), (kk - 1, jj)
                unsigned* o = p.quads + 4 * (size_t)q;
                o[0] = cell - sZ - sY;
                o[1] = s ? cell - sY : cell - sZ;
                o[2] = cell;
                o[3] = s ? cell - sZ : cell - sY;
            }
        }
    }
}

// off[i] = sum of cnt[j], j < i, for both columns of cnt [n][2]; totals (64-bit) to tot[0..1].  One workgroup.
__global__ __launch_bounds__(kScanT) void mesh_scan_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ off, unsigned n,
                                                           unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long wsum[2][kScanT / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned per = (n + kScanT - 1u) / kScanT;
    const unsigned lo = min(tid * per, n), hi = min(lo + per, n);
    unsigned long long s[2] = {0ull, 0ull};
    for (unsigned i = lo; i < hi; ++i) {
        s[0] += cnt[2 * (size_t)i];
        s[1] += cnt[2 * (size_t)i + 1];
    }
    unsigned long long excl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        unsigned long long incl = s[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d);
            if (lane >= (unsigned)d) incl += up;
        }
        excl[k] = incl - s[k];
        if (lane == 63u) wsum[k][wave] = incl;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        unsigned long long all = 0ull;
        for (unsigned v = 0; v < kScanT / 64; ++v) {
            if (v < wave) excl[k] += wsum[k][v];
            all += wsum[k][v];
        }
        if (tid == 0) tot[k] = all;
    }
    unsigned long long a = excl[0], b = excl[1];
    for (unsigned i = lo; i < hi; ++i) {  // (a total beyond 2^31 is refused by the host before these offsets are used)
        off[2 * (size_t)i] = (unsigned)a;
        off[2 * (size_t)i + 1] = (unsigned)b;
        a += cnt[2 * (size_t)i];
        b += cnt[2 * (size_t)i + 1];
    }
}

// quads[i] (a cell index) -> the cell's vertex id
__global__ __launch_bounds__(kMT) void mesh_quad_ids_kernel(unsigned* __restrict__ quads, const int* __restrict__ map, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kMT + threadIdx.x; i < n; i += (size_t)gridDim.x * kMT) quads[i] = (unsigned)map[quads[i]];
}

// one Jacobi pass p' = p + f * (avg - p) over the vertices; neighbours in the order -z, +z, -y, +y, -x, +x
__global__ __launch_bounds__(kMT) void mesh_smooth_kernel(const float* __restrict__ in, float* __restrict__ out, const unsigned* __restrict__ vcell,
                                                         const uint8_t* __restrict__ vmask, const int* __restrict__ map, unsigned nv,
                                                         unsigned sZ, unsigned sY, float f) {
    for (unsigned v = blockIdx.x * kMT + threadIdx.x; v < nv; v += gridDim.x * kMT) {
        const unsigned cell = vcell[v], m = vmask[v];
        // the face towards each neighbour: its four corner bits are not all equal
        const unsigned sel[6] = {0x0fu, 0xf0u, 0x33u, 0xccu, 0x55u, 0xaau};
        const unsigned nb[6] = {cell - sZ, cell + sZ, cell - sY, cell + sY, cell - 1u, cell + 1u};
        float mz = 0.f, my = 0.f, mx = 0.f;
        int count = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const unsigned face = m & sel[k];
            if (face != 0u && face != sel[k]) {
                const float* q = in + 3 * (size_t)map[nb[k]];
                mz = mz + q[0];
                my = my + q[1];
                mx = mx + q[2];
                ++count;
            }
        }
        const float* pv = in + 3 * (size_t)v;
        const float pz = pv[0], py = pv[1], px = pv[2], c = (float)count;
        float* o = out + 3 * (size_t)v;
        o[0] = pz + f * (mz / c - pz);
        o[1] = py + f * (my / c - py);
        o[2] = px + f * (mx / c - px);
    }
}

MeshParams params_of(const MeshWorkspace& ws, const uint8_t* lab, int h, int w) {
    MeshParams p;
    std::memset(&p, 0, sizeof p);
    p.lab = lab;
    p.H = h;
    p.W = w;
    p.z0 = ws.bbox[0], p.y0 = ws.bbox[2], p.x0 = ws.bbox[4];
    p.e0 = ws.bbox[1] - ws.bbox[0], p.e1 = ws.bbox[3] - ws.bbox[2], p.e2 = ws.bbox[5] - ws.bbox[4];
    p.C0 = p.e0 + 1, p.C1 = p.e1 + 1, p.C2 = p.e2 + 1;
    p.ytiles = (p.C1 + kRows - 1) / kRows;
    p.chunks = (p.C2 + 63) / 64;
    p.kb = label_table(ws.keep);
    return p;
}

}  // namespace

int mesh_plan(lm_engine* e, const uint8_t* lab, int n, int h, int w, const uint8_t keep[256], int32_t bbox[6], int64_t* n_vertices,
              int64_t* n_quads) {
    MeshWorkspace& ws = e->mesh;
    ws.planned = false;
    *n_vertices = *n_quads = 0;
    LM_TRY(roi_plan(e, lab, n, h, w, keep, bbox));  // (no kept voxel: LM_ERR_INVALID, "no kept voxel")
    std::memcpy(ws.bbox, bbox, sizeof ws.bbox);
    std::memcpy(ws.keep, keep, 256);
    MeshParams p = params_of(ws, lab, h, w);
    const size_t wgs = (size_t)p.C0 * p.ytiles;  // (<= 4097 * 513)
    LM_TRY(ws.wgcnt.reserve(wgs * 2 * sizeof(unsigned)));
    LM_TRY(ws.wgoff.reserve(wgs * 2 * sizeof(unsigned)));
    LM_TRY(ws.scal.reserve(2 * sizeof(unsigned long long)));
    LM_TRY(ws.h_scal.reserve(2 * sizeof(unsigned long long)));
    p.wgcnt = ws.wgcnt.as<unsigned>();
    const double box_vox = (double)p.e0 * p.e1 * p.e2;
    {
        ProfScope ps(e, "mesh_count", box_vox);
        LM_LAUNCH(mesh_pass_kernel<false>, dim3((unsigned)wgs), dim3(kMT), 0, e->stream, p);
        LM_K(hipGetLastError());
    }
    {
        ProfScope ps(e, "mesh_scan", (double)wgs * 16.0);
        LM_LAUNCH(mesh_scan_kernel, dim3(1), dim3(kScanT), 0, e->stream, ws.wgcnt.as<unsigned>(), ws.wgoff.as<unsigned>(), (unsigned)wgs,
                  ws.scal.as<unsigned long long>());
        LM_K(hipGetLastError());
    }
    LM_K(hipMemcpyAsync(ws.h_scal.p, ws.scal.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    LM_K(hipStreamSynchronize(e->stream));
    const unsigned long long nv = ws.h_scal.as<unsigned long long>()[0], nq = ws.h_scal.as<unsigned long long>()[1];
    if (nv >= 0x7fffffffull || nq >= 0x7fffffffull) {
        set_error("lm_mesh_plan_dev: mesh too large (%llu vertices, %llu quads; both must stay below 2^31)", nv, nq);
        return LM_ERR_INVALID;
    }
    ws.lab = lab;
    ws.n = n, ws.h = h, ws.w = w;
    ws.n_vertices = (long long)nv, ws.n_quads = (long long)nq;
    ws.planned = true;
    *n_vertices = (int64_t)nv;
    *n_quads = (int64_t)nq;
    return LM_OK;
}

int mesh(lm_engine* e, const uint8_t* lab, int n, int h, int w, const uint8_t keep[256], int smooth, float lambda, float mu, float* verts,
         int64_t n_vertices_cap, int32_t* quads, int64_t n_quads_cap) {
    MeshWorkspace& ws = e->mesh;
    if (!(ws.planned && ws.lab == lab && ws.n == n && ws.h == h && ws.w == w && std::memcmp(ws.keep, keep, 256) == 0)) {
        int32_t bbox[6];
        int64_t nv, nq;
        LM_TRY(mesh_plan(e, lab, n, h, w, keep, bbox, &nv, &nq));
    }
    ws.planned = false;  // one plan, one mesh
    const long long nv = ws.n_vertices, nq = ws.n_quads;
    if (n_vertices_cap < nv || n_quads_cap < nq) {  // refused before anything is written
        set_error("lm_mesh_dev: capacity too small (%lld vertices for %lld, %lld quads for %lld)", (long long)n_vertices_cap, nv,
                  (long long)n_quads_cap, nq);
        return LM_ERR_INVALID;
    }
    MeshParams p = params_of(ws, lab, h, w);
    const size_t wgs = (size_t)p.C0 * p.ytiles, cells = (size_t)p.C0 * p.C1 * p.C2;
    LM_TRY(ws.map.reserve(cells * sizeof(int)));
    if (smooth > 0) {
        LM_TRY(ws.vcell.reserve((size_t)nv * sizeof(unsigned)));
        LM_TRY(ws.vmask.reserve((size_t)nv));
        LM_TRY(ws.tmp.reserve((size_t)nv * 3 * sizeof(float)));
        p.vcell = ws.vcell.as<unsigned>();
        p.vmask = ws.vmask.as<uint8_t>();
    }
    p.wgoff = ws.wgoff.as<unsigned>();
    p.verts = verts;
    p.map = ws.map.as<int>();
    p.quads = reinterpret_cast<unsigned*>(quads);
    p.vcap = (unsigned)nv, p.qcap = (unsigned)nq;  // (<= the caller's capacities)
    const double box_vox = (double)p.e0 * p.e1 * p.e2;
    {
        ProfScope ps(e, "mesh_emit", box_vox + (double)cells * 4.0 + (double)nv * (smooth > 0 ? 17.0 : 12.0) + (double)nq * 16.0);
        LM_LAUNCH(mesh_pass_kernel<true>, dim3((unsigned)wgs), dim3(kMT), 0, e->stream, p);
        LM_K(hipGetLastError());
    }
    if (nq > 0) {
        const size_t nidx = (size_t)nq * 4;
        ProfScope ps(e, "mesh_quad_ids", (double)nidx * 12.0);
        LM_LAUNCH(mesh_quad_ids_kernel, dim3((unsigned)std::min<size_t>((nidx + kMT - 1) / kMT, 1u << 16)), dim3(kMT), 0, e->stream, p.quads,
                  ws.map.as<int>(), nidx);
        LM_K(hipGetLastError());
    }
    if (smooth > 0 && nv > 0) {
        const unsigned grid = (unsigned)std::min<size_t>(((size_t)nv + kMT - 1) / kMT, 1u << 16);
        const unsigned sY = (unsigned)p.C2, sZ = (unsigned)p.C1 * (unsigned)p.C2;
        ProfScope ps(e, "mesh_smooth", (double)smooth * 2.0 * (double)nv * (5.0 + 7.0 * 4.0 + 7.0 * 12.0));
        for (int it = 0; it < smooth; ++it) {
            LM_LAUNCH(mesh_smooth_kernel, dim3(grid), dim3(kMT), 0, e->stream, verts, ws.tmp.as<float>(), ws.vcell.as<unsigned>(),
                      ws.vmask.as<uint8_t>(), ws.map.as<int>(), (unsigned)nv, sZ, sY, lambda);
            LM_LAUNCH(mesh_smooth_kernel, dim3(grid), dim3(kMT), 0, e->stream, ws.tmp.as<float>(), verts, ws.vcell.as<unsigned>(),
                      ws.vmask.as<uint8_t>(), ws.map.as<int>(), (unsigned)nv, sZ, sY, mu);
        }
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

}  // namespace lm
