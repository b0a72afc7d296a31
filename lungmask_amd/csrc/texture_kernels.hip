// Per-label texture matrices (lm_texture_dev, include/lungmask_hip.h): the 3-D grey-level co-occurrence matrix (GLCM) and the 3-D
// grey-level run-length matrix (GLRLM) of every label over the 13 directions, as integer counts.
//
// Layout.  Three kernels.
//   1. texture_code_kernel reads the label and intensity volumes once (16 voxels per thread and step like label_stats_kernel; a
//      chunk without a counted label skips its intensity load) and writes one u16 code per voxel: 0 for a voxel that takes no part
//      (label 0 or >= n_labels, NaN, hu outside [lo, hi]), else 0x8000 | label << 6 | grey level.  Two voxels belong to one run iff
//      their codes are equal and non-zero; they form a pair iff both are non-zero and differ in the level bits only.  The per-label
//      counts (voxels, nonfinite, below, above) are taken here, in LDS, one u64 atomic add per counter and workgroup at the end.
//   2. texture_kernel: grid.y = direction x label group.  A workgroup (256 threads) keeps, for each of its G labels, the Ng x Ng
//      GLCM and the first RC = min(nr, 16) columns of the Ng x nr GLRLM of ONE direction in LDS as u32 (G is chosen so that this
//      stays within 64 KiB).  It walks the code volume one voxel per thread and step.  A voxel of the group adds its pair to the
//      GLCM; when its predecessor along the direction does not continue its run it walks the run forward and records it once.
//      Columns >= RC are rare (long runs) and go to the u64 result with a global atomic add; runs longer than RC also raise
//      longest_run with a global atomic max.  At the end the workgroup stores its LDS matrices to its slab.
//   3. texture_reduce_kernel sums the slabs in workgroup order into the u64 result.
// No per-voxel global atomic for the GLCM, integer counting throughout: the result does not depend on the schedule.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kTPB = 256;
constexpr int kDirs = 13;
constexpr int kRunColsLds = 16;     // GLRLM columns kept in LDS
constexpr int kLdsBytes = 64 * 1024;
constexpr int kCnt = 4;             // counters per label: voxels, nonfinite, below, above
constexpr int kHdr = 16 * kCnt + 16;  // result header (u64 words): [16 labels][kCnt] + longest_run[16]; the GLRLM, then the GLCM follow
enum { C_VOX, C_NF, C_BELOW, C_ABOVE };

struct CodeParams {
    const uint8_t* lab;
    const void* vol;
    int w, n_labels;
    unsigned cpr, nchunks;  // chunks per row, chunks in the volume
    int vec;                // 16-byte loads (w % 16 == 0, both bases 16-byte aligned)
    long long lo, hi;
    unsigned bin_width;
    uint16_t* code;
    unsigned long long* counts;  // [16][kCnt], zeroed
};

template <class T>
__global__ __launch_bounds__(kTPB) void texture_code_kernel(CodeParams p) {
    __shared__ unsigned cnt[16 * kCnt];
    const int tid = threadIdx.x;
    if (tid < 16 * kCnt) cnt[tid] = 0u;
    __syncthreads();
    const int nl = p.n_labels;
    constexpr int NV = 16 * (int)sizeof(T) / 16;  // 16-byte loads of one chunk's intensities
    for (unsigned c = blockIdx.x * kTPB + tid; c < p.nchunks; c += gridDim.x * kTPB) {
        const unsigned row = c / p.cpr;
        const int xb = (int)(c - row * p.cpr) * 16;
        const size_t off = (size_t)row * p.w + xb;
        const int nx = p.w - xb < 16 ? p.w - xb : 16;  // voxels of this chunk inside the row
        uint8_t l[16];
        if (p.vec) {
            const uint4 q = *reinterpret_cast<const uint4*>(p.lab + off);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned wd = i == 0 ? q.x : (i == 1 ? q.y : (i == 2 ? q.z : q.w));
                l[4 * i] = (uint8_t)wd;
                l[4 * i + 1] = (uint8_t)(wd >> 8);
                l[4 * i + 2] = (uint8_t)(wd >> 16);
                l[4 * i + 3] = (uint8_t)(wd >> 24);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) l[i] = i < nx ? p.lab[off + i] : (uint8_t)0;
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            l[i] = l[i] < nl ? l[i] : (uint8_t)0;  // labels >= n_labels take no part, like label 0
            any |= l[i] != 0;
        }
        uint16_t code[16];
        if (any) {
            T v[16];
            if (p.vec) {
                const uint4* src = reinterpret_cast<const uint4*>(static_cast<const T*>(p.vol) + off);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const uint4 q = src[k];
                    __builtin_memcpy(&v[k * 16 / (int)sizeof(T)], &q, 16);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = i < nx ? static_cast<const T*>(p.vol)[off + i] : (T)0;
            }
            int cur = 0;  // the voxels of one label in a row of the chunk are counted with one LDS add
            unsigned run = 0u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                bool nan;
                const long long hu = (long long)to_hu<T>(v[i], nan);
                const int lb = l[i];
                if (lb != cur) {
                    if (cur) atomicAdd(&cnt[cur * kCnt + C_VOX], run);
                    cur = lb;
                    run = 0u;
                }
                ++run;
                const bool below = !nan && hu < p.lo, above = !nan && hu > p.hi;
                if (lb && (nan || below || above)) atomicAdd(&cnt[lb * kCnt + (nan ? C_NF : (below ? C_BELOW : C_ABOVE))], 1u);
                // 0 <= hu - lo <= hi - lo < 2^32 for a valid voxel: the division is exact in 32 bits
                const unsigned g = (unsigned)(hu - p.lo) / p.bin_width;
                code[i] = (lb && !nan && !below && !above) ? (uint16_t)(0x8000u | ((unsigned)lb << 6) | g) : (uint16_t)0;
            }
            if (cur) atomicAdd(&cnt[cur * kCnt + C_VOX], run);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) code[i] = 0;
        }
        if (p.vec) {
            uint4 q[2];
            __builtin_memcpy(q, code, 32);
            reinterpret_cast<uint4*>(p.code + off)[0] = q[0];
            reinterpret_cast<uint4*>(p.code + off)[1] = q[1];
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < nx) p.code[off + i] = code[i];
        }
    }
    __syncthreads();
    if (tid < 16 * kCnt && cnt[tid]) atomicAdd(&p.counts[tid], (unsigned long long)cnt[tid]);
}

struct TexParams {
    const uint16_t* code;
    int n, h, w;
    unsigned nvox;
    int ng, rc, nr, distance;
    int G, S;        // labels per workgroup; u32 words per label in LDS = ng * (ng + rc)
    int n_labels;
    unsigned* slab;  // [13 * groups][gx][G * S] u32
    unsigned long long* glrlm;    // [n_labels - 1][13][ng][nr] u64, zeroed: the columns >= rc
    unsigned long long* longest;  // [16], zeroed: the longest run > rc of every label
};

__global__ __launch_bounds__(kTPB) void texture_kernel(TexParams p) {
    LM_DYN_SMEM(smem);
    unsigned* mat = reinterpret_cast<unsigned*>(smem);  // [G][ng * ng | ng * rc]
    const int tid = threadIdx.x;
    const int d = (int)(blockIdx.y % kDirs), group = (int)(blockIdx.y / kDirs), base = 1 + group * p.G;
    const int M = p.G * p.S;
    for (int i = tid; i < M; i += kTPB) mat[i] = 0u;
    __syncthreads();
    // direction d = the (d + 14)-th offset of {-1, 0, 1}^3 in lexicographic order (the 13 behind the centre)
    const int t = d + 14;
    const int dz = t / 9 - 1, dy = (t / 3) % 3 - 1, dx = t % 3 - 1;
    const int delta = (dz * p.h + dy) * p.w + dx;
    const int ng = p.ng, rc = p.rc, dist = p.distance;
    const unsigned hw = (unsigned)p.h * (unsigned)p.w;
    for (unsigned v = blockIdx.x * kTPB + tid; v < p.nvox; v += gridDim.x * kTPB) {
        const unsigned c = p.code[v];
        if (!c) continue;
        const int ls = (int)((c >> 6) & 15u) - base;
        if ((unsigned)ls >= (unsigned)p.G) continue;
        const int z = (int)(v / hw);
        const unsigned rem = v - (unsigned)z * hw;
        const int y = (int)(rem / (unsigned)p.w), x = (int)(rem - (unsigned)y * p.w);
        const unsigned g = c & 63u;
        unsigned* m = mat + ls * p.S;
        // the next voxel along the direction: the run's continuation, and the pair's partner at distance 1
        int nz = z + dz, ny = y + dy, nx = x + dx;
        bool in = (unsigned)nz < (unsigned)p.n && (unsigned)ny < (unsigned)p.h && (unsigned)nx < (unsigned)p.w;
        const unsigned cn = in ? p.code[(int)v + delta] : 0u;
        unsigned cq = cn;
        if (dist != 1) {
            const int qz = z + dist * dz, qy = y + dist * dy, qx = x + dist * dx;
            const bool qin = (unsigned)qz < (unsigned)p.n && (unsigned)qy < (unsigned)p.h && (unsigned)qx < (unsigned)p.w;
            cq = qin ? p.code[(int)v + dist * delta] : 0u;
        }
        if (cq && (c ^ cq) < 64u) atomicAdd(&m[g * ng + (cq & 63u)], 1u);
        const int pz = z - dz, py = y - dy, px = x - dx;
        const bool pin = (unsigned)pz < (unsigned)p.n && (unsigned)py < (unsigned)p.h && (unsigned)px < (unsigned)p.w;
        if (pin && p.code[(int)v - delta] == c) continue;  // inside a run: its first voxel records it
        int r = 1;
        if (cn == c) {
            int idx = (int)v + delta;
            for (;;) {
                ++r;
                nz += dz, ny += dy, nx += dx, idx += delta;
                in = (unsigned)nz < (unsigned)p.n && (unsigned)ny < (unsigned)p.h && (unsigned)nx < (unsigned)p.w;
                if (!in || p.code[idx] != c) break;
            }
        }
        const int col = (r < p.nr ? r : p.nr) - 1;
        if (col < rc) {
            atomicAdd(&m[ng * ng + g * rc + col], 1u);
        } else {
            const int label = base + ls;
            atomicAdd(&p.glrlm[(((size_t)(label - 1) * kDirs + d) * ng + g) * p.nr + col], 1ull);
        }
        if (r > rc) atomicMax(&p.longest[base + ls], (unsigned long long)r);
    }
    __syncthreads();
    unsigned* out = p.slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * M;
    for (int i = tid; i < M; i += kTPB) out[i] = mat[i];
}

// glcm[label - 1][d][i][j] = and glrlm[label - 1][d][i][col < rc] += the sum over the workgroups bx of slab[by][bx][...], in order
__global__ __launch_bounds__(kTPB) void texture_reduce_kernel(const unsigned* __restrict__ slab, unsigned long long* glcm,
                                                              unsigned long long* glrlm, int gx, int G, int S, int ng, int rc, int nr,
                                                              int n_labels) {
    const int idx = blockIdx.x * kTPB + threadIdx.x, M = G * S;
    if (idx >= M) return;
    const int d = (int)(blockIdx.y % kDirs), group = (int)(blockIdx.y / kDirs);
    const int ls = idx / S, rem = idx - ls * S, label = 1 + group * G + ls;
    if (label >= n_labels) return;
    const unsigned* src = slab + (size_t)blockIdx.y * gx * M + idx;
    unsigned long long s = 0;
    for (int bx = 0; bx < gx; ++bx) s += src[(size_t)bx * M];
    const size_t ld = (size_t)(label - 1) * kDirs + d;
    if (rem < ng * ng) {
        glcm[ld * ng * ng + rem] = s;
    } else {
        const int rr = rem - ng * ng, i = rr / rc, col = rr - i * rc;
        glrlm[(ld * ng + i) * nr + col] += s;
    }
}

template <class T>
hipError_t launch_code(const CodeParams& p, int gx, hipStream_t s) {
    LM_LAUNCH((texture_code_kernel<T>), dim3(gx), dim3(kTPB), 0, s, p);
    return hipGetLastError();
}

}  // namespace

int texture(lm_engine* e, const uint8_t* lab, const void* vol, int dtype, int n, int h, int w, int n_labels, const lm_texture_params& tp,
            lm_texture_counts* counts, int64_t* glcm_out, int64_t* glrlm_out) {
    const int H = n_labels - 1;
    const int ng = (int)(((long long)tp.hi - tp.lo) / tp.bin_width + 1);
    // without glrlm_out the run columns are needed for longest_run only: the LDS columns and the atomic max give it
    const int nr = glrlm_out ? tp.nr : std::min(tp.nr, kRunColsLds);
    const int rc = std::min(nr, kRunColsLds);
    const size_t glcm_words = (size_t)H * kDirs * ng * ng, glrlm_words = (size_t)H * kDirs * ng * nr;
    // label 0 has all-zero rows; without a voxel or a counted label so has every label
    const bool none = n == 0 || H == 0;
    std::memset(counts, 0, sizeof(lm_texture_counts) * n_labels);
    std::memset(glcm_out, 0, (size_t)(none ? n_labels : 1) * kDirs * ng * ng * 8);
    if (glrlm_out) std::memset(glrlm_out, 0, (size_t)(none ? n_labels : 1) * kDirs * ng * nr * 8);
    if (none) return LM_OK;
    // G labels per workgroup: as few passes over the codes as possible within 64 KiB of LDS, the passes evenly filled
    const int S = ng * (ng + rc);
    const int gmax = std::max(1, kLdsBytes / (S * 4));
    const int groups = (H + gmax - 1) / gmax, G = (H + groups - 1) / groups;
    const int M = G * S;
    const int esz = dtype_bytes(dtype);
    const unsigned nvox = (unsigned)((size_t)n * h * w);
    const unsigned cpr = (unsigned)(w + 15) / 16;
    const unsigned nchunks = (unsigned)((size_t)n * h * cpr);
    int cus = 0;
    LM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    cus = std::max(cus, 1);
    const long long gx_code = std::max(1LL, std::min((long long)cus * 8, ((long long)nchunks + kTPB - 1) / kTPB));
    // workgroups per CU as the LDS allows (160 KiB, at most 8 x 4 waves), spread over the directions and label groups
    const int per_cu = std::max(1, std::min(8, 160 * 1024 / (M * 4)));
    long long gx = ((long long)cus * per_cu + kDirs * groups - 1) / (kDirs * groups);
    gx = std::max(1LL, std::min(gx, ((long long)nvox + 4 * kTPB - 1) / (4 * kTPB)));
    TextureWorkspace& ws = e->texture;
    LM_TRY(ws.code.reserve((size_t)nvox * 2 + 32));
    LM_TRY(ws.slab.reserve((size_t)kDirs * groups * gx * M * 4));
    LM_TRY(ws.acc.reserve((kHdr + glrlm_words + glcm_words) * 8));
    LM_TRY(ws.h_acc.reserve((kHdr + (glrlm_out ? 0 : glrlm_words)) * 8));
    unsigned long long* acc = ws.acc.as<unsigned long long>();
    unsigned long long *d_glrlm = acc + kHdr, *d_glcm = acc + kHdr + glrlm_words;
    const bool vec = w % 16 == 0 && (reinterpret_cast<uintptr_t>(lab) & 15) == 0 && (reinterpret_cast<uintptr_t>(vol) & 15) == 0;
    {
        ProfScope ps(e, "texture", (double)n * h * w * (1.0 + esz + 2.0 + 2.0 * kDirs * groups));
        LM_HIP(hipMemsetAsync(acc, 0, (kHdr + glrlm_words) * 8, e->stream));
        CodeParams cp{lab, vol, w, n_labels, cpr, nchunks, vec ? 1 : 0, (long long)tp.lo, (long long)tp.hi, (unsigned)tp.bin_width,
                      ws.code.as<uint16_t>(), acc};
        hipError_t err = hipSuccess;
        switch (dtype) {
            case LM_I16: err = launch_code<int16_t>(cp, (int)gx_code, e->stream); break;
            case LM_I32: err = launch_code<int32_t>(cp, (int)gx_code, e->stream); break;
            case LM_I64: err = launch_code<int64_t>(cp, (int)gx_code, e->stream); break;
            case LM_F32: err = launch_code<float>(cp, (int)gx_code, e->stream); break;
            default: err = launch_code<double>(cp, (int)gx_code, e->stream); break;
        }
        LM_K(err);
        TexParams p{ws.code.as<uint16_t>(), n, h, w, nvox, ng, rc, nr, tp.distance, G, S, n_labels, ws.slab.as<unsigned>(), d_glrlm,
                    acc + 16 * kCnt};
        LM_LAUNCH(texture_kernel, dim3((unsigned)gx, (unsigned)(kDirs * groups)), dim3(kTPB), (size_t)M * 4, e->stream, p);
        LM_K(hipGetLastError());
    }
    {
        ProfScope ps(e, "texture_reduce", (double)kDirs * groups * gx * M * 4.0);
        LM_LAUNCH(texture_reduce_kernel, dim3((M + kTPB - 1) / kTPB, kDirs * groups), dim3(kTPB), 0, e->stream, ws.slab.as<unsigned>(),
                  d_glcm, d_glrlm, (int)gx, G, S, ng, rc, nr, n_labels);
        LM_K(hipGetLastError());
    }
    int64_t* hdr = ws.h_acc.as<int64_t>();
    int64_t* runs = glrlm_out ? glrlm_out + (size_t)kDirs * ng * nr : hdr + kHdr;  // rows of labels 1 .. on the host
    LM_HIP(hipMemcpyAsync(hdr, acc, kHdr * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipMemcpyAsync(runs, d_glrlm, glrlm_words * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipMemcpyAsync(glcm_out + (size_t)kDirs * ng * ng, d_glcm, glcm_words * 8, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    for (int k = 1; k < n_labels; ++k) {
        lm_texture_counts& c = counts[k];
        const int64_t* f = hdr + k * kCnt;
        c.voxels = f[C_VOX];
        c.nonfinite = f[C_NF];
        c.below = f[C_BELOW];
        c.above = f[C_ABOVE];
        c.valid = c.voxels - c.nonfinite - c.below - c.above;
        long long longest = hdr[16 * kCnt + k];  // runs longer than rc; the shorter ones from the LDS columns
        const int64_t* m = runs + (size_t)(k - 1) * kDirs * ng * nr;
        for (int row = 0; row < kDirs * ng; ++row)
            for (int col = rc - 1; col >= longest; --col)
                if (m[(size_t)row * nr + col]) longest = col + 1;
        c.longest_run = longest;
    }
    return LM_OK;
}

}  // namespace lm
