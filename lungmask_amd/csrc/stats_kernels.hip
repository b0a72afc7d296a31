// Per-label volume and density statistics (lm_label_stats_dev, include/lungmask_hip.h): one read of the label and intensity volumes,
// a 4096-bin HU histogram per label in LDS, per-label counts / index sums / extremes / boxes in registers.
//
// Layout.  A workgroup (256 threads) owns G labels (the template argument; grid.y = label group, labels 1 + g*G .. 1 + g*G + G - 1)
// and keeps their histograms in LDS as u32 bins (G x 16 KiB).  Each thread takes 16 consecutive voxels of one row per step (a
// "chunk": one 16-byte label load, 16 * sizeof(T) bytes of intensities); a chunk with no voxel of the group's labels skips its
// intensity load.  Per label the thread counts in registers (arrays indexed by the unrolled label slot, never by a runtime label).
// At the end the workgroup writes its histograms and its reduced accumulators to per-workgroup slabs; two small kernels reduce the
// slabs (the histogram rows in a few column splits with u64 atomic adds into a zeroed result, the accumulators in fixed order).
// No per-voxel global atomic, and integer arithmetic throughout: the result does not depend on the schedule.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#include "volume_common.h"

namespace lm {
namespace {

constexpr int kBins = 4096, kLo = -1024, kHi = 3071;  // 1-HU bins, bin = clip(hu, -1024, 3071) + 1024
constexpr int kTPB = 256;
constexpr int kF = 16;      // accumulator fields per (workgroup, label)
constexpr int kHdr = 17 * kF;  // acc header: [16 labels][16 fields] + the `other` row; the u64 histogram follows
// accumulator fields (kF int64 per label)
enum { F_VOX, F_NF, F_CLO, F_CHI, F_MIN, F_MAX, F_SZ, F_SY, F_SX, F_Z0, F_Z1, F_Y0, F_Y1, F_X0, F_X1 };
__host__ __device__ inline int field_op(int f) {  // 0 add, 1 min, 2 max
    return (f == F_MIN || f == F_Z0 || f == F_Y0 || f == F_X0) ? 1 : ((f == F_MAX || f == F_Z1 || f == F_Y1 || f == F_X1) ? 2 : 0);
}
__device__ __forceinline__ long long field_combine(int op, long long a, long long b) {
    return op == 0 ? a + b : (op == 1 ? (a < b ? a : b) : (a > b ? a : b));
}
__host__ __device__ inline long long field_identity(int op) { return op == 0 ? 0 : (op == 1 ? LLONG_MAX : LLONG_MIN); }

struct StatsParams {
    const uint8_t* lab;
    const void* vol;
    int h, w, n_labels, H;  // H = histogram labels = n_labels - 1
    unsigned cpr, nchunks;  // chunks per row, chunks in the volume
    int vec;                // 16-byte loads (w % 16 == 0, both bases 16-byte aligned)
    unsigned* slab;         // [gx][H][4096] u32
    long long* sslab;       // [gx][n_labels][kF]: label rows of the group's labels, row 0 = `other` (group 0)
};

__device__ __forceinline__ long long wave_reduce(long long v, int op) {
    for (int m = 32; m >= 1; m >>= 1) v = field_combine(op, v, __shfl_xor(v, m));
    return v;
}

template <int G, class T>
__global__ __launch_bounds__(kTPB) void label_stats_kernel(StatsParams p) {
    typedef typename HuOf<T>::type HuT;
    __shared__ __attribute__((aligned(16))) unsigned hist[G * kBins];
    const int tid = threadIdx.x;
    const int group = blockIdx.y, base = 1 + group * G;
    for (int i = tid; i < G * kBins; i += kTPB) hist[i] = 0u;
    __syncthreads();
    unsigned cnt[G], nf[G], clo[G], chi[G], other = 0u;
    HuT mn[G], mx[G];
    unsigned long long sz[G], sy[G], sx[G];
    int z0[G], z1[G], y0[G], y1[G], x0[G], x1[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        cnt[j] = nf[j] = clo[j] = chi[j] = 0u;
        mn[j] = sizeof(HuT) == 8 ? (HuT)LLONG_MAX : (HuT)INT_MAX;
        mx[j] = sizeof(HuT) == 8 ? (HuT)LLONG_MIN : (HuT)INT_MIN;
        sz[j] = sy[j] = sx[j] = 0ull;
        z0[j] = y0[j] = x0[j] = INT_MAX;
        z1[j] = y1[j] = x1[j] = -1;
    }
    const int nl = p.n_labels;
    constexpr int NV = 16 * (int)sizeof(T) / 16;  // 16-byte loads of one chunk's intensities
    for (unsigned c = blockIdx.x * kTPB + tid; c < p.nchunks; c += gridDim.x * kTPB) {
        const unsigned row = c / p.cpr;
        const int xb = (int)(c - row * p.cpr) * 16;
        const int z = (int)(row / (unsigned)p.h), y = (int)(row - (unsigned)z * p.h);
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
            for (int i = 0; i < 16; ++i) l[i] = i < nx ? p.lab[off + i] : (uint8_t)0;  // (label 0: counted by nobody here)
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            any |= (unsigned)(l[i] - base) < (unsigned)G;
            if (group == 0) other += l[i] >= nl ? 1u : 0u;
        }
        if (!any) continue;
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
        unsigned cc[G], si[G];
        int lo[G], hi[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            cc[j] = si[j] = 0u;
            lo[j] = 16;
            hi[j] = -1;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            bool nan;
            const HuT hu = to_hu<T>(v[i], nan);
            const int d = (int)l[i] - base;
            const int bin = (int)(hu < (HuT)kLo ? (HuT)kLo : (hu > (HuT)kHi ? (HuT)kHi : hu)) - kLo;
            if ((unsigned)d < (unsigned)G && !nan) atomicAdd(&hist[d * kBins + bin], 1u);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const bool e = d == j, ef = e && !nan;
                cc[j] += e ? 1u : 0u;
                si[j] += e ? (unsigned)i : 0u;
                lo[j] = min(lo[j], e ? i : 16);
                hi[j] = e ? i : hi[j];
                nf[j] += (e && nan) ? 1u : 0u;
                clo[j] += (ef && hu < (HuT)kLo) ? 1u : 0u;
                chi[j] += (ef && hu > (HuT)kHi) ? 1u : 0u;
                mn[j] = ef && hu < mn[j] ? hu : mn[j];
                mx[j] = ef && hu > mx[j] ? hu : mx[j];
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
            if (cc[j] == 0u) continue;
            cnt[j] += cc[j];
            sz[j] += (unsigned long long)z * cc[j];
            sy[j] += (unsigned long long)y * cc[j];
            sx[j] += (unsigned long long)xb * cc[j] + si[j];
            z0[j] = min(z0[j], z);
            z1[j] = max(z1[j], z);
            y0[j] = min(y0[j], y);
            y1[j] = max(y1[j], y);
            x0[j] = min(x0[j], xb + lo[j]);
            x1[j] = max(x1[j], xb + hi[j]);
        }
    }
    __syncthreads();
    // histograms -> this workgroup's slab rows (16-byte stores)
    const int bx = blockIdx.x;
    for (int i = tid; i < G * kBins / 4; i += kTPB) {
        const int j = i / (kBins / 4);
        if (base + j < nl) {
            const uint4 q = reinterpret_cast<const uint4*>(hist)[i];
            reinterpret_cast<uint4*>(p.slab + ((size_t)bx * p.H + (base - 1 + j)) * kBins)[i - j * (kBins / 4)] = q;
        }
    }
    __syncthreads();
    // accumulators: wave reduction, then the four waves' rows through LDS (the histogram's space), one slab row per label
    long long* red = reinterpret_cast<long long*>(hist);  // [4 waves][G + 1][kF]
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j <= G; ++j) {
        long long f[kF];
#pragma unroll
        for (int k = 0; k < kF; ++k) f[k] = field_identity(field_op(k));
        if (j < G) {
            f[F_VOX] = cnt[j];
            f[F_NF] = nf[j];
            f[F_CLO] = clo[j];
            f[F_CHI] = chi[j];
            f[F_MIN] = (long long)mn[j];
            f[F_MAX] = (long long)mx[j];
            f[F_SZ] = (long long)sz[j];
            f[F_SY] = (long long)sy[j];
            f[F_SX] = (long long)sx[j];
            f[F_Z0] = z0[j];
            f[F_Z1] = z1[j];
            f[F_Y0] = y0[j];
            f[F_Y1] = y1[j];
            f[F_X0] = x0[j];
            f[F_X1] = x1[j];
        } else {
            f[F_VOX] = other;
        }
#pragma unroll
        for (int k = 0; k < kF; ++k) f[k] = wave_reduce(f[k], field_op(k));
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kF; ++k) red[(wave * (G + 1) + j) * kF + k] = f[k];
        }
    }
    __syncthreads();
    if (tid < (G + 1) * kF) {
        const int j = tid / kF, k = tid - j * kF, op = field_op(k);
        long long a = red[j * kF + k];
        for (int wv = 1; wv < kTPB / 64; ++wv) a = field_combine(op, a, red[(wv * (G + 1) + j) * kF + k]);
        const int label = j < G ? base + j : 0;  // row 0: `other` (group 0 only)
        if (label < nl && (j < G || group == 0)) p.sslab[((size_t)bx * nl + label) * kF + k] = a;
    }
}

// hist[r][b] (u64, zeroed) += sum over the workgroups bx = split, split + S, ... of slab[bx][r][b]
__global__ __launch_bounds__(kTPB) void label_stats_reduce_hist_kernel(const unsigned* __restrict__ slab, unsigned long long* hist, int gx,
                                                                       int H) {
    const int idx = blockIdx.x * kTPB + threadIdx.x;  // r * 4096 + b
    if (idx >= H * kBins) return;
    const int S = gridDim.y;
    unsigned long long s = 0;
    for (int bx = blockIdx.y; bx < gx; bx += S) s += slab[(size_t)bx * H * kBins + idx];
    if (s) atomicAdd(&hist[idx], s);
}

// acc[label][k] = the fields of the workgroups' rows combined in workgroup order (one workgroup per label)
__global__ __launch_bounds__(kTPB) void label_stats_reduce_acc_kernel(const long long* __restrict__ sslab, long long* acc, int gx, int nl) {
    __shared__ long long part[kTPB];
    const int label = blockIdx.x, k = threadIdx.x % kF, part_id = threadIdx.x / kF, op = field_op(k);
    long long a = field_identity(op);
    for (int bx = part_id; bx < gx; bx += kTPB / kF) a = field_combine(op, a, sslab[((size_t)bx * nl + label) * kF + k]);
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x < kF) {
        for (int q = 1; q < kTPB / kF; ++q) a = field_combine(op, a, part[q * kF + k]);
        acc[label * kF + k] = a;
    }
}

template <int G, class T>
hipError_t launch_main(const StatsParams& p, int gx, int groups, hipStream_t s) {
    LM_LAUNCH((label_stats_kernel<G, T>), dim3(gx, groups), dim3(kTPB), 0, s, p);
    return hipGetLastError();
}

template <int G>
hipError_t launch_dtype(const StatsParams& p, int dtype, int gx, int groups, hipStream_t s) {
    switch (dtype) {
        case LM_I16: return launch_main<G, int16_t>(p, gx, groups, s);
        case LM_I32: return launch_main<G, int32_t>(p, gx, groups, s);
        case LM_I64: return launch_main<G, int64_t>(p, gx, groups, s);
        case LM_F32: return launch_main<G, float>(p, gx, groups, s);
        default: return launch_main<G, double>(p, gx, groups, s);
    }
}

}  // namespace

int label_stats(lm_engine* e, const uint8_t* lab, const void* vol, int dtype, int n, int h, int w, int n_labels, lm_label_stats* stats,
                int64_t* hist_out, int64_t* other_out) {
    const int H = n_labels - 1;
    // G labels per workgroup: as few passes over the volume as possible with at most 4 histograms (64 KiB of LDS) per workgroup, and
    // the passes evenly filled (5 histogram labels: 3 + 2, not 4 + 1).  Workgroups per CU as the LDS allows (at most 8 x 4 waves).
    const int groups = H <= 0 ? 1 : (H + 3) / 4;
    const int G = H <= 0 ? 1 : (H + groups - 1) / groups;
    static const int per_cu[5] = {0, 8, 4, 3, 2};
    const int esz = dtype_bytes(dtype);
    const unsigned cpr = (unsigned)(w + 15) / 16;
    const unsigned nchunks = (unsigned)((size_t)n * h * cpr);
    int cus = 0;
    LM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
    long long gx = ((long long)std::max(cus, 1) * per_cu[G] + groups - 1) / groups;
    gx = std::max(1LL, std::min(gx, ((long long)nchunks + kTPB - 1) / kTPB));
    StatsWorkspace& ws = e->stats;
    const size_t acc_words = kHdr + (size_t)std::max(H, 0) * kBins;
    LM_TRY(ws.acc.reserve(acc_words * 8));
    LM_TRY(ws.h_acc.reserve(acc_words * 8));
    LM_TRY(ws.slab.reserve((size_t)gx * std::max(H, 1) * kBins * 4 + (size_t)gx * n_labels * kF * 8 + 16));
    long long* acc = ws.acc.as<long long>();
    unsigned* slab = ws.slab.as<unsigned>();
    long long* sslab = reinterpret_cast<long long*>(slab + (size_t)gx * std::max(H, 1) * kBins);
    const bool vec = w % 16 == 0 && (reinterpret_cast<uintptr_t>(lab) & 15) == 0 && (reinterpret_cast<uintptr_t>(vol) & 15) == 0;
    if (n > 0) {
        StatsParams p{lab, vol, h, w, n_labels, H, cpr, nchunks, vec ? 1 : 0, slab, sslab};
        {
            ProfScope ps(e, "label_stats", (double)n * h * w * (1.0 + esz));
            hipError_t err = hipSuccess;
            switch (G) {
                case 1: err = launch_dtype<1>(p, dtype, (int)gx, groups, e->stream); break;
                case 2: err = launch_dtype<2>(p, dtype, (int)gx, groups, e->stream); break;
                case 3: err = launch_dtype<3>(p, dtype, (int)gx, groups, e->stream); break;
                default: err = launch_dtype<4>(p, dtype, (int)gx, groups, e->stream); break;
            }
            LM_K(err);
        }
        ProfScope ps(e, "label_stats_reduce", (double)gx * (std::max(H, 0) * kBins * 4.0 + n_labels * kF * 8.0));
        if (H > 0) {
            LM_HIP(hipMemsetAsync(acc + kHdr, 0, (size_t)H * kBins * 8, e->stream));
            const int splits = (int)std::min<long long>(gx, 128);
            LM_LAUNCH(label_stats_reduce_hist_kernel, dim3((H * kBins + kTPB - 1) / kTPB, splits), dim3(kTPB), 0, e->stream, slab,
                      reinterpret_cast<unsigned long long*>(acc + kHdr), (int)gx, H);
            LM_K(hipGetLastError());
        }
        LM_LAUNCH(label_stats_reduce_acc_kernel, dim3(n_labels), dim3(kTPB), 0, e->stream, sslab, acc, (int)gx, n_labels);
        LM_K(hipGetLastError());
        const size_t words = hist_out ? acc_words : kHdr;
        LM_HIP(hipMemcpyAsync(ws.h_acc.p, acc, words * 8, hipMemcpyDeviceToHost, e->stream));
        LM_HIP(hipStreamSynchronize(e->stream));
    }
    const long long* a = ws.h_acc.as<long long>();
    long long labelled = 0;
    for (int k = 0; k < n_labels; ++k) {
        lm_label_stats& s = stats[k];
        std::memset(&s, 0, sizeof s);
        for (int q = 0; q < 6; ++q) s.bbox[q] = -1;
        if (k == 0 || n == 0) continue;
        const long long* f = a + k * kF;
        s.voxels = f[F_VOX];
        labelled += s.voxels;
        if (s.voxels == 0) continue;
        s.nonfinite = f[F_NF];
        s.clipped_low = f[F_CLO];
        s.clipped_high = f[F_CHI];
        if (s.voxels > s.nonfinite) {
            s.hu_min = f[F_MIN];
            s.hu_max = f[F_MAX];
        }
        s.index_sum[0] = f[F_SZ];
        s.index_sum[1] = f[F_SY];
        s.index_sum[2] = f[F_SX];
        const int b[6] = {(int)f[F_Z0], (int)f[F_Z1] + 1, (int)f[F_Y0], (int)f[F_Y1] + 1, (int)f[F_X0], (int)f[F_X1] + 1};
        for (int q = 0; q < 6; ++q) s.bbox[q] = b[q];
    }
    const long long other = n > 0 ? a[F_VOX] : 0;  // row 0 of the accumulators: the voxels with a label >= n_labels
    stats[0].voxels = (long long)n * h * w - labelled - other;
    if (other_out) *other_out = other;
    if (hist_out) {
        std::memset(hist_out, 0, (size_t)n_labels * kBins * 8);
        if (n > 0) std::memcpy(hist_out + kBins, a + kHdr, (size_t)std::max(H, 0) * kBins * 8);
    }
    return LM_OK;
}

}  // namespace lm
