// The joint intensity histogram of a fixed and a moving volume under an affine map (lm_joint_hist_dev; include/lungmask_hip.h): the
// cost function of a mutual-information registration, evaluated hundreds to thousands of times per pair, so neither volume ever
// moves and no resampled volume is written.  The arithmetic is the header's: float64 without contraction for the coordinate and the
// trilinear value (lm_resample_dev's affine_coord and trilinear, sample_common.h), integers from the weights on, so the result does
// not depend on the schedule.
//
// jh_kernel<T, MODE> (T: the moving volume's element, MODE: LM_JH_*; the fixed volume's dtype is read at run time -- one load per
// sample): one thread per lattice point, x fastest, a workgroup of kJH = 256 threads walking a contiguous run of kJH * per_thread
// lattice points.  The eight trilinear corners, their indices and the three fractions stay in registers (no scratch).
//
// The histogram of a workgroup lives in LDS and is flushed once, as int64, into the workgroup's row of a partial table
// [blocks][bins^2 + 4]; jh_reduce_kernel sums the rows into hist_out and counts_out.  Integer sums: any order gives the same bits, and
// both outputs are fully written without zeroing.
//   Overflow.  The LDS counters are 64 bits wide (ds_add_u64): a weight is at most 2^16 and a volume has fewer than 2^31 voxels, so no
//   counter passes 2^47 and no bound on the samples per flush is needed.  The constant (41, 41, 41) case of the tests puts 68 921
//   samples of weight 65 536 -- more than 2^32 -- into one bin of one workgroup.
//   Contention.  ONE copy per workgroup, 64 x 64 x 8 bytes = 32 KiB whatever `bins` is, so four workgroups share a CU.  A CT pair puts
//   most of a wave's samples into a few bins (air with air), and equal addresses of one LDS atomic serialise: at worst 64 adds for q0
//   and 64 for q1 per wave-sample, against the eight dependent gathers and the float64 arithmetic of the same sample.  The add of
//   q1 == 0 is skipped (integer data with width 1, and every LM_JH_NEAREST sample, take one add).  Per-wave copies would not remove
//   the in-wave serialisation, which is the larger part, and would quadruple the flush.
//   LDS per workgroup: 32768 (histogram) + 32 (four counters) + 256 (label table) = 33056 bytes.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kJH = 256;            // threads of a workgroup
constexpr int kJHMaxBins = 64;
constexpr int kJHMaxBlocks = 1024;  // four workgroups per CU
constexpr int kJHPerThread = 8;     // lattice points per thread before the grid grows
constexpr int kJHRE = 8;            // reduce: entries per workgroup (64 contiguous bytes of every row)
constexpr int kJHRS = 32;           // reduce: slices the rows are dealt to
constexpr long long kQ = 65536;

struct JhMap {
    double A[9], b[3];
    int fe1, fe2;         // fixed extents h, w
    int me0, me1, me2;    // moving extents
    int start[3], step[3];
    unsigned K1, K2;      // lattice points along y and x
    unsigned total;       // lattice points
    unsigned per_block;   // lattice points per workgroup
    int bins, fdtype;
    long long f_lo, f_hi, f_width, m_lo, m_hi, m_width;  // hi = lo + bins * width - 1
    LabelTable keep;
};

// The HU value of the statistics (volume_common.h), always int: u8 as it is, int64 saturated.
template <class T>
__device__ __forceinline__ int jh_hu(T v, bool& nan) {
    const long long q = to_hu(v, nan);
    return q > (long long)INT_MAX ? INT_MAX : (q < (long long)INT_MIN ? INT_MIN : (int)q);
}

__device__ __forceinline__ int jh_fixed_hu(const void* vol, int dtype, size_t v, bool& nan) {
    if (dtype == LM_U8) {
        nan = false;
        return static_cast<const uint8_t*>(vol)[v];
    }
    return load_hu(vol, dtype, v, nan);
}

__device__ __forceinline__ int jh_bin(int hu, long long lo, long long hi, long long width) {
    long long c = hu;
    c = c < lo ? lo : (c > hi ? hi : c);
    return (int)((c - lo) / width);
}

template <class T, int MODE>
__global__ __launch_bounds__(kJH) void jh_kernel(JhMap m, const void* __restrict__ fixed, const uint8_t* __restrict__ flab,
                                                const T* __restrict__ mov, unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long hist[kJHMaxBins * kJHMaxBins];
    __shared__ unsigned long long cnt[4];
    __shared__ uint8_t table[256];
    const int tid = threadIdx.x;
    const int nb = m.bins * m.bins;
    for (int k = tid; k < nb; k += kJH) hist[k] = 0ull;
    if (tid < 4) cnt[tid] = 0ull;
    stage_table(m.keep, table, tid);
    __syncthreads();

    unsigned c_all = 0, c_in = 0, c_out = 0, c_nan = 0;
    const unsigned first = blockIdx.x * m.per_block;
    const unsigned last = min(m.total, first + m.per_block);  // (first < 2^31 + 2^18: no wrap)
    for (unsigned p = first + (unsigned)tid; p < last; p += (unsigned)kJH) {
        const unsigned row = p / m.K2;
        const int o2 = m.start[2] + (int)(p - row * m.K2) * m.step[2];
        const unsigned sl = row / m.K1;
        const int o1 = m.start[1] + (int)(row - sl * m.K1) * m.step[1];
        const int o0 = m.start[0] + (int)sl * m.step[0];
        const size_t fv = ((size_t)o0 * m.fe1 + o1) * m.fe2 + o2;
        if (flab && !table[flab[fv]]) continue;
        ++c_all;
        bool nan;
        const int fhu = jh_fixed_hu(fixed, m.fdtype, fv, nan);
        if (nan) {
            ++c_nan;
            continue;
        }
        const int bi = jh_bin(fhu, m.f_lo, m.f_hi, m.f_width);
        double c[3];
        int j[3];
        if (!affine_coord(m.A, m.b, (double)o0, (double)o1, (double)o2, m.me0, m.me1, m.me2, c, j)) {
            ++c_out;
            continue;
        }
        unsigned long long* __restrict__ hrow = hist + bi * m.bins;
        if (MODE == LM_JH_NEAREST) {
            const int mhu = jh_hu(mov[((size_t)j[0] * m.me1 + j[1]) * m.me2 + j[2]], nan);
            if (nan) {
                ++c_nan;
                continue;
            }
            atomicAdd(hrow + jh_bin(mhu, m.m_lo, m.m_hi, m.m_width), (unsigned long long)kQ);
        } else {
            const double v = trilinear(mov, c, m.me0, m.me1, m.me2);
            if (v != v) {
                ++c_nan;
                continue;
            }
            const double top = (double)(m.bins - 1);
            double u = (v - (double)m.m_lo) / (double)m.m_width;
            u = u > 0.0 ? u : 0.0;
            u = u < top ? u : top;
            const double k0f = floor(u);
            const int k0 = (int)k0f;
            const int k1 = k0 + 1 < m.bins - 1 ? k0 + 1 : m.bins - 1;
            const long long q1 = (long long)floor((u - k0f) * (double)kQ + 0.5);
            atomicAdd(hrow + k0, (unsigned long long)(kQ - q1));
            if (q1 != 0) atomicAdd(hrow + k1, (unsigned long long)q1);
        }
        ++c_in;
    }
    if (c_all) atomicAdd(&cnt[0], (unsigned long long)c_all);
    if (c_in) atomicAdd(&cnt[1], (unsigned long long)c_in);
    if (c_out) atomicAdd(&cnt[2], (unsigned long long)c_out);
    if (c_nan) atomicAdd(&cnt[3], (unsigned long long)c_nan);
    __syncthreads();
    unsigned long long* __restrict__ mine = partial + (size_t)blockIdx.x * (size_t)(nb + 4);
    for (int k = tid; k < nb; k += kJH) mine[k] = hist[k];
    if (tid < 4) mine[nb + tid] = cnt[tid];
}

// hist_out and counts_out = the column sums of the partial table [blocks][entries], entries = bins^2 + 4.  A workgroup takes kJHRE
// consecutive entries (64 contiguous bytes of every row) and deals the rows to kJHRS slices, so that a thread's chain of loads is
// at most 1024 / 32 long; 8 x 32 x 8 = 2048 bytes of LDS.
__global__ __launch_bounds__(kJHRE * kJHRS) void jh_reduce_kernel(const unsigned long long* __restrict__ partial, int blocks, int entries,
                                                                 int64_t* __restrict__ hist_out, int64_t* __restrict__ counts_out) {
    __shared__ unsigned long long part[kJHRE * kJHRS];
    const int col = threadIdx.x % kJHRE, slice = threadIdx.x / kJHRE;
    const int entry = blockIdx.x * kJHRE + col;
    unsigned long long s = 0ull;
    if (entry < entries)
        for (int r = slice; r < blocks; r += kJHRS) s += partial[(size_t)r * entries + entry];
    part[slice * kJHRE + col] = s;
    __syncthreads();
    if (slice == 0 && entry < entries) {
#pragma unroll
        for (int k = 1; k < kJHRS; ++k) s += part[k * kJHRE + col];
        const int nb = entries - 4;
        if (entry < nb) hist_out[entry] = (int64_t)s;
        else counts_out[entry - nb] = (int64_t)s;
    }
}

template <class T>
hipError_t launch_jh(const JhMap& m, int mode, int blocks, const void* fixed, const uint8_t* flab, const void* mov, unsigned long long* partial,
                     hipStream_t s) {
    const dim3 grid(blocks), block(kJH);
    if (mode == LM_JH_LINEAR) LM_LAUNCH((jh_kernel<T, LM_JH_LINEAR>), grid, block, 0, s, m, fixed, flab, static_cast<const T*>(mov), partial);
    else LM_LAUNCH((jh_kernel<T, LM_JH_NEAREST>), grid, block, 0, s, m, fixed, flab, static_cast<const T*>(mov), partial);
    return hipGetLastError();
}

}  // namespace

int joint_hist(lm_engine* e, const void* fixed, int fdtype, int fn, int fh, int fw, const uint8_t* flab, const void* mov, int mdtype, int mn,
               int mh, int mw, const lm_joint_hist_params& p, int64_t* hist_out, int64_t* counts_out) {
    JhMap m;
    for (int i = 0; i < 9; ++i) m.A[i] = p.A[i];
    for (int i = 0; i < 3; ++i) m.b[i] = p.b[i];
    m.fe1 = fh, m.fe2 = fw;
    m.me0 = mn, m.me1 = mh, m.me2 = mw;
    const int fe[3] = {fn, fh, fw};
    unsigned K[3];
    for (int i = 0; i < 3; ++i) {
        m.start[i] = p.start[i], m.step[i] = p.step[i];
        K[i] = p.start[i] < fe[i] ? (unsigned)((fe[i] - p.start[i] + p.step[i] - 1) / p.step[i]) : 0u;
    }
    m.K1 = K[1] ? K[1] : 1u, m.K2 = K[2] ? K[2] : 1u;
    m.total = K[0] * K[1] * K[2];  // (at most the fixed volume's voxels: below 2^31)
    m.bins = p.bins, m.fdtype = fdtype;
    m.f_lo = p.f_lo, m.f_width = p.f_width, m.f_hi = (long long)p.f_lo + (long long)p.bins * p.f_width - 1;
    m.m_lo = p.m_lo, m.m_width = p.m_width, m.m_hi = (long long)p.m_lo + (long long)p.bins * p.m_width - 1;
    m.keep = label_table(p.keep);
    const int blocks = walk_plan(m.total, kJH, kJHPerThread, kJHMaxBlocks, m.per_block);
    const int entries = p.bins * p.bins + 4;
    LM_TRY(e->jhist.partial.reserve((size_t)blocks * entries * sizeof(unsigned long long)));
    unsigned long long* partial = e->jhist.partial.as<unsigned long long>();
    {
        const int fsz = fdtype == LM_U8 ? 1 : dtype_bytes(fdtype);
        ProfScope ps(e, p.mode == LM_JH_LINEAR ? "jh_linear" : "jh_nearest", (double)m.total * (fsz + (flab ? 1 : 0)) + (double)blocks * entries * 8.0);
        LM_K(with_image_type<true>(mdtype, [&](auto tag) {
            return launch_jh<typename decltype(tag)::type>(m, p.mode, blocks, fixed, flab, mov, partial, e->stream);
        }));
    }
    {
        ProfScope ps(e, "jh_reduce", ((double)blocks + 1.0) * entries * 8.0);
        LM_LAUNCH(jh_reduce_kernel, dim3((entries + kJHRE - 1) / kJHRE), dim3(kJHRE * kJHRS), 0, e->stream, partial, blocks, entries, hist_out,
                  counts_out);
        LM_K(hipGetLastError());
    }
    return LM_OK;
}

}  // namespace lm
