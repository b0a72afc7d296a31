// Paired-CT analysis (lm_pair_map_dev; include/lungmask_hip.h): per fixed voxel the fixed HU, the moving HU through the transform,
// the Jacobian of the transform and the label give the class of the parametric response map, the mass-corrected density change and
// the local volume change, and a per-label table of their integer sums -- one streaming pass over the fixed grid in place of
// lm_warp_dev, lm_jacobian_dev, two downloads and the per-lobe arithmetic on the host.  The arithmetic is the header's: float64
// without contraction in the order written, one rounding to float32 per output; the coordinate, the inside test, the clamp and the
// taps are lm_resample_dev's, from sample_common.h; every sum across threads is an integer sum, so no result depends on the schedule.
// The determinant is lm_jacobian_dev's and the displaced coordinate lm_warp_dev's: field_det and displace of sample_common.h, the
// one definition df_jacobian_kernel and DfMap (deform_kernels.hip) use.
//
// pm_pair_kernel<T> (T: the moving volume's element; the fixed volume's dtype is read at run time): df_demons_kernel's walk -- a
// workgroup of kPM = 256 threads takes a contiguous share of the voxels (walk_plan) in sweeps of 256, so that a wave reads and writes
// contiguous runs of the labels, the fixed volume, every field component and every output.  A voxel that is not selected costs its
// label byte and the stores.  The table: a thread keeps the thirteen columns of ONE label in registers (ten 32-bit counts, three
// 64-bit sums) and adds them into the workgroup's LDS table only when its label changes and once at the end -- inside a lobe a
// thread's voxels, 256 apart along a row or on the next rows, share a label, so the LDS atomics number a few per thread and lobe
// border, not six per voxel, and lanes of a wave that share a label do not serialise on one LDS address per voxel.  The workgroup
// flushes its table with one 64-bit global atomic per non-zero cell into the output, which the call zeroes first (hipMemsetAsync on
// the same stream).  Column 6 is signed: it is added in two's complement.
//   LDS per workgroup: 1664 (16 x 13 cells of 8 bytes) + 256 (label table) = 1920 bytes.  No scratch.
//   A term of column 5 is at most 2^26, of column 6 at most 2^20 in magnitude, of column 7 at most 2^28; a volume has fewer than 2^31
//   voxels: every sum stays below 2^59.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sample_common.h"

namespace lm {
namespace {

constexpr int kPM = 256;            // threads of a workgroup
constexpr int kPMMaxBlocks = 2048;  // eight workgroups per CU
constexpr int kPMPerThread = 8;     // voxels per thread before the grid grows
constexpr int kPMRows = 16;         // rows of the LDS table (n_labels <= 16)
static_assert(kPMRows * LM_PAIR_COLS <= kPM, "one thread per cell zeroes and flushes the table");

struct PairMap {
    double A[9], b[3], fs[3];
    double jac_scale, air, fthr, mthr, lo, hi;
    int fe0, fe1, fe2;   // fixed extents
    int me0, me1, me2;   // moving extents
    unsigned total;      // fixed voxels
    unsigned per_block;  // voxels per workgroup
    int fdtype, cells;   // cells: n_labels * LM_PAIR_COLS
    LabelTable keep;     // keep[l] != 0 and l < n_labels
};

// the columns of one label, in a thread's registers
struct PairAcc {
    unsigned sel, valid, outside, nan, folded, excluded, code[4];
    long long sj, sc;
    unsigned long long sc2;
};

__device__ __forceinline__ void acc_clear(PairAcc& a) {
    a.sel = a.valid = a.outside = a.nan = a.folded = a.excluded = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.code[k] = 0u;
    a.sj = a.sc = 0ll;
    a.sc2 = 0ull;
}

// adds a thread's columns into row `row` of the LDS table and clears them
__device__ __forceinline__ void acc_flush(PairAcc& a, unsigned long long* row) {
    if (a.sel) atomicAdd(row + 0, (unsigned long long)a.sel);
    if (a.valid) atomicAdd(row + 1, (unsigned long long)a.valid);
    if (a.outside) atomicAdd(row + 2, (unsigned long long)a.outside);
    if (a.nan) atomicAdd(row + 3, (unsigned long long)a.nan);
    if (a.folded) atomicAdd(row + 4, (unsigned long long)a.folded);
    if (a.sj) atomicAdd(row + 5, (unsigned long long)a.sj);
    if (a.sc) atomicAdd(row + 6, (unsigned long long)a.sc);
    if (a.sc2) atomicAdd(row + 7, a.sc2);
    if (a.excluded) atomicAdd(row + 8, (unsigned long long)a.excluded);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (a.code[k]) atomicAdd(row + 9 + k, (unsigned long long)a.code[k]);
    acc_clear(a);
}

template <class T>
__global__ __launch_bounds__(kPM) void pm_pair_kernel(PairMap m, const void* __restrict__ fixed, const uint8_t* __restrict__ lab,
                                                     const T* __restrict__ mov, const float* __restrict__ u, uint8_t* __restrict__ cls_out,
                                                     float* __restrict__ chg_out, float* __restrict__ jac_out,
                                                     unsigned long long* __restrict__ table_out) {
    __shared__ unsigned long long tab[kPMRows * LM_PAIR_COLS];
    __shared__ uint8_t table[256];
    const int tid = threadIdx.x;
    if (tid < kPMRows * LM_PAIR_COLS) tab[tid] = 0ull;
    stage_table(m.keep, table, tid);
    __syncthreads();

    PairAcc acc;
    acc_clear(acc);
    int cur = -1;  // the label whose columns acc holds
    const size_t N = (size_t)m.total;
    const int fe[3] = {m.fe0, m.fe1, m.fe2};
    const size_t stride[3] = {(size_t)m.fe1 * m.fe2, (size_t)m.fe2, (size_t)1};
    const unsigned first = blockIdx.x * m.per_block;
    const unsigned last = min(m.total, first + m.per_block);  // (first < 2^31 + 2^19: no wrap)
    for (unsigned p = first + (unsigned)tid; p < last; p += (unsigned)kPM) {
        const int L = lab[p];
        uint8_t cls = 0;
        float chg = 0.0f, jac = 0.0f;
        if (table[L]) {  // 1. selected
            if (L != cur) {
                if (cur >= 0) acc_flush(acc, tab + cur * LM_PAIR_COLS);
                cur = L;
            }
            ++acc.sel;
            unsigned q0, q1, q2;
            index_split(p, (unsigned)m.fe1, (unsigned)m.fe2, q0, q1, q2);
            const int o[3] = {(int)q0, (int)q1, (int)q2};
            const double f = load_as<double>(fixed, m.fdtype, (size_t)p);  // 2.
            double p0 = (double)o[0], p1 = (double)o[1], p2 = (double)o[2], c[3];
            int j[3];
            displace(u, N, p, m.fs, p0, p1, p2);  // 3. the coordinate rule
            if (f != f) {
                ++acc.nan;
            } else if (!affine_coord(m.A, m.b, p0, p1, p2, m.me0, m.me1, m.me2, c, j)) {
                ++acc.outside;
            } else {
                const double mv = trilinear(mov, c, m.me0, m.me1, m.me2);  // 4.
                const double det = u ? field_det(u, N, p, o, fe, stride, m.fs) : 1.0;
                const double J = m.jac_scale * det;  // 5.
                if (mv != mv || J != J) {
                    ++acc.nan;
                } else if (J <= 0.0) {
                    ++acc.folded;
                    jac = (float)J;
                } else {
                    const double mc = J * (mv - m.air) + m.air;  // 6.
                    const double change = mc - f;
                    if (change != change) {
                        ++acc.nan;
                    } else {
                        ++acc.valid;
                        jac = (float)J;
                        chg = (float)change;
                        const double jc = J < 64.0 ? J : 64.0;
                        acc.sj += (long long)floor(jc * 1048576.0 + 0.5);
                        double cc = change < 65536.0 ? change : 65536.0;
                        cc = cc > -65536.0 ? cc : -65536.0;
                        acc.sc += (long long)floor(cc * 16.0 + 0.5);
                        const double c2 = change * change;
                        const double c2c = c2 < 16777216.0 ? c2 : 16777216.0;
                        acc.sc2 += (unsigned long long)(long long)floor(c2c * 16.0 + 0.5);
                        if (m.lo <= f && f <= m.hi && m.lo <= mv && mv <= m.hi) {  // 7.
                            const int code = (f < m.fthr ? 1 : 0) + (mv < m.mthr ? 2 : 0);
                            cls = (uint8_t)(1 + code);
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc.code[k] += code == k ? 1u : 0u;
                        } else {
                            ++acc.excluded;
                        }
                    }
                }
            }
        }
        if (cls_out) cls_out[p] = cls;
        if (chg_out) chg_out[p] = chg;
        if (jac_out) jac_out[p] = jac;
    }
    if (cur >= 0) acc_flush(acc, tab + cur * LM_PAIR_COLS);
    __syncthreads();
    if (tid < m.cells && tab[tid]) atomicAdd(table_out + tid, tab[tid]);
}

template <class T>
hipError_t launch_pair(const PairMap& m, int blocks, const void* fixed, const uint8_t* lab, const void* mov, const float* u, uint8_t* cls,
                       float* chg, float* jac, unsigned long long* table, hipStream_t s) {
    LM_LAUNCH((pm_pair_kernel<T>), dim3(blocks), dim3(kPM), 0, s, m, fixed, lab, static_cast<const T*>(mov), u, cls, chg, jac, table);
    return hipGetLastError();
}

}  // namespace

int pair_map(lm_engine* e, const void* fixed, int fdtype, int fn, int fh, int fw, const uint8_t* lab, const void* mov, int mdtype, int mn,
             int mh, int mw, const float* u, const lm_pair_params& p, uint8_t* cls, float* chg, float* jac, int64_t* table_out) {
    PairMap m;
    for (int i = 0; i < 9; ++i) m.A[i] = p.A[i];
    for (int i = 0; i < 3; ++i) m.b[i] = p.b[i], m.fs[i] = p.field_scale[i];
    m.jac_scale = p.jac_scale, m.air = p.air, m.fthr = p.fixed_thr, m.mthr = p.moving_thr, m.lo = p.lo, m.hi = p.hi;
    m.fe0 = fn, m.fe1 = fh, m.fe2 = fw;
    m.me0 = mn, m.me1 = mh, m.me2 = mw;
    m.total = (unsigned)((size_t)fn * fh * fw);
    m.fdtype = fdtype;
    m.cells = p.n_labels * LM_PAIR_COLS;
    uint8_t keep[256];
    for (int l = 0; l < 256; ++l) keep[l] = (uint8_t)(p.keep[l] != 0 && l < p.n_labels);
    m.keep = label_table(keep);
    const int blocks = walk_plan(m.total, kPM, kPMPerThread, kPMMaxBlocks, m.per_block);
    unsigned long long* table = reinterpret_cast<unsigned long long*>(table_out);
    LM_K(hipMemsetAsync(table, 0, (size_t)m.cells * sizeof(unsigned long long), e->stream));
    // reads: the labels, the fixed value, the field (its neighbours from cache), the moving corners; writes: the maps asked for
    ProfScope ps(e, "pm_pair", (double)m.total * (1 + dtype_bytes(fdtype) + (u ? 12 : 0) + dtype_bytes(mdtype) + (cls ? 1 : 0) + (chg ? 4 : 0) +
                                                  (jac ? 4 : 0)));
    LM_K(with_image_type(mdtype, [&](auto tag) {
        return launch_pair<typename decltype(tag)::type>(m, blocks, fixed, lab, mov, u, cls, chg, jac, table, e->stream);
    }));
    return LM_OK;
}

}  // namespace lm
