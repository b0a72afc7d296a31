// Paired-CT analysis (lm_pair_map_dev; include/lungmask_hip.h): per fixed voxel the fixed HU, the moving HU through the transform,
// the Jacobian of the transform and the label give the class of the parametric response map, the mass-corrected density change and
// the local volume change, and a per-label table of their integer sums -- one streaming pass over the fixed grid in place of
// lm_warp_dev, lm_jacobian_dev, two downloads and the per-lobe arithmetic on the host.  The arithmetic is the header's: float64
// without contraction in the order written, one rounding to float32 per output; the coordinate, the inside test, the clamp and the
// taps are lm_resample_dev's, from sample_common.h; every sum across threads is an integer sum, so no result depends on the schedule.
// This file also holds the extern "C" entry point with its argument checks (the limits are lm_demons_step_dev's).
//
// The determinant is lm_jacobian_dev's, RESTATED here (field_det) from df_jacobian_kernel in deform_kernels.hip expression by
// expression, not shared through a header: moving that kernel's body would change the file whose instantiations and registers
// tests/test_deform_resources.py pins.  tests/test_pair_emu.py holds the two to the same bits.
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

// lm_jacobian_dev's determinant at voxel p = (o[0], o[1], o[2]) of a field [3][N] on a grid of extents e: df_jacobian_kernel's
// expressions (deform_kernels.hip), restated
__device__ __forceinline__ double field_det(const float* __restrict__ field, size_t N, unsigned p, const int o[3], const int e[3],
                                            const size_t stride[3], const double fs[3]) {
    double a[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float* __restrict__ ui = field + (size_t)i * N;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool up = o[j] + 1 < e[j], down = o[j] > 0;
            double G = 0.0;  // (an axis of extent 1)
            if (up && down) G = (((double)ui[(size_t)p + stride[j]] - (double)ui[(size_t)p - stride[j]]) * fs[i]) * 0.5;
            else if (up) G = ((double)ui[(size_t)p + stride[j]] - (double)ui[p]) * fs[i];
            else if (down) G = ((double)ui[p] - (double)ui[(size_t)p - stride[j]]) * fs[i];
            a[i][j] = (i == j ? 1.0 : 0.0) + G;
        }
    }
    return (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
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
            if (u) {  // 3. the coordinate rule
                p0 = p0 + (double)u[p] * m.fs[0];
                p1 = p1 + (double)u[N + p] * m.fs[1];
                p2 = p2 + (double)u[2 * N + p] * m.fs[2];
            }
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
    hipError_t err;
    switch (mdtype) {
        case LM_I16: err = launch_pair<int16_t>(m, blocks, fixed, lab, mov, u, cls, chg, jac, table, e->stream); break;
        case LM_I32: err = launch_pair<int32_t>(m, blocks, fixed, lab, mov, u, cls, chg, jac, table, e->stream); break;
        case LM_I64: err = launch_pair<int64_t>(m, blocks, fixed, lab, mov, u, cls, chg, jac, table, e->stream); break;
        case LM_F32: err = launch_pair<float>(m, blocks, fixed, lab, mov, u, cls, chg, jac, table, e->stream); break;
        default: err = launch_pair<double>(m, blocks, fixed, lab, mov, u, cls, chg, jac, table, e->stream);
    }
    LM_K(err);
    return LM_OK;
}

bool pm_finite(double v) { return v == v && v < 1e300 && v > -1e300; }

bool pm_dtype_ok(int dt) { return dt == LM_I16 || dt == LM_I32 || dt == LM_I64 || dt == LM_F32 || dt == LM_F64; }

struct PmRange {
    const char* lo;
    size_t bytes;
};

bool pm_overlap(const PmRange& a, const PmRange& b) {
    return a.lo && b.lo && a.bytes && b.bytes && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes;
}

}  // namespace
}  // namespace lm

extern "C" int lm_pair_map_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* lab_dev,
                               const void* moving_dev, int mdtype, int mn, int mh, int mw, const float* field_dev, const lm_pair_params* p,
                               uint8_t* class_out_dev, float* change_out_dev, float* jac_out_dev, int64_t* table_out_dev) {
    using namespace lm;
    if (!e) return LM_ERR_INVALID;
    const int dims[6] = {fn, fh, fw, mn, mh, mw};
    for (int i = 0; i < 6; ++i)
        if (dims[i] < 1 || dims[i] > 4096) {
            set_error("lm_pair_map_dev: every dimension of the %s volume must lie in 1 .. 4096 (got %d)", i < 3 ? "fixed" : "moving", dims[i]);
            return LM_ERR_INVALID;
        }
    if ((unsigned long long)fn * fh * fw >= 0x7fffffffull || (unsigned long long)mn * mh * mw >= 0x7fffffffull) {
        set_error("lm_pair_map_dev: volume too large (n * h * w must stay below 2^31)");
        return LM_ERR_INVALID;
    }
    if (!p || !fixed_dev || !lab_dev || !moving_dev || !table_out_dev) {
        set_error("lm_pair_map_dev: bad arguments (fixed_dev, lab_dev, moving_dev, params and table_out_dev not NULL; field_dev and the three "
                  "maps may be)");
        return LM_ERR_INVALID;
    }
    if (!pm_dtype_ok(fdtype) || !pm_dtype_ok(mdtype)) {
        set_error("lm_pair_map_dev: dtype must be LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 (got %d, %d)", fdtype, mdtype);
        return LM_ERR_INVALID;
    }
    if (p->n_labels < 1 || p->n_labels > 16) {
        set_error("lm_pair_map_dev: n_labels must lie in 1 .. 16 (got %d)", p->n_labels);
        return LM_ERR_INVALID;
    }
    bool finite = pm_finite(p->jac_scale) && pm_finite(p->air) && pm_finite(p->fixed_thr) && pm_finite(p->moving_thr) && pm_finite(p->lo) &&
                  pm_finite(p->hi);
    for (int i = 0; i < 9; ++i) finite = finite && pm_finite(p->A[i]);
    for (int i = 0; i < 3; ++i) finite = finite && pm_finite(p->b[i]) && pm_finite(p->field_scale[i]);
    if (!finite || !(p->jac_scale > 0.0) || !(p->lo <= p->hi)) {
        set_error("lm_pair_map_dev: A, b, field_scale, air, the thresholds, lo and hi must be finite, jac_scale finite and > 0, lo <= hi");
        return LM_ERR_INVALID;
    }
    const size_t N = (size_t)fn * fh * fw, M = (size_t)mn * mh * mw;
    const PmRange in[4] = {{(const char*)fixed_dev, N * dtype_bytes(fdtype)}, {(const char*)lab_dev, N}, {(const char*)moving_dev, M * dtype_bytes(mdtype)},
                           {(const char*)field_dev, 12 * N}};
    const PmRange out[4] = {{(const char*)class_out_dev, N}, {(const char*)change_out_dev, 4 * N}, {(const char*)jac_out_dev, 4 * N},
                            {(const char*)table_out_dev, (size_t)p->n_labels * LM_PAIR_COLS * 8}};
    for (int a = 0; a < 4; ++a) {
        for (int b = 0; b < 4; ++b)
            if (pm_overlap(out[a], in[b])) {
                set_error("lm_pair_map_dev: an output must not overlap an input (the call is not in-place)");
                return LM_ERR_INVALID;
            }
        for (int b = a + 1; b < 4; ++b)
            if (pm_overlap(out[a], out[b])) {
                set_error("lm_pair_map_dev: the outputs must not overlap one another");
                return LM_ERR_INVALID;
            }
    }
    LM_HIP(hipSetDevice(e->device));
    return pair_map(e, fixed_dev, fdtype, fn, fh, fw, lab_dev, moving_dev, mdtype, mn, mh, mw, field_dev, *p, class_out_dev, change_out_dev,
                    jac_out_dev, table_out_dev);
}
