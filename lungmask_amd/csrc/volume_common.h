// What the analysis kernels on label / intensity volumes share (stats_, texture_, metrics_, mesh_, morph_, component_, filter_,
// vessel_, skeleton_kernels.hip, and through sample_common.h roi_, resample_, register_, deform_kernels.hip): the label table
// passed by value, the HU value and the floating value of a voxel, the box of a selection, and the pieces of the exact distance
// transform that lm_edt_dev and lm_nearest_label_dev have in common.  One definition each; compiles under hipcc and under the g++
// emulation (lm_platform.h).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "engine.h"

namespace lm {

// ------------------------------------------------------------------------------------------------ label table
struct LabelTable {
    unsigned w[8];  // bit l of the table: table[l] != 0
};

// a 256-entry table in LDS (one thread per entry; the words are picked with constant indices: the argument stays in registers)
__device__ __forceinline__ void stage_table(const LabelTable& tb, uint8_t* table, int tid) {
    if (tid < 256) {
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) word = (tid >> 5) == k ? tb.w[k] : word;
        table[tid] = (uint8_t)((word >> (tid & 31)) & 1u);
    }
}

inline LabelTable label_table(const uint8_t table[256]) {
    LabelTable tb;
    for (int k = 0; k < 8; ++k) tb.w[k] = 0u;
    for (int l = 0; l < 256; ++l)
        if (table[l]) tb.w[l >> 5] |= 1u << (l & 31);
    return tb;
}

// ------------------------------------------------------------------------------------------------ HU value of a voxel
// THE definition for statistics, texture, components, filters and the LAA map: integers as they are; floats rint (half to even)
// saturated to int32, NaN flagged.
//   to_hu<T>   for kernels templated on the volume's type.  An int64 value is returned as it is, as long long (HuOf): the
//              statistics and the texture codes compare and accumulate the unsaturated value.
//   load_hu    for kernels that take the dtype at run time; always int, so int64 volumes are SATURATED to int32 here.
template <class T> struct HuOf { typedef int type; };
template <> struct HuOf<int64_t> { typedef long long type; };

template <class T> __device__ __forceinline__ typename HuOf<T>::type to_hu(T v, bool& nan) {
    nan = false;
    return v;
}
template <> __device__ __forceinline__ int to_hu<float>(float v, bool& nan) {
    nan = v != v;
    const float r = rintf(v);
    return nan ? 0 : (r >= 2147483648.0f ? INT_MAX : (r < -2147483648.0f ? INT_MIN : (int)r));
}
template <> __device__ __forceinline__ int to_hu<double>(double v, bool& nan) {
    nan = v != v;
    const double r = rint(v);
    return nan ? 0 : (r >= 2147483648.0 ? INT_MAX : (r < -2147483648.0 ? INT_MIN : (int)r));
}

__device__ __forceinline__ int load_hu(const void* vol, int dtype, size_t v, bool& nan) {
    switch (dtype) {
        case LM_I16: return to_hu(static_cast<const int16_t*>(vol)[v], nan);
        case LM_I32: return to_hu(static_cast<const int32_t*>(vol)[v], nan);
        case LM_I64: {
            const long long q = to_hu(static_cast<const int64_t*>(vol)[v], nan);
            return q > (long long)INT_MAX ? INT_MAX : (q < (long long)INT_MIN ? INT_MIN : (int)q);
        }
        case LM_F32: return to_hu(static_cast<const float*>(vol)[v], nan);
        default: return to_hu(static_cast<const double*>(vol)[v], nan);
    }
}

// the value of voxel v of a volume of a run-time `dtype` (LM_I16 .. LM_F64) as F = float or double
template <class F>
__device__ __forceinline__ F load_as(const void* vol, int dtype, size_t v) {
    switch (dtype) {
        case LM_I16: return (F)static_cast<const int16_t*>(vol)[v];
        case LM_I32: return (F)static_cast<const int32_t*>(vol)[v];
        case LM_I64: return (F)static_cast<const long long*>(vol)[v];
        case LM_F32: return (F)static_cast<const float*>(vol)[v];
        default: return (F)static_cast<const double*>(vol)[v];
    }
}

// bytes of one element of a volume of `dtype` (LM_I16 .. LM_F64)
inline int dtype_bytes(int dtype) { return dtype == LM_I16 ? 2 : ((dtype == LM_I32 || dtype == LM_F32) ? 4 : 8); }

// Host side: f(TypeTag<T>()) for the element type T of a volume of a run-time `dtype` (LM_I16 .. LM_F64, checked by the caller; U8:
// LM_U8 as well).  f is a generic lambda that launches the kernel instantiated for T: `typename decltype(tag)::type`.
template <class T> struct TypeTag { typedef T type; };

template <bool U8 = false, class F>
auto with_image_type(int dtype, F&& f) {
    if constexpr (U8)
        if (dtype == LM_U8) return f(TypeTag<uint8_t>());
    switch (dtype) {
        case LM_I16: return f(TypeTag<int16_t>());
        case LM_I32: return f(TypeTag<int32_t>());
        case LM_I64: return f(TypeTag<int64_t>());
        case LM_F32: return f(TypeTag<float>());
        default: return f(TypeTag<double>());
    }
}

// ------------------------------------------------------------------------------------------------ box of a selection
struct VolBox {
    int z0, y0, x0, n, h, w;  // origin in the volume, extent
};

// bbox = {z0, z1, y0, y1, x0, x1} grown by margin[i] voxels on either side of axis i, clipped to the volume.  A margin may be +inf
// (the whole axis): it is compared before it is cast.
inline VolBox grown_box(const int32_t bbox[6], const double margin[3], const int dims[3]) {
    int lo[3], hi[3];
    for (int i = 0; i < 3; ++i) {
        const double m = margin[i];
        lo[i] = m >= (double)bbox[2 * i] ? 0 : bbox[2 * i] - (int)m;
        hi[i] = m >= (double)(dims[i] - bbox[2 * i + 1]) ? dims[i] : bbox[2 * i + 1] + (int)m;
    }
    return VolBox{lo[0], lo[1], lo[2], hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
}

// ------------------------------------------------------------------------------------------------ distance transform
constexpr int kMaxDim = 4096;  // dx^2 <= 2^24 stays exact in float32; one row = at most 64 ballot words

inline void edt_weights(const double* spacing, float wgt[3]) {
    for (int i = 0; i < 3; ++i) {
        const double s = spacing ? spacing[i] : 1.0;
        wgt[i] = (float)(s * s);
    }
}

// The x pass of both transforms: bit x' of words[x' >> 6] = voxel x' of the row is a feature.  xl = position of the nearest
// feature at or before x, xr = of the nearest one after x; -1 for none.  Integer work only.
__device__ __forceinline__ void nearest_set_bits(const unsigned long long* words, int nwords, int x, int& xl, int& xr) {
    const int wi = x >> 6, bi = x & 63;
    xl = xr = -1;
    unsigned long long m = words[wi] & (~0ull >> (63 - bi));
    for (int j = wi; j >= 0; --j) {
        if (j != wi) m = words[j];
        if (m) {
            xl = j * 64 + 63 - __clzll((long long)m);
            break;
        }
    }
    m = bi == 63 ? 0ull : words[wi] & (~0ull << (bi + 1));
    for (int j = wi; j < nwords; ++j) {
        if (j != wi) m = words[j];
        if (m) {
            xr = j * 64 + __ffsll((long long)m) - 1;
            break;
        }
    }
}

// Launch geometry of a y (axis 1) or z (axis 0) line pass over the box: lines of L voxels, n_outer slabs of them, element
// (o, l, x) at o * so + l * sl + x; a workgroup's tile = TX consecutive x of one o with all L values of l in tile_cells cells of
// LDS.  L == 1: the pass is skipped (the only candidate is the voxel itself).
struct LinePass {
    int L, TX, n_outer;
    size_t so, sl;
    long long tiles;
};

inline LinePass line_pass_plan(const VolBox& b, int axis, int tile_cells) {
    LinePass p;
    p.L = axis == 1 ? b.h : b.n;
    p.TX = std::min(b.w, tile_cells / p.L);
    if (p.TX >= 32) p.TX &= ~31;
    p.n_outer = axis == 1 ? b.n : b.h;
    const size_t plane = (size_t)b.h * b.w;
    p.so = axis == 1 ? plane : (size_t)b.w;
    p.sl = axis == 1 ? (size_t)b.w : plane;
    p.tiles = (long long)p.n_outer * ((b.w + p.TX - 1) / p.TX);
    return p;
}

}  // namespace lm
