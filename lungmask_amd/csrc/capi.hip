// extern "C" surface of liblungmask_hip.so (include/lungmask_hip.h).
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>

#include "engine.h"
#include "post_kernels.h"
#include "pre_kernels.h"
#include "volume_common.h"

using namespace lm;

// every entry point that launches work first makes the engine's device current (callers such as
// torch.distributed workers may have switched devices on this thread)
#define LM_DEVICE(e) LM_HIP(hipSetDevice((e)->device))

// the dtypes of an intensity volume
static int image_dtype_ok(int dtype) { return dtype == LM_I16 || dtype == LM_I32 || dtype == LM_I64 || dtype == LM_F32 || dtype == LM_F64; }

// n parameters that must be numbers of ordinary size (v may be NULL: not finite)
static int finite_all(const double* v, int n) {
    for (int i = 0; v && i < n; ++i)
        if (!(v[i] == v[i]) || !(v[i] < 1e300 && v[i] > -1e300)) return 0;
    return v != nullptr;
}

// the output grid of the resampling entry points: every extent in 1 .. 4096, 32-bit voxel indices
static int out_dims_ok(const char* who, const int32_t dims[3]) {
    unsigned long long nout = 1;
    for (int i = 0; i < 3; ++i) {
        if (dims[i] < 1 || dims[i] > 4096) {
            set_error("%s: output too large or empty (1 <= out_dims[%d] <= 4096, got %d)", who, i, dims[i]);
            return 0;
        }
        nout *= (unsigned long long)dims[i];
    }
    if (nout >= 0x7fffffffull) {
        set_error("%s: output too large (N_0 * N_1 * N_2 must stay below 2^31)", who);
        return 0;
    }
    return 1;
}

extern "C" {

const char* lm_last_error(void) { return get_error(); }
const char* lm_version(void) { return "lungmask_hip 0.1 (gfx950)"; }
int lm_is_gpu_build(void) { return LM_IS_GPU_BUILD; }

int lm_engine_create(lm_engine** out, int device_id) {
    if (!out) return LM_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    LM_HIP(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) {
        set_error("device %d not present (%d devices)", device_id, n);
        return LM_ERR_INVALID;
    }
    LM_HIP(hipSetDevice(device_id));
    lm_engine* e = new lm_engine();
    e->device = device_id;
    hipError_t err = hipStreamCreate(&e->stream);
    if (err != hipSuccess) {
        set_error("hipStreamCreate failed: %s", hipGetErrorString(err));
        delete e;
        return LM_ERR_DEVICE;
    }
    // The second forward lane must sit on a different hardware queue than the first, or the two batches serialise.
    // Same-priority streams share a small round-robin pool of queues (whether two of them collide depends on how many
    // streams the process created before -- e.g. torch.distributed's -- which cost 15 % in one start-up order); a stream of
    // another priority class always gets a queue of its own.  Lowest priority: the lane fills gaps, it never preempts.
    hipError_t err2;
    {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        err2 = hipStreamCreateWithPriority(&e->stream2, hipStreamDefault, least);
    }
    if (err2 != hipSuccess || hipEventCreate(&e->ev_fork) != hipSuccess || hipEventCreate(&e->ev_join) != hipSuccess) {
        set_error("creating the second forward lane failed");
        e->stream2 = nullptr;
        e->n_streams = 1;
    }
    *out = e;
    return LM_OK;
}

void lm_engine_destroy(lm_engine* e) {
    if (!e) return;
    e->helper.stop();
    (void)lm_dist_destroy(e);
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    e->prof.release();
    for (auto& m : e->models) m.release();
    if (e->stream2) (void)hipStreamSynchronize(e->stream2);
    if (e->zero_page) (void)hipFree(e->zero_page);
    if (e->range_flag_host) (void)hipHostFree(e->range_flag_host);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->tail_ready) (void)hipEventDestroy(e->tail_ready);
    if (e->mid_ready) (void)hipEventDestroy(e->mid_ready);
    if (e->pre_fork) (void)hipEventDestroy(e->pre_fork);
    if (e->pre_tail_done) (void)hipEventDestroy(e->pre_tail_done);
    e->nn.release();
    e->nn2.release();
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    e->post.release();
    e->slab.release();
    e->app.release();
    e->stats.release();
    e->texture.release();
    e->metrics.release();
    e->roi.release();
    e->resample.release();
    e->jhist.release();
    e->morph.release();
    e->comp.release();
    e->filter.release();
    e->lcc.release();
    e->vessel.release();
    e->skel.release();
    e->airway.release();
    e->mesh.release();
    e->pipe.release();
    (void)hipStreamDestroy(e->stream);
    delete e;
}

int lm_engine_sync(lm_engine* e) {
    if (!e) return LM_ERR_INVALID;
    if (e->stream2) LM_HIP(hipStreamSynchronize(e->stream2));
    LM_HIP(hipStreamSynchronize(e->stream));
    return LM_OK;
}

int lm_dev_alloc(lm_engine* e, void** dev_ptr, size_t bytes) {
    if (!e || !dev_ptr) return LM_ERR_INVALID;
    LM_HIP(hipSetDevice(e->device));
    LM_HIP(hipMalloc(dev_ptr, bytes ? bytes : 16));
    return LM_OK;
}
int lm_dev_free(lm_engine* e, void* dev_ptr) {
    if (!e) return LM_ERR_INVALID;
    LM_HIP(hipStreamSynchronize(e->stream));
    LM_HIP(hipFree(dev_ptr));
    return LM_OK;
}
int lm_host_alloc(lm_engine* e, void** host_ptr, size_t bytes) {
    if (!e || !host_ptr) return LM_ERR_INVALID;
    LM_HIP(hipSetDevice(e->device));
    LM_HIP(hipHostMalloc(host_ptr, bytes ? bytes : 16, 0));
    return LM_OK;
}
int lm_host_free(lm_engine* e, void* host_ptr) {
    if (e) LM_HIP(hipStreamSynchronize(e->stream));
    if (host_ptr) LM_HIP(hipHostFree(host_ptr));
    return LM_OK;
}
// whether [p, p + bytes) is page-locked memory the runtime knows (lm_host_alloc, hipHostMalloc, a registered range)
static bool host_range_is_pinned(const void* p, size_t bytes) {
#ifdef LM_EMU_BUILD
    (void)p;
    (void)bytes;
    return false;
#else
    hipPointerAttribute_t a0{}, a1{};
    if (hipPointerGetAttributes(&a0, p) != hipSuccess) {
        (void)hipGetLastError();  // ordinary memory: "invalid value", not an error of ours
        return false;
    }
    if (bytes > 1 && hipPointerGetAttributes(&a1, reinterpret_cast<const char*>(p) + bytes - 1) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a0.type == hipMemoryTypeHost && (bytes <= 1 || a1.type == hipMemoryTypeHost);
#endif
}
int lm_copy_h2d(lm_engine* e, void* dev_dst, const void* host_src, size_t bytes) {
    if (!e) return LM_ERR_INVALID;
    LM_HIP(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    return LM_OK;
}
int lm_copy_d2h(lm_engine* e, void* host_dst, const void* dev_src, size_t bytes) {
    if (!e) return LM_ERR_INVALID;
    LM_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    return LM_OK;
}

int lm_model_load(lm_engine* e, int slot, const lm_tensor* tensors, int n_tensors) {
    if (!e) return LM_ERR_INVALID;
    LM_HIP(hipSetDevice(e->device));
    LM_TRY(model_load(e, slot, tensors, n_tensors));
    return model_probe(e, slot);  // accuracy guard (a split-f16 engine only)
}

int lm_model_probe_error(lm_engine* e, int slot, float* err_out) {
    if (!e || slot < 0 || slot >= 4 || !e->models[slot].loaded || !err_out) return LM_ERR_NOMODEL;
    *err_out = e->models[slot].probe_err;
    return e->models[slot].acc_pinned ? 1 : (e->models[slot].chain_k > 0 ? 2 : 0);
}
void* lm_engine_stream(lm_engine* e) { return e ? reinterpret_cast<void*>(e->stream) : nullptr; }

int lm_model_chain_limit(lm_engine* e, int slot) {
    if (!e || slot < 0 || slot >= 4 || !e->models[slot].loaded) return LM_ERR_NOMODEL;
    return e->models[slot].chain_k;
}

int lm_model_classes(lm_engine* e, int slot) {
    if (!e || slot < 0 || slot >= 4 || !e->models[slot].loaded) return LM_ERR_NOMODEL;
    return e->models[slot].n_classes;
}

int lm_model_precision(lm_engine* e, int slot) {
    if (!e || slot < 0 || slot >= 4 || !e->models[slot].loaded) return LM_ERR_NOMODEL;
    return (e->precision == 1 && !e->models[slot].force_f32) ? 1 : 0;
}

int lm_set_precision(lm_engine* e, int mode) {
    if (!e || (mode != 0 && mode != 1)) {
        set_error("lm_set_precision: mode must be 0 (exact fp32) or 1 (split-f16)");
        return LM_ERR_INVALID;
    }
    e->precision = mode;
    if (mode == 1) {  // models loaded while the engine was on the exact kernels have not met the accuracy guard yet
        LM_DEVICE(e);
        for (int slot = 0; slot < 4; ++slot) LM_TRY(model_probe(e, slot));
    }
    return LM_OK;
}

int lm_set_streams(lm_engine* e, int n) {
    if (!e || n < 1 || n > 2) {
        set_error("lm_set_streams: 1 or 2");
        return LM_ERR_INVALID;
    }
    e->n_streams = (n == 2 && e->stream2) ? 2 : 1;
    return LM_OK;
}

int lm_set_fusion(lm_engine* e, int mask) {
    if (!e || mask < 0 || mask > 15) {
        set_error("lm_set_fusion: mask is a combination of bits 0..3");
        return LM_ERR_INVALID;
    }
    e->fusion = mask;
    return LM_OK;
}

int lm_forward_batches_dev(lm_engine* e, int slot, const float* x_dev, int n, int h, int w, int batch_size, uint8_t* labels_dev) {
    if (!e || !x_dev || !labels_dev || n < 0) return LM_ERR_INVALID;
    LM_DEVICE(e);
    return forward_guarded(e, slot, x_dev, n, h, w, batch_size <= 0 ? 20 : batch_size, labels_dev, nullptr);
}

int lm_forward_dev(lm_engine* e, int slot, const float* x_dev, int b, int h, int w, uint8_t* labels_dev, float* logp_dev) {
    if (!e || !x_dev) return LM_ERR_INVALID;
    LM_DEVICE(e);
    return forward_guarded(e, slot, x_dev, b, h, w, 0, labels_dev, logp_dev);
}

int lm_preprocess_dev(lm_engine* e, const void* vol_dev, int dtype, int n, int h, int w, int oh, int ow, int32_t* bbox_dev,
                      float* x_f32_dev, int16_t* x_i16_dev, uint8_t* bmask_dev) {
    if (!e || !vol_dev || !bbox_dev || n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) {
        set_error("lm_preprocess_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    if (!image_dtype_ok(dtype)) {
        set_error("lm_preprocess_dev: unsupported dtype code %d", dtype);
        return LM_ERR_INVALID;
    }
    if (x_i16_dev && (dtype == LM_F32 || dtype == LM_F64)) {
        set_error("lm_preprocess_dev: the int16 resample output only exists for integer volumes");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    BodyMaskParams bp{vol_dev, dtype, n, h, w, bbox_dev, bmask_dev};
    const double vox = (double)n * h * w;
    const int esz = dtype == LM_I16 ? 2 : ((dtype == LM_I32 || dtype == LM_F32) ? 4 : 8);
    e->prof.begin(e->stream, e->prof.kind_id("bodymask_bbox"), 0, (double)n * 128 * 128 * esz);
    hipError_t err = launch_bodymask_bbox(bp, e->stream);
    e->prof.end(e->stream);
    if (err != hipSuccess) {
        set_error("bodymask launch failed: %s", hipGetErrorString(err));
        return LM_ERR_DEVICE;
    }
    if (x_f32_dev || x_i16_dev) {
        ResampleParams rp{vol_dev, dtype, n, h, w, bbox_dev, oh, ow, x_i16_dev, x_f32_dev};
        e->prof.begin(e->stream, e->prof.kind_id("resample_norm"), 0, vox * esz + (double)n * oh * ow * 4);
        err = launch_resample_norm(rp, e->stream);
        e->prof.end(e->stream);
        if (err != hipSuccess) {
            set_error("resample launch failed: %s", hipGetErrorString(err));
            return LM_ERR_DEVICE;
        }
    }
    return LM_OK;
}

int lm_reshape_mask_dev(lm_engine* e, const uint8_t* mask_dev, const int32_t* bbox_dev, int n, int mh, int mw, int h, int w,
                        uint8_t* out_dev) {
    if (!e || !mask_dev || !bbox_dev || !out_dev || n < 0 || mh <= 0 || mw <= 0 || h <= 0 || w <= 0) {
        set_error("lm_reshape_mask_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    ReshapeParams p{mask_dev, bbox_dev, out_dev, n, mh, mw, h, w};
    e->prof.begin(e->stream, e->prof.kind_id("reshape_mask"), 0, (double)n * ((double)mh * mw + (double)h * w));
    hipError_t err = launch_reshape_mask(p, e->stream);
    e->prof.end(e->stream);
    if (err != hipSuccess) {
        set_error("reshape_mask launch failed: %s", hipGetErrorString(err));
        return LM_ERR_DEVICE;
    }
    return LM_OK;
}

int lm_uncrop_probs_dev(lm_engine* e, const float* logp_dev, const int32_t* bbox_dev, int n, int C, int mh, int mw, int h, int w,
                        int out_dtype, void* out_dev) {
    if (!e || !logp_dev || !bbox_dev || !out_dev || n < 0 || C <= 0 || C > 65535 || mh <= 0 || mw <= 0 || mw > 256 || h <= 0 || w <= 0 ||
        (out_dtype != LM_F32 && out_dtype != LM_F16)) {
        set_error("lm_uncrop_probs_dev: bad arguments (need C >= 1, 1 <= mw <= 256, h, w >= 1, out_dtype LM_F32 or LM_F16)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    UncropParams p{logp_dev, bbox_dev, out_dev, out_dtype, n, C, mh, mw, h, w, n, 0};
    const double osz = out_dtype == LM_F16 ? 2.0 : 4.0;
    e->prof.begin(e->stream, e->prof.kind_id("uncrop_probs"), 0, (double)n * C * ((double)mh * mw * 4.0 + (double)h * w * osz));
    hipError_t err = launch_uncrop_probs(p, e->stream);
    e->prof.end(e->stream);
    if (err != hipSuccess) {
        set_error("uncrop_probs launch failed: %s", hipGetErrorString(err));
        return LM_ERR_DEVICE;
    }
    return LM_OK;
}

int lm_reorient_dev(lm_engine* e, const void* in_dev, void* out_dev, int elem_size, int n0, int n1, int n2, int64_t s0, int64_t s1,
                    int64_t s2, int64_t base) {
    if (!e || !in_dev || !out_dev || n0 < 0 || n1 < 0 || n2 < 0 || base < 0 ||
        (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)) {
        set_error("lm_reorient_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    ReorientParams p{in_dev, out_dev, elem_size, n0, n1, n2, (long long)s0, (long long)s1, (long long)s2, (long long)base};
    e->prof.begin(e->stream, e->prof.kind_id("reorient"), 0, 2.0 * elem_size * (double)n0 * n1 * n2);
    hipError_t err = launch_reorient(p, e->stream);
    e->prof.end(e->stream);
    if (err != hipSuccess) {
        set_error("reorient launch failed: %s", hipGetErrorString(err));
        return LM_ERR_DEVICE;
    }
    return LM_OK;
}

int lm_postprocess_dev(lm_engine* e, uint8_t* lab_dev, int n, int h, int w, const int* spare, int n_spare, int skip_below) {
    if (!e || !lab_dev || n < 0 || h <= 0 || w <= 0 || n_spare < 0) {
        set_error("lm_postprocess_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return postprocess(e, lab_dev, n, h, w, spare, n_spare, skip_below);
}

int lm_bbox3d_dev(lm_engine* e, const uint8_t* mask_dev, int n, int h, int w, int margin, int32_t bbox_out[6]) {
    if (!e || (!mask_dev && n > 0) || !bbox_out || n < 0 || h <= 0 || w <= 0 || margin < 0) {
        set_error("lm_bbox3d_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return bbox3d(e, mask_dev, n, h, w, margin, bbox_out);
}

int lm_keep_largest_dev(lm_engine* e, uint8_t* mask_dev, int n, int h, int w, int64_t* area_out) {
    if (!e || (!mask_dev && n > 0) || n < 0 || h <= 0 || w <= 0) {
        set_error("lm_keep_largest_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    long long a = 0;
    const int rc = keep_largest(e, mask_dev, n, h, w, &a);
    if (area_out) *area_out = (int64_t)a;
    return rc;
}

int lm_label_stats_dev(lm_engine* e, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h, int w, int n_labels,
                       lm_label_stats* stats_host, int64_t* hist_host, int64_t* other_out) {
    if (!e || !stats_host || n_labels < 1 || n_labels > 16 || n < 0 || h <= 0 || w <= 0 || (n > 0 && (!lab_dev || !vol_dev)) ||
        !image_dtype_ok(dtype)) {
        set_error("lm_label_stats_dev: bad arguments (1 <= n_labels <= 16, n >= 0, h, w >= 1, dtype LM_I16 / LM_I32 / LM_I64 / LM_F32 / "
                  "LM_F64)");
        return LM_ERR_INVALID;
    }
    if ((unsigned long long)n * h * w >= 0x7fffffffull) {
        set_error("lm_label_stats_dev: volume too large (n * h * w must stay below 2^31: u32 bins per workgroup, 32-bit voxel indices)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return label_stats(e, lab_dev, vol_dev, dtype, n, h, w, n_labels, stats_host, hist_host, other_out);
}

int lm_texture_dev(lm_engine* e, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h, int w, int n_labels,
                   const lm_texture_params* params, lm_texture_counts* counts_host, int64_t* glcm_host, int64_t* glrlm_host) {
    if (!e || !params || !counts_host || !glcm_host || n_labels < 1 || n_labels > 16 || n < 0 || h <= 0 || w <= 0 ||
        (n > 0 && (!lab_dev || !vol_dev)) || !image_dtype_ok(dtype)) {
        set_error("lm_texture_dev: bad arguments (1 <= n_labels <= 16, n >= 0, h, w >= 1, dtype LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64, "
                  "params, counts and glcm not NULL)");
        return LM_ERR_INVALID;
    }
    if (params->bin_width < 1 || params->hi < params->lo) {
        set_error("lm_texture_dev: bad discretisation (bin_width >= 1 and lo <= hi, got lo %d hi %d bin_width %d)", params->lo, params->hi,
                  params->bin_width);
        return LM_ERR_INVALID;
    }
    const long long ng = ((long long)params->hi - params->lo) / params->bin_width + 1;
    if (ng > 64) {
        set_error("lm_texture_dev: %lld grey levels ((hi - lo) / bin_width + 1 must lie in 1 .. 64)", ng);
        return LM_ERR_INVALID;
    }
    if (params->distance < 1 || params->distance > 8 || params->nr < 1 || params->nr > 8192) {
        set_error("lm_texture_dev: bad arguments (1 <= distance <= 8, 1 <= nr <= 8192, got distance %d nr %d)", params->distance, params->nr);
        return LM_ERR_INVALID;
    }
    if (n > 4096 || h > 4096 || w > 4096 || (unsigned long long)n * h * w >= 0x7fffffffull) {
        set_error("lm_texture_dev: volume too large (every dimension <= 4096 and n * h * w below 2^31)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return lm::texture(e, lab_dev, vol_dev, dtype, n, h, w, n_labels, *params, counts_host, glcm_host, glrlm_host);
}

// the limits both metrics entry points share: dx^2 exact in float32, 32-bit voxel indices
static int metrics_shape_ok(const char* who, int n, int h, int w) {
    if (n < 0 || h <= 0 || w <= 0) {
        set_error("%s: bad arguments (n >= 0, h, w >= 1)", who);
        return 0;
    }
    if (n > 4096 || h > 4096 || w > 4096 || (unsigned long long)n * h * w >= 0x7fffffffull) {
        set_error("%s: volume too large (every dimension <= 4096 and n * h * w below 2^31)", who);
        return 0;
    }
    return 1;
}

static int spacing_ok(const double* spacing) {
    for (int i = 0; spacing && i < 3; ++i)
        if (!(spacing[i] > 0.0) || !(spacing[i] < 1e15)) return 0;
    return 1;
}

int lm_edt_dev(lm_engine* e, const uint8_t* feat_dev, int n, int h, int w, const double* spacing, float* d2_out_dev) {
    if (!e || !metrics_shape_ok("lm_edt_dev", n, h, w)) return LM_ERR_INVALID;
    if ((n > 0 && (!feat_dev || !d2_out_dev)) || !spacing_ok(spacing)) {
        set_error("lm_edt_dev: bad arguments (device pointers, spacing finite and > 0)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return edt(e, feat_dev, n, h, w, spacing, d2_out_dev);
}

int lm_label_agreement_dev(lm_engine* e, const uint8_t* a_dev, const uint8_t* b_dev, int n, int h, int w, int n_labels,
                           const double* spacing, const double* percentiles, int n_percentiles, lm_label_agreement* out_rows) {
    if (!e || !metrics_shape_ok("lm_label_agreement_dev", n, h, w)) return LM_ERR_INVALID;
    bool ok = out_rows && n_labels >= 1 && n_labels <= 16 && n_percentiles >= 0 && n_percentiles <= 8 && (n_percentiles == 0 || percentiles) &&
              (n == 0 || (a_dev && b_dev)) && spacing_ok(spacing);
    for (int i = 0; ok && i < n_percentiles; ++i) ok = percentiles[i] >= 0.0 && percentiles[i] <= 100.0;
    if (!ok) {
        set_error("lm_label_agreement_dev: bad arguments (1 <= n_labels <= 16, at most 8 percentiles in [0, 100], spacing finite and > 0)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return label_agreement(e, a_dev, b_dev, n, h, w, n_labels, spacing, percentiles, n_percentiles, out_rows);
}

int lm_roi_plan_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], int32_t bbox_out[6]) {
    if (!e || !metrics_shape_ok("lm_roi_plan_dev", n, h, w)) return LM_ERR_INVALID;
    if ((n > 0 && !lab_dev) || !keep || !bbox_out) {
        set_error("lm_roi_plan_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return roi_plan(e, lab_dev, n, h, w, keep, bbox_out);
}

int lm_roi_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev, int n, int h, int w, const lm_roi_params* p,
               void* out_image_dev, uint8_t* out_labels_dev) {
    if (!e || !metrics_shape_ok("lm_roi_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || !vol_dev || !lab_dev || !out_image_dev || !out_labels_dev || n < 1 ||
        !image_dtype_ok(dtype)) {
        set_error("lm_roi_dev: bad arguments (device pointers, n >= 1, dtype LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64)");
        return LM_ERR_INVALID;
    }
    const bool window = (p->flags & LM_ROI_WINDOW) != 0;
    if (p->out_dtype != LM_F32 && p->out_dtype != LM_F16 && p->out_dtype != LM_I16) {
        set_error("lm_roi_dev: out_dtype must be LM_F32, LM_F16 or LM_I16");
        return LM_ERR_INVALID;
    }
    if (p->out_dtype == LM_I16 && (dtype == LM_F32 || dtype == LM_F64 || window || !(p->fill == p->fill))) {
        set_error("lm_roi_dev: LM_I16 output needs an integer volume, no window and a fill that is a number");
        return LM_ERR_INVALID;
    }
    if ((p->flags & ~(LM_ROI_MASK_OUTSIDE | LM_ROI_WINDOW)) != 0 ||
        (window && !(p->window_hi > p->window_lo && p->window_lo > -1e300 && p->window_hi < 1e300))) {
        set_error("lm_roi_dev: unknown flags, or a window without lo < hi (both finite)");
        return LM_ERR_INVALID;
    }
    if (!(p->dilate_mm >= 0.0) || !(p->dilate_mm < 1e15) || !spacing_ok(p->spacing)) {
        set_error("lm_roi_dev: dilate_mm must be >= 0 and finite, spacing finite and > 0");
        return LM_ERR_INVALID;
    }
    const int dim[3] = {n, h, w};
    unsigned long long nout = 1;
    for (int i = 0; i < 3; ++i) {
        const int lo = p->bbox[2 * i], hi = p->bbox[2 * i + 1];
        if (lo < 0 || hi <= lo || hi > dim[i]) {
            set_error("lm_roi_dev: bbox axis %d = [%d, %d) does not lie inside the volume (%d)", i, lo, hi, dim[i]);
            return LM_ERR_INVALID;
        }
        const double st = p->step[i];
        if (!(st > 0.0) || !(st < 1e15)) {
            set_error("lm_roi_dev: step %d must be finite and > 0", i);
            return LM_ERR_INVALID;
        }
        const double want = floor((double)(hi - lo - 1) / st) + 1.0;  // the header's N_i
        if (!(want < 2147483648.0) || p->out_dims[i] != (int)want) {
            set_error("lm_roi_dev: out_dims[%d] = %d is not floor((e - 1) / step) + 1 = %.0f", i, p->out_dims[i], want);
            return LM_ERR_INVALID;
        }
        nout *= (unsigned long long)p->out_dims[i];
        if (nout >= 0x7fffffffull) {
            set_error("lm_roi_dev: output too large (N_0 * N_1 * N_2 must stay below 2^31)");
            return LM_ERR_INVALID;
        }
    }
    LM_DEVICE(e);
    return roi(e, vol_dev, dtype, lab_dev, n, h, w, *p, out_image_dev, out_labels_dev);
}

int lm_spline_prefilter_dev(lm_engine* e, const void* vol_dev, int dtype, int n, int h, int w, double* coef_out_dev) {
    if (!e || !metrics_shape_ok("lm_spline_prefilter_dev", n, h, w)) return LM_ERR_INVALID;
    if (!vol_dev || !coef_out_dev || vol_dev == (const void*)coef_out_dev || n < 1 ||
        !image_dtype_ok(dtype)) {
        set_error("lm_spline_prefilter_dev: bad arguments (device pointers, coef_out_dev not vol_dev, n >= 1, dtype LM_I16 / LM_I32 / LM_I64 / "
                  "LM_F32 / LM_F64)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return spline_prefilter(e, vol_dev, dtype, n, h, w, coef_out_dev);
}

// The checks lm_resample_dev and lm_warp_dev share: the output extents, the mode against the dtypes, the fill.  `coef_source`: the
// cubic mode takes prefiltered float64 coefficients as its source (lm_warp_dev).
static int resample_params_ok(const char* who, int dtype, const lm_resample_params* p, bool coef_source) {
    if (!out_dims_ok(who, p->out_dims)) return 0;
    const bool image = image_dtype_ok(dtype);
    const bool coef = coef_source && p->mode == LM_RS_CUBIC;
    const bool is_float = (dtype == LM_F32 || dtype == LM_F64) && !coef;
    switch (p->mode) {
        case LM_RS_NEAREST:
            if (!image && dtype != LM_U8) {
                set_error("%s: dtype must be LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64, or LM_U8 for labels", who);
                return 0;
            }
            if (p->out_dtype != dtype) {
                set_error("%s: LM_RS_NEAREST returns the raw source values: out_dtype must equal dtype", who);
                return 0;
            }
            break;
        case LM_RS_LINEAR:
        case LM_RS_CUBIC:
            if (coef && dtype != LM_F64) {
                set_error("%s: LM_RS_CUBIC takes the LM_F64 coefficients of lm_spline_prefilter_dev as its source", who);
                return 0;
            }
            if (!image) {
                set_error("%s: LM_RS_LINEAR / LM_RS_CUBIC need dtype LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64", who);
                return 0;
            }
            if (p->out_dtype != LM_F32 && p->out_dtype != LM_F16 && p->out_dtype != LM_I16) {
                set_error("%s: out_dtype must be LM_F32, LM_F16 or LM_I16", who);
                return 0;
            }
            if (p->out_dtype == LM_I16 && (is_float || !(p->fill == p->fill))) {
                set_error("%s: LM_I16 output needs an integer source and a fill that is a number", who);
                return 0;
            }
            break;
        case LM_RS_LABEL_LINEAR:
            if (dtype != LM_U8 || p->out_dtype != LM_U8) {
                set_error("%s: LM_RS_LABEL_LINEAR needs LM_U8 labels in and out", who);
                return 0;
            }
            break;
        default:
            set_error("%s: unknown mode %d", who, p->mode);
            return 0;
    }
    if (p->out_dtype == LM_U8 && !(p->fill >= 0.0 && p->fill <= 255.0)) {
        set_error("%s: the fill of a LM_U8 output must lie in [0, 255]", who);
        return 0;
    }
    if (p->mode == LM_RS_NEAREST && !(dtype == LM_F32 || dtype == LM_F64) && !(p->fill == p->fill)) {
        set_error("%s: an integer output needs a fill that is a number", who);
        return 0;
    }
    return 1;
}

int lm_resample_dev(lm_engine* e, const void* src_dev, int dtype, int n, int h, int w, const lm_resample_params* p, void* out_dev) {
    if (!e || !metrics_shape_ok("lm_resample_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || !src_dev || !out_dev || out_dev == src_dev || n < 1) {
        set_error("lm_resample_dev: bad arguments (device pointers, out_dev not src_dev, params not NULL, n >= 1)");
        return LM_ERR_INVALID;
    }
    if (!resample_params_ok("lm_resample_dev", dtype, p, false)) return LM_ERR_INVALID;
    LM_DEVICE(e);
    return resample(e, src_dev, dtype, n, h, w, *p, out_dev);
}

// the limits the two-volume entry points share: every dimension of both volumes in 1 .. 4096, 32-bit voxel indices
static int pair_shape_ok(const char* who, int fn, int fh, int fw, int mn, int mh, int mw) {
    const int dims[6] = {fn, fh, fw, mn, mh, mw};
    for (int i = 0; i < 6; ++i)
        if (dims[i] < 1 || dims[i] > 4096) {
            set_error("%s: every dimension of the %s volume must lie in 1 .. 4096 (got %d)", who, i < 3 ? "fixed" : "moving", dims[i]);
            return 0;
        }
    if ((unsigned long long)fn * fh * fw >= 0x7fffffffull || (unsigned long long)mn * mh * mw >= 0x7fffffffull) {
        set_error("%s: volume too large (n * h * w must stay below 2^31)", who);
        return 0;
    }
    return 1;
}

int lm_joint_hist_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* fixed_lab_dev,
                      const void* moving_dev, int mdtype, int mn, int mh, int mw, const lm_joint_hist_params* p, int64_t* hist_out_dev,
                      int64_t* counts_out_dev) {
    if (!e) return LM_ERR_INVALID;
    if (!pair_shape_ok("lm_joint_hist_dev", fn, fh, fw, mn, mh, mw)) return LM_ERR_INVALID;
    if (!p || !fixed_dev || !moving_dev || !hist_out_dev || !counts_out_dev) {
        set_error("lm_joint_hist_dev: bad arguments (device pointers and params not NULL; only fixed_lab_dev may be)");
        return LM_ERR_INVALID;
    }
    const int dt[2] = {fdtype, mdtype};
    for (int i = 0; i < 2; ++i)
        if (dt[i] != LM_U8 && dt[i] != LM_I16 && dt[i] != LM_I32 && dt[i] != LM_I64 && dt[i] != LM_F32 && dt[i] != LM_F64) {
            set_error("lm_joint_hist_dev: dtype must be LM_U8 / LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 (got %d)", dt[i]);
            return LM_ERR_INVALID;
        }
    if (p->mode != LM_JH_LINEAR && p->mode != LM_JH_NEAREST) {
        set_error("lm_joint_hist_dev: unknown mode %d", p->mode);
        return LM_ERR_INVALID;
    }
    if (p->bins < 2 || p->bins > 64) {
        set_error("lm_joint_hist_dev: bins must lie in 2 .. 64 (got %d)", p->bins);
        return LM_ERR_INVALID;
    }
    if (p->f_width < 1 || p->m_width < 1) {
        set_error("lm_joint_hist_dev: the HU per bin must be >= 1 on both axes (got %d, %d)", p->f_width, p->m_width);
        return LM_ERR_INVALID;
    }
    for (int i = 0; i < 3; ++i)
        if (p->step[i] < 1 || p->start[i] < 0) {
            set_error("lm_joint_hist_dev: step[%d] must be >= 1 and start[%d] >= 0 (got %d, %d)", i, i, p->step[i], p->start[i]);
            return LM_ERR_INVALID;
        }
    LM_DEVICE(e);
    return joint_hist(e, fixed_dev, fdtype, fn, fh, fw, fixed_lab_dev, moving_dev, mdtype, mn, mh, mw, *p, hist_out_dev, counts_out_dev);
}

int lm_warp_dev(lm_engine* e, const void* src_dev, int dtype, int n, int h, int w, const float* field_dev, const lm_resample_params* p,
                const double field_scale[3], void* out_dev) {
    if (!e || !metrics_shape_ok("lm_warp_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || !src_dev || !out_dev || out_dev == src_dev || (const void*)field_dev == (const void*)out_dev || n < 1 || !finite_all(field_scale, 3)) {
        set_error("lm_warp_dev: bad arguments (device pointers, out_dev neither src_dev nor field_dev, params not NULL, n >= 1, field_scale "
                  "finite)");
        return LM_ERR_INVALID;
    }
    if (!resample_params_ok("lm_warp_dev", dtype, p, true)) return LM_ERR_INVALID;
    LM_DEVICE(e);
    return warp(e, src_dev, dtype, n, h, w, field_dev, *p, field_scale, out_dev);
}

int lm_demons_step_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* fixed_lab_dev,
                       const void* moving_dev, int mdtype, int mn, int mh, int mw, const float* u_dev, const lm_demons_params* p, float* out_dev,
                       int64_t* counts_out_dev) {
    if (!e) return LM_ERR_INVALID;
    if (!pair_shape_ok("lm_demons_step_dev", fn, fh, fw, mn, mh, mw)) return LM_ERR_INVALID;
    if (!p || !fixed_dev || !moving_dev || !u_dev || !out_dev || !counts_out_dev) {
        set_error("lm_demons_step_dev: bad arguments (device pointers and params not NULL; only fixed_lab_dev may be)");
        return LM_ERR_INVALID;
    }
    if (out_dev == u_dev) {
        set_error("lm_demons_step_dev: out_dev must not be u_dev (the step is not in-place)");
        return LM_ERR_INVALID;
    }
    const int dt[2] = {fdtype, mdtype};
    for (int i = 0; i < 2; ++i)
        if (!image_dtype_ok(dt[i])) {
            set_error("lm_demons_step_dev: dtype must be LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 (got %d)", dt[i]);
            return LM_ERR_INVALID;
        }
    if (!finite_all(p->field_scale, 3) || !finite_all(p->grad_scale, 3) || !(p->inv_k2 >= 0.0 && p->inv_k2 < 1e300) || !(p->den_min >= 0.0 && p->den_min < 1e300)) {
        set_error("lm_demons_step_dev: field_scale and grad_scale must be finite, inv_k2 and den_min finite and >= 0");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return demons_step(e, fixed_dev, fdtype, fn, fh, fw, fixed_lab_dev, moving_dev, mdtype, mn, mh, mw, u_dev, *p, out_dev, counts_out_dev);
}

// a device range of lm_pair_map_dev (lo may be NULL: overlaps nothing)
struct ByteRange {
    const char* lo;
    size_t bytes;
};

static bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
    return a.lo && b.lo && a.bytes && b.bytes && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes;
}

int lm_pair_map_dev(lm_engine* e, const void* fixed_dev, int fdtype, int fn, int fh, int fw, const uint8_t* lab_dev, const void* moving_dev,
                    int mdtype, int mn, int mh, int mw, const float* field_dev, const lm_pair_params* p, uint8_t* class_out_dev,
                    float* change_out_dev, float* jac_out_dev, int64_t* table_out_dev) {
    if (!e) return LM_ERR_INVALID;
    if (!pair_shape_ok("lm_pair_map_dev", fn, fh, fw, mn, mh, mw)) return LM_ERR_INVALID;
    if (!p || !fixed_dev || !lab_dev || !moving_dev || !table_out_dev) {
        set_error("lm_pair_map_dev: bad arguments (fixed_dev, lab_dev, moving_dev, params and table_out_dev not NULL; field_dev and the three "
                  "maps may be)");
        return LM_ERR_INVALID;
    }
    if (!image_dtype_ok(fdtype) || !image_dtype_ok(mdtype)) {
        set_error("lm_pair_map_dev: dtype must be LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 (got %d, %d)", fdtype, mdtype);
        return LM_ERR_INVALID;
    }
    if (p->n_labels < 1 || p->n_labels > 16) {
        set_error("lm_pair_map_dev: n_labels must lie in 1 .. 16 (got %d)", p->n_labels);
        return LM_ERR_INVALID;
    }
    const double scalars[6] = {p->jac_scale, p->air, p->fixed_thr, p->moving_thr, p->lo, p->hi};
    if (!finite_all(scalars, 6) || !finite_all(p->A, 9) || !finite_all(p->b, 3) || !finite_all(p->field_scale, 3) || !(p->jac_scale > 0.0) ||
        !(p->lo <= p->hi)) {
        set_error("lm_pair_map_dev: A, b, field_scale, air, the thresholds, lo and hi must be finite, jac_scale finite and > 0, lo <= hi");
        return LM_ERR_INVALID;
    }
    const size_t N = (size_t)fn * fh * fw, M = (size_t)mn * mh * mw;
    const ByteRange in[4] = {{(const char*)fixed_dev, N * dtype_bytes(fdtype)}, {(const char*)lab_dev, N}, {(const char*)moving_dev, M * dtype_bytes(mdtype)},
                             {(const char*)field_dev, 12 * N}};
    const ByteRange out[4] = {{(const char*)class_out_dev, N}, {(const char*)change_out_dev, 4 * N}, {(const char*)jac_out_dev, 4 * N},
                              {(const char*)table_out_dev, (size_t)p->n_labels * LM_PAIR_COLS * 8}};
    for (int a = 0; a < 4; ++a) {
        for (int b = 0; b < 4; ++b)
            if (ranges_overlap(out[a], in[b])) {
                set_error("lm_pair_map_dev: an output must not overlap an input (the call is not in-place)");
                return LM_ERR_INVALID;
            }
        for (int b = a + 1; b < 4; ++b)
            if (ranges_overlap(out[a], out[b])) {
                set_error("lm_pair_map_dev: the outputs must not overlap one another");
                return LM_ERR_INVALID;
            }
    }
    LM_DEVICE(e);
    return pair_map(e, fixed_dev, fdtype, fn, fh, fw, lab_dev, moving_dev, mdtype, mn, mh, mw, field_dev, *p, class_out_dev, change_out_dev,
                    jac_out_dev, table_out_dev);
}

int lm_local_moments_dev(lm_engine* e, const float* f_dev, const float* m_dev, int n, int h, int w, const int32_t radius[3], double* out_dev) {
    if (!e || !metrics_shape_ok("lm_local_moments_dev", n, h, w)) return LM_ERR_INVALID;
    if (!f_dev || !m_dev || !out_dev || !radius || n < 1) {
        set_error("lm_local_moments_dev: bad arguments (device pointers and radius not NULL, n >= 1)");
        return LM_ERR_INVALID;
    }
    for (int i = 0; i < 3; ++i)
        if (radius[i] < 0 || radius[i] > LM_LCC_MAX_RADIUS) {
            set_error("lm_local_moments_dev: radius[%d] = %d must lie in 0 .. %d", i, radius[i], LM_LCC_MAX_RADIUS);
            return LM_ERR_INVALID;
        }
    const size_t N = (size_t)n * h * w;
    const ByteRange out{(const char*)out_dev, 48 * N};
    if (ranges_overlap(out, ByteRange{(const char*)f_dev, 4 * N}) || ranges_overlap(out, ByteRange{(const char*)m_dev, 4 * N})) {
        set_error("lm_local_moments_dev: out_dev must not overlap f_dev or m_dev");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return local_moments(e, f_dev, m_dev, n, h, w, radius, out_dev);
}

int lm_lcc_step_dev(lm_engine* e, const float* f_dev, const float* m_dev, const double* moments_dev, const uint8_t* fixed_lab_dev, int n, int h,
                    int w, const float* u_dev, const lm_lcc_params* p, float* out_dev, int64_t* counts_out_dev) {
    if (!e) return LM_ERR_INVALID;
    if (!p) {
        set_error("lm_lcc_step_dev: bad arguments (device pointers and params not NULL; only fixed_lab_dev may be)");
        return LM_ERR_INVALID;
    }
    if (!pair_shape_ok("lm_lcc_step_dev", n, h, w, p->moving_dims[0], p->moving_dims[1], p->moving_dims[2])) return LM_ERR_INVALID;
    if (!f_dev || !m_dev || !moments_dev || !u_dev || !out_dev || !counts_out_dev || n < 1) {
        set_error("lm_lcc_step_dev: bad arguments (device pointers and params not NULL; only fixed_lab_dev may be)");
        return LM_ERR_INVALID;
    }
    if (out_dev == u_dev) {
        set_error("lm_lcc_step_dev: out_dev must not be u_dev (the step is not in-place)");
        return LM_ERR_INVALID;
    }
    const size_t N = (size_t)n * h * w;
    const ByteRange out{(const char*)out_dev, 12 * N};
    const ByteRange in[6] = {{(const char*)f_dev, 4 * N}, {(const char*)m_dev, 4 * N}, {(const char*)moments_dev, 48 * N},
                             {(const char*)fixed_lab_dev, N}, {(const char*)u_dev, 12 * N}, {(const char*)counts_out_dev, 48}};
    for (int i = 0; i < 6; ++i)
        if (ranges_overlap(out, in[i])) {
            set_error("lm_lcc_step_dev: out_dev must not overlap an input or the counts (the step is not in-place)");
            return LM_ERR_INVALID;
        }
    if (!finite_all(p->A, 9) || !finite_all(p->b, 3) || !finite_all(p->field_scale, 3) || !finite_all(p->grad_scale, 3) ||
        !(p->inv_k2 >= 0.0 && p->inv_k2 < 1e300) || !(p->den_min >= 0.0 && p->den_min < 1e300) || !(p->var_eps >= 0.0 && p->var_eps < 1e300) ||
        !(p->a_max > 0.0 && p->a_max < 1e300)) {
        set_error("lm_lcc_step_dev: A, b, field_scale and grad_scale must be finite, inv_k2, den_min and var_eps finite and >= 0, a_max finite "
                  "and > 0");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return lcc_step(e, f_dev, m_dev, moments_dev, fixed_lab_dev, n, h, w, u_dev, *p, out_dev, counts_out_dev);
}

int lm_jacobian_dev(lm_engine* e, const float* field_dev, int n, int h, int w, const double field_scale[3], float* det_out_dev,
                    int64_t* counts_out_dev) {
    if (!e || !metrics_shape_ok("lm_jacobian_dev", n, h, w)) return LM_ERR_INVALID;
    if (!field_dev || !det_out_dev || n < 1 || !finite_all(field_scale, 3)) {
        set_error("lm_jacobian_dev: bad arguments (device pointers, n >= 1, field_scale finite; only counts_out_dev may be NULL)");
        return LM_ERR_INVALID;
    }
    const float* field_end = field_dev + 3 * (size_t)n * h * w;
    if (det_out_dev >= field_dev && det_out_dev < field_end) {
        set_error("lm_jacobian_dev: det_out_dev must not lie inside the field");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return jacobian(e, field_dev, n, h, w, field_scale, det_out_dev, counts_out_dev);
}

int lm_field_combine_dev(lm_engine* e, const float* add_dev, const float* coord_dev, const float* src_dev, int n, int h, int w,
                         const float* ref_dev, const lm_field_combine_params* p, float* out_dev, int64_t* counts_out_dev) {
    if (!e || !metrics_shape_ok("lm_field_combine_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || !src_dev || !out_dev || n < 1) {
        set_error("lm_field_combine_dev: bad arguments (src_dev, out_dev and params not NULL, n >= 1; add_dev, coord_dev, ref_dev and "
                  "counts_out_dev may be NULL)");
        return LM_ERR_INVALID;
    }
    if (out_dev == src_dev || out_dev == add_dev || out_dev == coord_dev || out_dev == ref_dev) {
        set_error("lm_field_combine_dev: out_dev must not be one of the inputs (the call is not in-place)");
        return LM_ERR_INVALID;
    }
    if (!out_dims_ok("lm_field_combine_dev", p->out_dims)) return LM_ERR_INVALID;
    const double ab[2] = {p->alpha, p->beta};
    if (!finite_all(p->field_scale, 3) || !finite_all(p->A, 9) || !finite_all(p->b, 3) || !finite_all(p->R, 9) || !finite_all(ab, 2)) {
        set_error("lm_field_combine_dev: field_scale, A, b, R, alpha and beta must be finite");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return field_combine(e, add_dev, coord_dev, src_dev, n, h, w, ref_dev, *p, out_dev, counts_out_dev);
}

int lm_nearest_label_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], const double* spacing,
                         float* d2_out_dev, uint8_t* near_out_dev) {
    if (!e || !metrics_shape_ok("lm_nearest_label_dev", n, h, w)) return LM_ERR_INVALID;
    if ((n > 0 && (!lab_dev || !near_out_dev || near_out_dev == lab_dev)) || !keep || !spacing_ok(spacing)) {
        set_error("lm_nearest_label_dev: bad arguments (device pointers, near_out_dev not lab_dev, keep table, spacing finite and > 0)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return nearest_label(e, lab_dev, n, h, w, keep, spacing, d2_out_dev, near_out_dev);
}

int lm_morph_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const lm_morph_params* p, uint8_t* out_dev,
                 int64_t changed_host[2]) {
    if (!e || !metrics_shape_ok("lm_morph_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || !changed_host || (n > 0 && (!lab_dev || !out_dev))) {
        set_error("lm_morph_dev: bad arguments (device pointers, params and changed_host not NULL)");
        return LM_ERR_INVALID;
    }
    if (p->op < LM_MORPH_DILATE || p->op > LM_MORPH_CLOSE) {
        set_error("lm_morph_dev: unknown op %d (LM_MORPH_DILATE, LM_MORPH_ERODE, LM_MORPH_OPEN or LM_MORPH_CLOSE)", p->op);
        return LM_ERR_INVALID;
    }
    if (!(p->radius_mm >= 0.0) || (!(p->radius_mm < 1e15) && !(p->op == LM_MORPH_DILATE && std::isinf(p->radius_mm))) ||
        !spacing_ok(p->spacing)) {
        set_error("lm_morph_dev: radius_mm must be >= 0 and below 1e15 (+inf for LM_MORPH_DILATE only), spacing > 0 and below 1e15");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return morph(e, lab_dev, n, h, w, *p, out_dev, changed_host);
}

int lm_components_dev(lm_engine* e, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h, int w,
                      const lm_components_params* p, int32_t* ids_out_dev, int64_t* total_out, int64_t counts_host[3][256]) {
    if (!e || !metrics_shape_ok("lm_components_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || !total_out || !counts_host || (n > 0 && (!lab_dev || !ids_out_dev)) || (vol_dev && !image_dtype_ok(dtype))) {
        set_error("lm_components_dev: bad arguments (device pointers, params, total_out and counts_host not NULL, dtype LM_I16 / LM_I32 / "
                  "LM_I64 / LM_F32 / LM_F64 with an image)");
        return LM_ERR_INVALID;
    }
    if (p->connectivity != 6 && p->connectivity != 26) {
        set_error("lm_components_dev: connectivity must be 6 or 26, got %d", p->connectivity);
        return LM_ERR_INVALID;
    }
    if (p->has_lo && p->has_hi && p->lo > p->hi) {
        set_error("lm_components_dev: empty HU range (lo %d > hi %d)", p->lo, p->hi);
        return LM_ERR_INVALID;
    }
    if (p->per_label && p->keep[0]) {
        set_error("lm_components_dev: keep[0] with per_label (the key of a selected voxel must not be 0)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return components(e, lab_dev, vol_dev, dtype, n, h, w, *p, ids_out_dev, total_out, &counts_host[0][0]);
}

int lm_component_table_dev(lm_engine* e, const int32_t* ids_dev, const uint8_t* lab_dev, const void* vol_dev, int dtype, int n, int h,
                           int w, lm_component* table_host, int64_t cap, int64_t* total_out) {
    if (!e || !metrics_shape_ok("lm_component_table_dev", n, h, w)) return LM_ERR_INVALID;
    if (!total_out || cap < 0 || cap >= 0x7fffffffLL || (cap > 0 && !table_host) || (n > 0 && (!ids_dev || !lab_dev)) ||
        (vol_dev && !image_dtype_ok(dtype))) {
        set_error("lm_component_table_dev: bad arguments (device pointers, total_out not NULL, 0 <= cap < 2^31 with table_host, dtype "
                  "LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64 with an image)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return component_table(e, ids_dev, lab_dev, vol_dev, dtype, n, h, w, table_host, cap, total_out);
}

int lm_component_table_launch(int64_t nvox, int64_t* workgroups, int64_t* voxels_per_workgroup) {
    if (nvox < 0 || nvox >= 0x7fffffffLL || !workgroups || !voxels_per_workgroup) {
        set_error("lm_component_table_launch: bad arguments (0 <= nvox < 2^31)");
        return LM_ERR_INVALID;
    }
    long long g = 0, per = 0;
    component_table_launch((size_t)nvox, &g, &per);
    *workgroups = g;
    *voxels_per_workgroup = per;
    return LM_OK;
}

// Test seam.  Every DevBuf / HostBuf member of the engine registers itself (engine.h: BufRegistry), so nothing is listed here but the
// EXEMPTIONS -- the buffers whose contents are state between calls rather than scratch of one call:
//   - Pipe::vol / out / stage (lm_pipe_*): a volume lives there from lm_pipe_upload to lm_pipe_download;
//   - SlabState's buffers between lm_slab_begin and the last lm_slab_step: the call is refused while an exchange is open
//     (idle, they are scratch and are filled);
//   - MeshWorkspace between lm_mesh_plan_dev and the lm_mesh_dev that consumes the plan: the plan is dropped (that lm_mesh_dev plans
//     itself, as it does for any other labels).
// Model weights, zero_page and range_flag are not DevBufs and stay as they are.
int lm_debug_fill_workspaces(lm_engine* e, int byte, int64_t* bytes_filled) {
    if (!e || !bytes_filled || byte < 0 || byte > 255) {
        set_error("lm_debug_fill_workspaces: bad arguments (0 <= byte <= 255, bytes_filled not NULL)");
        return LM_ERR_INVALID;
    }
    *bytes_filled = 0;
    if (e->slab.phase >= 0) {
        set_error("lm_debug_fill_workspaces: a slab exchange is open (lm_slab_begin without the last lm_slab_step)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    auto sync = [&]() -> int {
        for (hipStream_t s : {e->stream, e->stream2, e->copy_stream, e->pipe.up_stream, e->pipe.out_stream})
            if (s) LM_HIP(hipStreamSynchronize(s));
        return LM_OK;
    };
    auto in_pipe = [&](const void* b) {
        const char* c = reinterpret_cast<const char*>(b);
        const char* lo = reinterpret_cast<const char*>(&e->pipe);
        return c >= lo && c < lo + sizeof(e->pipe);
    };
    LM_TRY(sync());
    e->mesh.planned = false;
    int64_t total = 0;
    for (DevBuf* b : e->bufs.dev) {
        if (in_pipe(b) || !b->p || !b->cap) continue;
        LM_HIP(hipMemset(b->p, byte, b->cap));
        total += (int64_t)b->cap;
    }
    for (HostBuf* b : e->bufs.host) {
        if (in_pipe(b) || !b->p || !b->cap) continue;
        std::memset(b->p, byte, b->cap);
        total += (int64_t)b->cap;
    }
    LM_HIP(hipDeviceSynchronize());
    LM_TRY(sync());
    *bytes_filled = total;
    return LM_OK;
}

int lm_relabel_dev(lm_engine* e, const int32_t* ids_dev, const int32_t* lut_dev, int64_t lut_len, int64_t nvox, int32_t* out_dev) {
    if (!e || nvox < 0 || nvox >= 0x7fffffffLL || lut_len < 0 || lut_len > 0x7fffffffLL ||
        (nvox > 0 && (!ids_dev || !out_dev || (lut_len > 0 && !lut_dev)))) {
        set_error("lm_relabel_dev: bad arguments (device pointers, 0 <= nvox < 2^31, 0 <= lut_len <= 2^31 - 1)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return relabel(e, ids_dev, lut_dev, lut_len, nvox, out_dev);
}

int lm_filter_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev, int n, int h, int w, const lm_filter_params* p,
                  void* out_dev) {
    if (!e || !metrics_shape_ok("lm_filter_dev", n, h, w)) return LM_ERR_INVALID;
    if (!p || (n > 0 && (!vol_dev || !out_dev || out_dev == vol_dev))) {
        set_error("lm_filter_dev: bad arguments (device pointers, out_dev not vol_dev, params not NULL)");
        return LM_ERR_INVALID;
    }
    if ((p->flags & ~(LM_FILTER_MASKED | LM_FILTER_INDICATOR | LM_FILTER_FILL_OUTSIDE)) != 0) {
        set_error("lm_filter_dev: unknown flags");
        return LM_ERR_INVALID;
    }
    const bool masked = (p->flags & LM_FILTER_MASKED) != 0;
    if (masked && n > 0 && !lab_dev) {
        set_error("lm_filter_dev: LM_FILTER_MASKED needs labels (lab_dev is NULL)");
        return LM_ERR_INVALID;
    }
    if (p->kind == LM_FILTER_MEDIAN) {
        if (dtype != LM_I16 && dtype != LM_I32 && dtype != LM_F32) {
            set_error("lm_filter_dev: the median takes dtype LM_I16, LM_I32 or LM_F32");
            return LM_ERR_INVALID;
        }
        for (int i = 0; i < 3; ++i)
            if (p->size[i] != 1 && p->size[i] != 3 && p->size[i] != 5) {
                set_error("lm_filter_dev: median size[%d] = %d must be 1, 3 or 5", i, p->size[i]);
                return LM_ERR_INVALID;
            }
        if (p->flags & LM_FILTER_INDICATOR) {
            set_error("lm_filter_dev: LM_FILTER_INDICATOR belongs to the separable kind");
            return LM_ERR_INVALID;
        }
        if (masked && (p->flags & LM_FILTER_FILL_OUTSIDE) && dtype != LM_F32) {
            const double lim = dtype == LM_I16 ? 32768.0 : 2147483648.0;
            if (!(p->fill >= -lim && p->fill < lim) || p->fill != std::floor(p->fill)) {
                set_error("lm_filter_dev: fill %g is not a value of the integer dtype", (double)p->fill);
                return LM_ERR_INVALID;
            }
        }
    } else if (p->kind == LM_FILTER_SEPARABLE) {
        if (!image_dtype_ok(dtype)) {
            set_error("lm_filter_dev: dtype LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64");
            return LM_ERR_INVALID;
        }
        for (int i = 0; i < 3; ++i) {
            const int r = p->radius[i];
            if (r < 0 || r > 32) {
                set_error("lm_filter_dev: radius[%d] = %d must lie in 0 .. 32", i, r);
                return LM_ERR_INVALID;
            }
            for (int k = 0; masked && k <= 2 * r; ++k)
                if (!(p->taps[i][k] >= 0.0f) || (k == r && !(p->taps[i][k] > 0.0f))) {
                    set_error("lm_filter_dev: the masked form needs taps >= 0 and a centre tap > 0 (axis %d, tap %d = %g)", i, k - r,
                              (double)p->taps[i][k]);
                    return LM_ERR_INVALID;
                }
        }
    } else {
        set_error("lm_filter_dev: unknown kind %d (LM_FILTER_MEDIAN or LM_FILTER_SEPARABLE)", p->kind);
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return filter(e, vol_dev, dtype, lab_dev, n, h, w, *p, out_dev);
}

static int vessel_args_ok(const char* who, lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev, int n, int h, int w,
                          const lm_vessel_params* p, const void* out_dev, int max_scales) {
    if (!e || !metrics_shape_ok(who, n, h, w)) return 0;
    if (!p || (n > 0 && (!vol_dev || !out_dev || out_dev == vol_dev))) {
        set_error("%s: bad arguments (device pointers, the output not vol_dev, params not NULL)", who);
        return 0;
    }
    if ((p->flags & ~(LM_VESSEL_MASKED | LM_VESSEL_DARK)) != 0) {
        set_error("%s: unknown flags", who);
        return 0;
    }
    if ((p->flags & LM_VESSEL_MASKED) && n > 0 && !lab_dev) {
        set_error("%s: LM_VESSEL_MASKED needs labels (lab_dev is NULL)", who);
        return 0;
    }
    if (!image_dtype_ok(dtype)) {
        set_error("%s: dtype LM_I16 / LM_I32 / LM_I64 / LM_F32 / LM_F64", who);
        return 0;
    }
    if (p->n_scales < 1 || p->n_scales > max_scales) {
        set_error("%s: n_scales = %d must lie in 1 .. %d", who, p->n_scales, max_scales);
        return 0;
    }
    for (int s = 0; s < p->n_scales; ++s)
        for (int i = 0; i < 3; ++i)
            if (p->scales[s].radius[i] < 0 || p->scales[s].radius[i] > 32) {
                set_error("%s: scales[%d].radius[%d] = %d must lie in 0 .. 32", who, s, i, p->scales[s].radius[i]);
                return 0;
            }
    return 1;
}

int lm_hessian_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev, int n, int h, int w, const lm_vessel_params* p,
                   float* comp_out_dev, float* eig_out_dev) {
    if (!vessel_args_ok("lm_hessian_dev", e, vol_dev, dtype, lab_dev, n, h, w, p, comp_out_dev, 1)) return LM_ERR_INVALID;
    LM_DEVICE(e);
    return hessian(e, vol_dev, dtype, lab_dev, n, h, w, *p, comp_out_dev, eig_out_dev);
}

int lm_vesselness_dev(lm_engine* e, const void* vol_dev, int dtype, const uint8_t* lab_dev, int n, int h, int w, const lm_vessel_params* p,
                      float* v_out_dev, uint8_t* scale_out_dev) {
    if (!vessel_args_ok("lm_vesselness_dev", e, vol_dev, dtype, lab_dev, n, h, w, p, v_out_dev, LM_VESSEL_MAX_SCALES)) return LM_ERR_INVALID;
    for (float k : {p->ka, p->kb, p->kc})
        if (!(k >= 0.0f && k <= 3.0e38f)) {
            set_error("lm_vesselness_dev: ka, kb and kc must be >= 0 and finite (got %g, %g, %g)", (double)p->ka, (double)p->kb, (double)p->kc);
            return LM_ERR_INVALID;
        }
    LM_DEVICE(e);
    return vesselness(e, vol_dev, dtype, lab_dev, n, h, w, *p, v_out_dev, scale_out_dev);
}

int lm_vessel_counts_dev(lm_engine* e, const float* v_dev, const uint8_t* scale_dev, const uint8_t* lab_dev, int n, int h, int w, int n_labels,
                         float threshold, int64_t* counts_host) {
    if (!e || !metrics_shape_ok("lm_vessel_counts_dev", n, h, w)) return LM_ERR_INVALID;
    if (!counts_host || n_labels < 1 || n_labels > 16 || (n > 0 && (!v_dev || !scale_dev || !lab_dev))) {
        set_error("lm_vessel_counts_dev: bad arguments (device pointers, 1 <= n_labels <= 16, counts_host not NULL)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return vessel_counts(e, v_dev, scale_dev, lab_dev, n, h, w, n_labels, threshold, counts_host);
}

int lm_skeleton_dev(lm_engine* e, const uint8_t* sel_dev, int n, int h, int w, const uint8_t keep[256], uint8_t* out_dev, int64_t info_host[4]) {
    if (!e || !metrics_shape_ok("lm_skeleton_dev", n, h, w)) return LM_ERR_INVALID;
    if (!keep || !info_host || (n > 0 && (!sel_dev || !out_dev))) {
        set_error("lm_skeleton_dev: bad arguments (device pointers, keep table and info_host not NULL)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return skeleton(e, sel_dev, n, h, w, keep, out_dev, info_host);
}

int lm_skeleton_points_dev(lm_engine* e, const uint8_t* skel_dev, const float* d2_dev, int n, int h, int w, int64_t cap, int32_t* index_out_dev,
                           uint8_t* code_out_dev, float* d2_out_dev, int64_t* total_out) {
    if (!e || !metrics_shape_ok("lm_skeleton_points_dev", n, h, w)) return LM_ERR_INVALID;
    if (!total_out || cap < 0 || (n > 0 && !skel_dev) || (cap > 0 && (!index_out_dev || !code_out_dev || (d2_dev && !d2_out_dev)))) {
        set_error("lm_skeleton_points_dev: bad arguments (device pointers, cap >= 0, d2_out_dev with d2_dev, total_out not NULL)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return skeleton_points(e, skel_dev, d2_dev, n, h, w, cap, index_out_dev, code_out_dev, d2_out_dev, total_out);
}

int lm_calibre_dev(lm_engine* e, const uint8_t* skel_dev, const uint8_t* sel_dev, const uint8_t keep[256], const uint8_t* lab_dev, int n, int h,
                   int w, const double* spacing, const double* edges_mm, int n_edges, int n_labels, uint8_t* class_out_dev, float* d2_out_dev,
                   int64_t* counts_host) {
    if (!e || !metrics_shape_ok("lm_calibre_dev", n, h, w)) return LM_ERR_INVALID;
    if (!keep || !counts_host || n_labels < 2 || n_labels > 16 || !spacing_ok(spacing) ||
        (n > 0 && (!skel_dev || !sel_dev || !class_out_dev || class_out_dev == skel_dev || class_out_dev == sel_dev || class_out_dev == lab_dev))) {
        set_error("lm_calibre_dev: bad arguments (device pointers, class_out_dev not an input, 2 <= n_labels <= 16, spacing finite and > 0)");
        return LM_ERR_INVALID;
    }
    bool ok = edges_mm && n_edges >= 1 && n_edges <= LM_CALIBRE_MAX_EDGES;
    for (int j = 0; ok && j < n_edges; ++j) ok = edges_mm[j] > 0.0 && edges_mm[j] < 1e15 && (j == 0 || edges_mm[j] > edges_mm[j - 1]);
    if (!ok) {
        set_error("lm_calibre_dev: edges_mm must hold 1 .. %d strictly ascending values > 0 and < 1e15", LM_CALIBRE_MAX_EDGES);
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return calibre(e, skel_dev, sel_dev, keep, lab_dev, n, h, w, spacing, edges_mm, n_edges, n_labels, class_out_dev, d2_out_dev, counts_host);
}

int lm_vessel_mask_dev(lm_engine* e, const float* v_dev, const uint8_t* lab_dev, int n, int h, int w, float threshold, uint8_t* out_dev) {
    if (!e || !metrics_shape_ok("lm_vessel_mask_dev", n, h, w)) return LM_ERR_INVALID;
    if (n > 0 && (!v_dev || !lab_dev || !out_dev)) {
        set_error("lm_vessel_mask_dev: bad arguments (device pointers)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return vessel_mask(e, v_dev, lab_dev, n, h, w, threshold, out_dev);
}

int lm_seed_cost_dev(lm_engine* e, const void* vol_dev, int dtype, int n, int h, int w, const int64_t* seeds, int n_seeds, int cap_hu,
                     int64_t max_rounds, int16_t* cost_out_dev, int64_t* curve_host, int64_t info_host[4]) {
    if (!e || !metrics_shape_ok("lm_seed_cost_dev", n, h, w)) return LM_ERR_INVALID;
    if (!seeds || n_seeds < 1 || n_seeds > LM_SEED_MAX || cap_hu < -1023 || cap_hu > 3071 || max_rounds < 0 || !curve_host || !info_host ||
        !image_dtype_ok(dtype) || (n > 0 && (!vol_dev || !cost_out_dev || (const void*)cost_out_dev == vol_dev))) {
        set_error("lm_seed_cost_dev: bad arguments (device pointers, dtype int16 / int32 / int64 / float32 / float64, 1 .. %d seeds, "
                  "-1023 <= cap_hu <= 3071, max_rounds >= 0, curve_host and info_host not NULL)", LM_SEED_MAX);
        return LM_ERR_INVALID;
    }
    const long long nvox = (long long)n * h * w;
    for (int i = 0; i < n_seeds; ++i)
        if (seeds[i] < 0 || seeds[i] >= nvox) {
            set_error("lm_seed_cost_dev: seed %d (%lld) lies outside the volume of %lld voxels", i, (long long)seeds[i], nvox);
            return LM_ERR_INVALID;
        }
    LM_DEVICE(e);
    return seed_cost(e, vol_dev, dtype, n, h, w, seeds, n_seeds, cap_hu, max_rounds, cost_out_dev, curve_host, info_host);
}

int lm_seed_cost_bricks(int n, int h, int w, int64_t* bricks_out, int32_t brick_out[3]) {
    if (!bricks_out || !brick_out || !metrics_shape_ok("lm_seed_cost_bricks", n, h, w)) return LM_ERR_INVALID;
    long long b;
    int br[3];
    seed_cost_bricks(n, h, w, &b, br);
    *bricks_out = b;
    brick_out[0] = br[0], brick_out[1] = br[1], brick_out[2] = br[2];
    return LM_OK;
}

int lm_airway_mask_dev(lm_engine* e, const int16_t* cost_dev, const uint8_t* lab_dev, int n, int h, int w, int threshold, uint8_t* mask_out_dev,
                       int64_t counts_host[256]) {
    if (!e || !metrics_shape_ok("lm_airway_mask_dev", n, h, w)) return LM_ERR_INVALID;
    if (!counts_host || threshold < -32768 || threshold > 32766 ||
        (n > 0 && (!cost_dev || !mask_out_dev || (const void*)mask_out_dev == (const void*)cost_dev || (lab_dev && mask_out_dev == lab_dev)))) {
        set_error("lm_airway_mask_dev: bad arguments (device pointers, mask_out_dev not an input, -32768 <= threshold <= 32766, counts_host not NULL)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return airway_mask(e, cost_dev, lab_dev, n, h, w, threshold, mask_out_dev, counts_host);
}

int lm_mesh_plan_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], int32_t bbox_out[6],
                     int64_t* n_vertices, int64_t* n_quads) {
    if (!e || !metrics_shape_ok("lm_mesh_plan_dev", n, h, w)) return LM_ERR_INVALID;
    if ((n > 0 && !lab_dev) || !keep || !bbox_out || !n_vertices || !n_quads) {
        set_error("lm_mesh_plan_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return mesh_plan(e, lab_dev, n, h, w, keep, bbox_out, n_vertices, n_quads);
}

int lm_mesh_dev(lm_engine* e, const uint8_t* lab_dev, int n, int h, int w, const uint8_t keep[256], int smooth, float lambda, float mu,
                float* verts_out_dev, int64_t n_vertices_cap, int32_t* quads_out_dev, int64_t n_quads_cap) {
    if (!e || !metrics_shape_ok("lm_mesh_dev", n, h, w)) return LM_ERR_INVALID;
    if ((n > 0 && !lab_dev) || !keep || !verts_out_dev || !quads_out_dev || n_vertices_cap < 0 || n_quads_cap < 0 || smooth < 0 ||
        smooth > 100000 || !(lambda > -1e30f && lambda < 1e30f) || !(mu > -1e30f && mu < 1e30f)) {
        set_error("lm_mesh_dev: bad arguments (device pointers, capacities >= 0, 0 <= smooth <= 100000, finite lambda and mu)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return mesh(e, lab_dev, n, h, w, keep, smooth, lambda, mu, verts_out_dev, n_vertices_cap, quads_out_dev, n_quads_cap);
}

int lm_slab_begin(lm_engine* e, uint8_t* lab_slab_dev, int n, int h, int w, int rank, int world, int z0, int n_total, const int* spare,
                  int n_spare, int skip_below) {
    if (!e || !lab_slab_dev || n_spare < 0) {
        set_error("lm_slab_begin: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return slab_begin(e, lab_slab_dev, n, h, w, rank, world, z0, n_total, spare, n_spare, skip_below);
}

int64_t lm_slab_pending(lm_engine* e) { return (e && e->slab.phase >= 0) ? (int64_t)e->slab.pending : -1; }

int lm_slab_pending_uniform(lm_engine* e) { return (e && e->slab.phase >= 0 && e->slab.pending_uniform) ? 1 : 0; }

int lm_slab_emit(lm_engine* e, int32_t* dst_dev) {
    if (!e) return LM_ERR_INVALID;
    LM_DEVICE(e);
    return slab_emit(e, dst_dev);
}

int lm_slab_step(lm_engine* e, const int32_t* gathered_dev, int64_t stride, const int64_t* lens) {
    if (!e) return LM_ERR_INVALID;
    LM_DEVICE(e);
    static_assert(sizeof(long long) == sizeof(int64_t), "");
    return slab_step(e, gathered_dev, (long long)stride, reinterpret_cast<const long long*>(lens));
}

int lm_postprocess_info(lm_engine* e, int64_t info[5]) {
    if (!e || !info) return LM_ERR_INVALID;
    info[0] = e->post_info.regions;
    info[1] = e->post_info.boundary_records;
    info[2] = e->post_info.processed;
    info[3] = e->post_info.merged;
    info[4] = (int64_t)(e->post_info.host_replay_ms * 1000.0);
    return LM_OK;
}

// res_l.max() of mask.py:228 on the voxels this engine holds (a rank's slab: the pipeline combines the ranks' maxima)
int lm_label_max_dev(lm_engine* e, const uint8_t* lab_dev, size_t nvox, int* max_out) {
    if (!e || (!lab_dev && nvox) || !max_out) {
        set_error("lm_label_max_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    *max_out = 0;
    if (nvox == 0) return LM_OK;
    LM_DEVICE(e);
    LM_TRY(e->post.scalars.reserve(4096));
    unsigned* mx_dev = e->post.scalars.as<unsigned>() + 2;
    hipError_t err = volume_max(lab_dev, mx_dev, nvox, e->stream);
    if (err != hipSuccess) {
        set_error("volume_max failed: %s", hipGetErrorString(err));
        return LM_ERR_DEVICE;
    }
    unsigned mx = 0;
    LM_HIP(hipMemcpyAsync(&mx, mx_dev, sizeof mx, hipMemcpyDeviceToHost, e->stream));
    LM_HIP(hipStreamSynchronize(e->stream));
    *max_out = (int)mx;
    return LM_OK;
}

// mask.py:229-230 with a spare label the caller determined (multi-GPU: max over ALL ranks' slabs + 1)
int lm_fuse_spare_dev(lm_engine* e, uint8_t* res_l_dev, const uint8_t* res_r_dev, size_t nvox, int spare) {
    if (!e || ((!res_l_dev || !res_r_dev) && nvox) || spare < 0 || spare > 255) {
        set_error("lm_fuse_spare_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    if (nvox == 0) return LM_OK;
    LM_DEVICE(e);
    e->prof.begin(e->stream, e->prof.kind_id("fuse_labels"), 0, (double)nvox * 3);
    const hipError_t err = fuse_labels(res_l_dev, res_r_dev, (uint8_t)spare, nvox, e->stream);
    e->prof.end(e->stream);
    if (err != hipSuccess) {
        set_error("fuse_labels failed: %s", hipGetErrorString(err));
        return LM_ERR_DEVICE;
    }
    return LM_OK;
}

int lm_fuse_dev(lm_engine* e, uint8_t* res_l_dev, const uint8_t* res_r_dev, size_t nvox, int* spare_out) {
    if (!e || !res_l_dev || !res_r_dev) return LM_ERR_INVALID;
    int mx = 0;
    LM_TRY(lm_label_max_dev(e, res_l_dev, nvox, &mx));
    const int spare = (mx + 1) & 0xff;  // res_l.max() + 1 in uint8 arithmetic (mask.py:228)
    LM_TRY(lm_fuse_spare_dev(e, res_l_dev, res_r_dev, nvox, spare));
    if (spare_out) *spare_out = spare;
    return LM_OK;
}

int lm_apply_dev(lm_engine* e, int slot, int fill_slot, const void* vol_dev, int dtype, int n, int h, int w, int batch_size,
                 int volume_postprocessing, uint8_t* out_dev) {
    if (!e || !vol_dev || !out_dev || n < 0 || h <= 0 || w <= 0) {
        set_error("lm_apply_dev: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    return apply_volume(e, slot, fill_slot, vol_dev, dtype, n, h, w, batch_size, volume_postprocessing, out_dev);
}

int lm_apply_probs_dev(lm_engine* e, int slot, const void* vol_dev, int dtype, int n, int h, int w, int batch_size, int volume_postprocessing,
                       uint8_t* labels_out_dev, int prob_dtype, void* probs_out_dev) {
    if (!e || !vol_dev || !probs_out_dev || n < 0 || h <= 0 || w <= 0 || (prob_dtype != LM_F32 && prob_dtype != LM_F16)) {
        set_error("lm_apply_probs_dev: bad arguments (prob_dtype LM_F32 or LM_F16, probs_out_dev not NULL)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    uint8_t* lab = labels_out_dev;
    if (lab == nullptr) {  // the labels are computed anyway (post-processing): into the engine's own result buffer
        LM_TRY(e->app.out.reserve((size_t)std::max(n, 1) * h * w));
        lab = e->app.out.as<uint8_t>();
    }
    return apply_volume(e, slot, -1, vol_dev, dtype, n, h, w, batch_size, volume_postprocessing, lab, prob_dtype, probs_out_dev);
}

int lm_apply_host(lm_engine* e, int slot, int fill_slot, const void* vol_host, int dtype, int n, int h, int w, int batch_size,
                  int volume_postprocessing, uint8_t* out_host) {
    return lm_apply_host_ex(e, slot, fill_slot, vol_host, dtype, n, h, w, batch_size, volume_postprocessing, out_host, 0u);
}

int lm_apply_host_ex(lm_engine* e, int slot, int fill_slot, const void* vol_host, int dtype, int n, int h, int w, int batch_size,
                     int volume_postprocessing, uint8_t* out_host, unsigned flags) {
    if (!e || !vol_host || !out_host || n < 0 || h <= 0 || w <= 0 || (flags & ~(unsigned)LM_APPLY_OUT_SCRATCH)) {
        set_error("lm_apply_host: bad arguments");
        return LM_ERR_INVALID;
    }
    // LM_APPLY_OUT_SCRATCH: the output array's previous contents are of no value to the caller.  The helper thread then fills it
    // with zeros while the network runs and, at the end, only the slab of slices x rows that holds a label is copied back (a
    // strided copy) -- a lung mask is mostly background: 31 of 79 MB on the bench phantom.
    const bool scratch = (flags & LM_APPLY_OUT_SCRATCH) != 0;
    const int esz = dtype == LM_I16 ? 2 : ((dtype == LM_I32 || dtype == LM_F32) ? 4 : ((dtype == LM_I64 || dtype == LM_F64) ? 8 : 0));
    if (!esz) {
        set_error("lm_apply_host: unsupported dtype code %d", dtype);
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    const size_t nvox = (size_t)n * h * w, slice = (size_t)h * w;
    LM_TRY(e->app.vol.reserve(nvox * esz));
    LM_TRY(e->app.out.reserve(nvox));
    // mask.py:178-186 moves every batch to the device and back on its own; here the boundary is crossed once per volume, in two
    // pieces.  The head (two batches) goes in on the main stream, and while it is pre-processed and run through the network the
    // engine's helper thread (persistent: started on the first call, parked between calls) (a) copies the tail in on a second
    // stream and (b) faults in every page of the caller's output array WITHOUT changing it (each page's first byte is read and
    // written back), so that the copy back at the end does not take the page faults of a freshly allocated buffer.  The
    // caller's array is only ever overwritten by the final copy of a successful call; on any error it is left as it was.
    if (batch_size <= 0) batch_size = 20;
    // two lanes: the head is the main stream's first batch, the second lane's first batch follows as a piece of its own (`mid`)
    const bool two_lanes = e->n_streams > 1 && e->stream2 != nullptr;
    const int mid = (two_lanes && n > 2 * batch_size) ? 2 * batch_size : 0;
    const int head = mid ? batch_size : (two_lanes ? 2 : 1) * batch_size;
    bool split = n > head;
    if (split && !e->copy_stream) {
        if (hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e->tail_ready, hipEventDisableTiming) != hipSuccess) {
            set_error("lm_apply_host: creating the copy stream failed");
            return LM_ERR_DEVICE;
        }
    }
    const bool out_pinned = host_range_is_pinned(out_host, nvox);
    const bool threaded = e->helper.start();  // false: no thread could be created -- one copy on the main stream, no page touching
    if (!threaded) split = false;
    if (split && mid && !e->mid_ready && hipEventCreateWithFlags(&e->mid_ready, hipEventDisableTiming) != hipSuccess) {
        set_error("lm_apply_host: creating the copy events failed");
        return LM_ERR_DEVICE;
    }
    const int tail0 = (split && mid) ? mid : head;  // first slice of the tail piece
    e->mid_enqueued.store(0, std::memory_order_release);
    static const bool timing = [] { const char* v = getenv("LM_HOST_TIMING"); return v && v[0] == '1'; }();  // stderr breakdown of this call
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    double t_tail = 0, t_touch = 0;
    e->tail_enqueued.store(0, std::memory_order_release);
    if (threaded)
        e->helper.run([&, split] {
            hipError_t terr = hipSuccess;
            if (split) {
                terr = hipSetDevice(e->device);
                // (a pageable source makes this call return only when the data has been staged: that is why it lives on this thread)
                if (terr == hipSuccess && tail0 > head) {  // lane 1's first batch, in front of the tail
                    terr = hipMemcpyAsync(reinterpret_cast<char*>(e->app.vol.p) + (size_t)head * slice * esz, reinterpret_cast<const char*>(vol_host) + (size_t)head * slice * esz,
                                          (size_t)(tail0 - head) * slice * esz, hipMemcpyHostToDevice, e->copy_stream);
                    if (terr == hipSuccess) terr = hipEventRecord(e->mid_ready, e->copy_stream);
                    e->mid_enqueued.store(terr == hipSuccess ? 1 : -1, std::memory_order_release);
                }
                if (terr == hipSuccess)
                    terr = hipMemcpyAsync(reinterpret_cast<char*>(e->app.vol.p) + (size_t)tail0 * slice * esz, reinterpret_cast<const char*>(vol_host) + (size_t)tail0 * slice * esz,
                                          (size_t)(n - tail0) * slice * esz, hipMemcpyHostToDevice, e->copy_stream);
                if (terr == hipSuccess) terr = hipEventRecord(e->tail_ready, e->copy_stream);
            }
            if (terr != hipSuccess) e->mid_enqueued.store(-1, std::memory_order_release);
            e->tail_enqueued.store(terr == hipSuccess ? 1 : -1, std::memory_order_release);
            t_tail = ms_since(t_start);
            // (Pinning the caller's array here with hipHostRegister makes the copy back 0.4 ms faster -- tools/host_pin_probe.py -- but an
            // array from the malloc heap shares its first and last page with other objects and with the runtime's own cache of pinned
            // user ranges; one whole-suite run aborted inside the next model load after such a registration, so the pages are touched.)
            if (scratch) {
                memset(out_host, 0, nvox);
            } else if (!out_pinned) {  // (a page-locked block -- lm_host_alloc, what LMInferer hands out -- has no faults to take)
                volatile uint8_t* o = out_host;
                for (size_t i = 0; i < nvox; i += 4096) o[i] = o[i];
                if (nvox) o[nvox - 1] = o[nvox - 1];
            }
            t_touch = ms_since(t_start);
        });
    hipError_t err = hipMemcpyAsync(e->app.vol.p, vol_host, (size_t)(split ? head : n) * slice * esz, hipMemcpyHostToDevice, e->stream);
    const double t_head = ms_since(t_start);
    int rc = LM_OK;
    if (err != hipSuccess) {
        set_error("lm_apply_host: host-to-device copy failed: %s", hipGetErrorString(err));
        rc = LM_ERR_DEVICE;
    } else {
        e->head_slices = split ? head : 0;
        e->mid_slices = split ? mid : 0;
        rc = apply_volume(e, slot, fill_slot, e->app.vol.p, dtype, n, h, w, batch_size, volume_postprocessing, e->app.out.as<uint8_t>());
        e->head_slices = 0;
        e->mid_slices = 0;
    }
    const double t_apply = ms_since(t_start);
    if (threaded) e->helper.wait();
    const double t_join = ms_since(t_start);
    if (rc != LM_OK) {
        // the tail copy may still be reading the caller's volume / writing the staging buffer: nothing of this call may be in
        // flight when it returns
        if (split && e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
        (void)hipStreamSynchronize(e->stream);
        return rc;
    }
    hipError_t back = hipSuccess;
    double t_ext = 0;
    int ext[4] = {0, n, 0, h};
    if (scratch && threaded) {
        // where the labels are: one pass over the result on the device (tens of microseconds), four ints back, then ONE strided copy
        // of rows [y0, y1) of slices [z0, z1) -- whole image rows, so every piece of the copy is (y1 - y0) * w contiguous bytes
        if (e->post.scalars.reserve(4096) != LM_OK) return LM_ERR_ALLOC;
        int* ext_dev = e->post.scalars.as<int>() + 64;
        back = launch_label_extent(e->app.out.as<uint8_t>(), n, h, w, ext_dev, e->stream);
        if (back == hipSuccess) back = hipMemcpyAsync(ext, ext_dev, sizeof ext, hipMemcpyDeviceToHost, e->stream);
        if (back == hipSuccess) back = hipStreamSynchronize(e->stream);
        t_ext = ms_since(t_start);
        if (back == hipSuccess && ext[1] > ext[0] && ext[3] > ext[2]) {
            const size_t off = ((size_t)ext[0] * h + ext[2]) * w;
            back = hipMemcpy2DAsync(out_host + off, slice, e->app.out.as<uint8_t>() + off, slice, (size_t)(ext[3] - ext[2]) * w, (size_t)(ext[1] - ext[0]),
                                    hipMemcpyDeviceToHost, e->stream);
        }
    } else {
        // (without the helper thread nothing was zero-filled: the whole volume is copied)
        back = hipMemcpyAsync(out_host, e->app.out.p, nvox, hipMemcpyDeviceToHost, e->stream);
    }
    if (back == hipSuccess) back = hipStreamSynchronize(e->stream);
    if (back != hipSuccess) {
        set_error("lm_apply_host: device-to-host copy failed: %s", hipGetErrorString(back));
        return LM_ERR_DEVICE;
    }
    if (timing)
        fprintf(stderr, "lm_apply_host: head H2D returned %.2f ms | helper: tail enqueued %.2f, pages %s %.2f | hot path returned %.2f | joined %.2f | extent known %.2f "
                "(slices %d..%d rows %d..%d) | D2H done %.2f ms\n", t_head, t_tail, scratch ? "zeroed" : "touched", t_touch, t_apply, t_join, t_ext, ext[0], ext[1], ext[2], ext[3],
                ms_since(t_start));
    return LM_OK;
}

// ---- volumes queued through one engine (include/lungmask_hip.h: lm_pipe_*) ---------------------------------------------------
static int pipe_init(lm_engine* e) {
    lm_engine::Pipe& q = e->pipe;
    if (q.up_stream) return LM_OK;
    // The two copy streams get the HIGHEST priority class: same-priority streams share a small pool of hardware queues (see
    // lm_engine_create), and a copy that lands on the queue of a forward lane holds that lane's kernels behind its barrier packet
    // for the length of the copy -- measured: +2.9 ms per volume with ordinary streams (profiles/r06e_async_probe.log).  The streams
    // carry nothing but copies, so the priority preempts nobody.
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&q.up_stream, hipStreamNonBlocking, greatest) != hipSuccess ||
        hipStreamCreateWithPriority(&q.out_stream, hipStreamNonBlocking, greatest) != hipSuccess) {
        set_error("lm_pipe: creating the copy streams failed");
        return LM_ERR_DEVICE;
    }
    for (int k = 0; k < 2; ++k)
        if (hipEventCreateWithFlags(&q.uploaded[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&q.done[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&q.copied[k], hipEventDisableTiming) != hipSuccess) {
            set_error("lm_pipe: creating the events failed");
            return LM_ERR_DEVICE;
        }
    return LM_OK;
}

int lm_pipe_upload(lm_engine* e, int k, const void* vol_host, size_t bytes) {
    if (!e || (k != 0 && k != 1) || (!vol_host && bytes)) {
        set_error("lm_pipe_upload: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    LM_TRY(pipe_init(e));
    lm_engine::Pipe& q = e->pipe;
    LM_TRY(q.vol[k].reserve(bytes ? bytes : 16));
    // A pageable source goes through a page-locked staging block of this buffer FIRST (a plain memcpy on this thread, which is why
    // the call has a host thread of its own), then ONE truly asynchronous copy: handing the runtime a pageable pointer makes it stage
    // the data itself, piece by piece, inside calls that the hot path's kernel launches on the other thread then queue behind.
    const void* src = vol_host;
    if (bytes && !host_range_is_pinned(vol_host, bytes)) {
        if (q.staged[k]) LM_HIP(hipEventSynchronize(q.uploaded[k]));  // the previous copy out of this staging block
        if (q.stage[k].reserve(bytes) == LM_OK) {
            memcpy(q.stage[k].p, vol_host, bytes);
            src = q.stage[k].p;
            q.staged[k] = true;
        }  // (no page-locked memory left: the runtime stages it)
    }
    // vol[k] may still be read by the hot path of the volume that used it last: lm_pipe_apply returns without a round trip on the
    // exact-fp32 kernels (no range flag to read back) when there is neither post-processing nor a fill model, so its host return
    // orders nothing on the device.  The copy waits for that volume's hot path here.
    if (q.done_valid[k].load(std::memory_order_acquire)) LM_HIP(hipStreamWaitEvent(q.up_stream, q.done[k], 0));
    if (bytes) LM_HIP(hipMemcpyAsync(q.vol[k].p, src, bytes, hipMemcpyHostToDevice, q.up_stream));
    LM_HIP(hipEventRecord(q.uploaded[k], q.up_stream));
    return LM_OK;
}

int lm_pipe_apply(lm_engine* e, int k, int slot, int fill_slot, int dtype, int n, int h, int w, int batch_size, int volume_postprocessing) {
    if (!e || (k != 0 && k != 1) || n < 0 || h <= 0 || w <= 0) {
        set_error("lm_pipe_apply: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    LM_TRY(pipe_init(e));
    lm_engine::Pipe& q = e->pipe;
    const int esz = dtype == LM_I16 ? 2 : ((dtype == LM_I32 || dtype == LM_F32) ? 4 : ((dtype == LM_I64 || dtype == LM_F64) ? 8 : 0));
    const size_t nvox = (size_t)n * h * w;
    if (!esz || q.vol[k].cap < nvox * esz) {
        set_error("lm_pipe_apply: buffer %d does not hold a volume of this size and dtype (lm_pipe_upload first)", k);
        return LM_ERR_INVALID;
    }
    LM_TRY(q.out[k].reserve(nvox ? nvox : 16));
    // the hot path reads vol[k] behind its copy-in and overwrites out[k] behind the copy-back of the volume that used it last
    LM_HIP(hipStreamWaitEvent(e->stream, q.uploaded[k], 0));
    if (q.copied_valid[k]) LM_HIP(hipStreamWaitEvent(e->stream, q.copied[k], 0));
    const int rc = apply_volume(e, slot, fill_slot, q.vol[k].p, dtype, n, h, w, batch_size, volume_postprocessing, q.out[k].as<uint8_t>());
    // (Also behind a hot path that failed half way: what it did enqueue may read vol[k].  A failure can leave the tail's pre-processing
    // on the copy stream, or a lane, unjoined: the error path waits for them, like lm_apply_host's.)
    if (rc != LM_OK) {
        if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
        if (e->stream2) (void)hipStreamSynchronize(e->stream2);
    }
    LM_HIP(hipEventRecord(q.done[k], e->stream));
    q.done_valid[k].store(true, std::memory_order_release);
    return rc;
}

int lm_pipe_download(lm_engine* e, int k, uint8_t* out_host, size_t bytes) {
    if (!e || (k != 0 && k != 1) || (!out_host && bytes) || !e->pipe.out_stream || e->pipe.out[k].cap < bytes) {
        set_error("lm_pipe_download: bad arguments (lm_pipe_apply first)");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    lm_engine::Pipe& q = e->pipe;
    LM_HIP(hipStreamWaitEvent(q.out_stream, q.done[k], 0));
    if (bytes) LM_HIP(hipMemcpyAsync(out_host, q.out[k].p, bytes, hipMemcpyDeviceToHost, q.out_stream));
    LM_HIP(hipEventRecord(q.copied[k], q.out_stream));
    q.copied_valid[k] = true;
    return LM_OK;
}

int lm_pipe_wait(lm_engine* e, int k) {
    if (!e || (k != 0 && k != 1) || !e->pipe.out_stream) {
        set_error("lm_pipe_wait: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    if (e->pipe.copied_valid[k]) LM_HIP(hipEventSynchronize(e->pipe.copied[k]));
    return LM_OK;
}

int lm_pipe_query(lm_engine* e, int k) {
    if (!e || (k != 0 && k != 1) || !e->pipe.out_stream) {
        set_error("lm_pipe_query: bad arguments");
        return LM_ERR_INVALID;
    }
    LM_DEVICE(e);
    if (!e->pipe.copied_valid[k]) return 1;  // nothing enqueued: nothing to wait for
#ifdef LM_EMU_BUILD
    return 1;  // (the test emulator's streams are synchronous: whatever was enqueued has arrived)
#else
    const hipError_t st = hipEventQuery(e->pipe.copied[k]);
    if (st == hipSuccess) return 1;
    if (st == hipErrorNotReady) {
        (void)hipGetLastError();  // "not ready" is an answer, not an error of ours
        return 0;
    }
    set_error("lm_pipe_query: %s", hipGetErrorString(st));
    return LM_ERR_DEVICE;
#endif
}

int lm_profile_enable(lm_engine* e, int on) {
    if (!e) return LM_ERR_INVALID;
    e->prof.on = on != 0;
    e->prof.per_layer = on == 2 || on == 4;
    e->prof.dominant_only = on == 3;
    e->prof.timeline = on == 4;
    return LM_OK;
}
int lm_profile_timeline(lm_engine* e, lm_launch_span* out, int cap) {
    if (!e) return LM_ERR_INVALID;
    e->prof.collect();
    const int n = (int)e->prof.spans.size();
    for (int i = 0; i < n && i < cap && out; ++i) out[i] = e->prof.spans[i];
    return n;
}
int lm_profile_reset(lm_engine* e) {
    if (!e) return LM_ERR_INVALID;
    e->prof.reset();
    return LM_OK;
}
int lm_profile_read(lm_engine* e, lm_kernel_stat* out, int cap) {
    if (!e) return LM_ERR_INVALID;
    e->prof.collect();
    int n = 0;
    for (auto& kv : e->prof.acc) {
        if (n < cap && out) out[n] = kv.second;
        ++n;
    }
    return n;
}

}  // extern "C"
