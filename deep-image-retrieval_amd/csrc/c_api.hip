// c_api.hip — the extern "C" surface declared in include/dir_engine.h.
// Nothing above this file knows about Python or torch; nothing below it throws.
#include <initializer_list>
#include <new>

#include "engine.h"
#include "pointwise.h"
#include "strip_stream.h"

namespace dir {
const char* last_error();
}
using namespace dir;

// databases at least this long take the split-bf16 similarity kernel (sim_split.hip)
static constexpr int kSimSplitMinRows = 32768;

// dir_op_overflow_word: the device word the per-op 16-bit entry points hand their kernels (null = none, as before the hook
// existed).  Process-wide, not thread-scoped; it never takes part in picking a kernel.
static std::atomic<int*> g_op_ovf{nullptr};
static inline int* op_ovf() { return g_op_ovf.load(std::memory_order_relaxed); }

#define DIR_TRY try {
#define DIR_CATCH                                                   \
    }                                                               \
    catch (const std::bad_alloc&) {                                 \
        return fail(DIR_ERR_NOMEM, "out of host memory");           \
    }                                                               \
    catch (const std::exception& ex) {                              \
        return fail(DIR_ERR_INVALID, std::string("exception: ") + ex.what()); \
    }                                                               \
    catch (...) {                                                   \
        return fail(DIR_ERR_INVALID, "unknown exception");          \
    }

extern "C" {

const char* dir_last_error(void) { return last_error(); }
const char* dir_version(void) { return "dir_engine 0.1 gfx950"; }

int64_t dir_launch_max_threads(void) { return (int64_t)kMaxLaunchThreads; }

int dir_reload_env(void) {
    dir::reload_env();
    return DIR_OK;
}

int dir_op_overflow_word(int* device_word) {
    g_op_ovf.store(device_word, std::memory_order_relaxed);
    return DIR_OK;
}

int dir_engine_create(const dir_model_desc* desc, int device, dir_engine** out) {
    DIR_TRY
    if (!desc || !out) return fail(DIR_ERR_INVALID, "create: null argument");
    if (desc->pooling < DIR_POOL_GEM || desc->pooling > DIR_POOL_AVG)
        return fail(DIR_ERR_INVALID, "create: bad pooling mode");  // ValueError(pooling), rmac_resnet.py:31
    if (!desc->without_fc && desc->out_dim <= 0) return fail(DIR_ERR_INVALID, "create: out_dim <= 0");
    if (desc->head < DIR_HEAD_RMAC || desc->head > DIR_HEAD_CLASSIFIER)
        return fail(DIR_ERR_INVALID, "create: bad head");
    if ((desc->head == DIR_HEAD_FPN || desc->head == DIR_HEAD_FPN0) && desc->pooling != DIR_POOL_GEM)
        // the reference only builds adpoolx5/adpoolc4 for 'gem' (rmac_resnet_fpn.py:39-45)
        return fail(DIR_ERR_INVALID, "create: the FPN heads exist for GeM pooling only");
    if (desc->head == DIR_HEAD_CLASSIFIER && desc->without_fc)
        return fail(DIR_ERR_INVALID, "create: the classifier head needs its FC");
    int ndev = 0;
    DIR_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(DIR_ERR_INVALID, "create: no such device");
    dir_engine* e = new dir_engine();
    e->desc = *desc;
    e->device = device;
    e->sw = dir::env();   // the A/B switches as they stand now; forward() never reads the environment
    int rc = e->build_graph();
    if (rc != DIR_OK) {
        delete e;
        return rc;
    }
    *out = e;
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_destroy(dir_engine* e) {
    DIR_TRY
    if (!e) return DIR_OK;
    e->release();
    for (ProfSlot& s : e->prof) {
        (void)hipEventDestroy(s.start);
        (void)hipEventDestroy(s.stop);
    }
    delete e;
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_set_tensor(dir_engine* e, const char* key, const float* data, const int64_t* shape,
                          int ndim) {
    DIR_TRY
    if (!e || !key || !data || ndim < 0 || (ndim > 0 && !shape))
        return fail(DIR_ERR_INVALID, "set_tensor: null argument");
    std::string k(key);
    if (k.rfind("module.", 0) == 0) k = k.substr(7);  // DataParallel prefix, common.py:128-131
    if (k.size() >= 19 && k.compare(k.size() - 19, 19, "num_batches_tracked") == 0) return DIR_OK;
    HostTensor t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return fail(DIR_ERR_INVALID, "set_tensor: negative dimension");
        t.shape.push_back(shape[i]);
        n *= shape[i];
    }
    t.data.assign(data, data + n);
    e->state[k] = std::move(t);
    e->finalized = false;
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_finalize(dir_engine* e, int dtype) {
    DIR_TRY
    if (!e) return fail(DIR_ERR_INVALID, "finalize: null engine");
    return e->finalize(dtype);
    DIR_CATCH
}

int dir_engine_out_dim(const dir_engine* e, int* out_dim) {
    if (!e || !out_dim) return fail(DIR_ERR_INVALID, "out_dim: null argument");
    *out_dim = e->desc.without_fc ? e->head_dim : e->desc.out_dim;
    return DIR_OK;
}

int dir_workspace_bytes(const dir_engine* e, int B, int H, int W, size_t* bytes) {
    DIR_TRY
    if (!e || !bytes) return fail(DIR_ERR_INVALID, "workspace_bytes: null argument");
    Plan p;
    DIR_CHECK(e->plan(B, H, W, &p));
    *bytes = p.total;
    return DIR_OK;
    DIR_CATCH
}

int dir_forward(dir_engine* e, const void* img, int B, int H, int W, int fmt, float* desc_out,
                void* ws, size_t ws_bytes, void* stream) {
    DIR_TRY
    if (!e || !img || !desc_out) return fail(DIR_ERR_INVALID, "forward: null argument");
    return e->forward(img, B, H, W, fmt, desc_out, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes,
                      (hipStream_t)stream);
    DIR_CATCH
}

int dir_conv_bn_act_f32(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int H,
                        int W, int Cin, int Cout, int R, int S, int stride, int pad, int OH, int OW, int relu,
                        void* stream) {
    DIR_TRY
    if (!x || !w || !bias || !y) return fail(DIR_ERR_INVALID, "conv_bn_act_f32: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0 || pad < 0)
        return fail(DIR_ERR_INVALID, "conv_bn_act_f32: bad dimension");     // (before the geometry check divides by stride)
    if (OH != (H + 2 * pad - R) / stride + 1 || OW != (W + 2 * pad - S) / stride + 1)
        return fail(DIR_ERR_INVALID, "conv_bn_act_f32: OH/OW do not match the conv geometry");
    ConvF32Args a;
    conv_geom_fill(a, {B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu}, x, w, bias, res, y);
    return conv_f32_launch(a, (hipStream_t)stream);
    DIR_CATCH
}

// The fp32 twins of dir_prep_input / dir_maxpool_3x3s2 / dir_global_pool / dir_upsample_add (conv_f32.hip): the same
// checks and argument order, no dtype.
int dir_prep_input_f32(const void* img, int fmt, const float* mean3, const float* std3, float* out, int B, int H, int W,
                       void* stream) {
    DIR_TRY
    if (!img || !out || B <= 0 || H <= 0 || W <= 0) return fail(DIR_ERR_INVALID, "prep_input: bad argument");
    return prep_input_f32(img, fmt, mean3, std3, out, B, H, W, (hipStream_t)stream);
    DIR_CATCH
}

int dir_maxpool_3x3s2_f32(const float* x, float* y, int B, int H, int W, int C, void* stream) {
    DIR_TRY
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(DIR_ERR_INVALID, "maxpool: bad argument");
    return maxpool_3x3s2_f32(x, y, B, H, W, C, (hipStream_t)stream);
    DIR_CATCH
}

int dir_global_pool_f32(const float* x, float* out, int B, int H, int W, int C, int pooling, float p, float eps,
                        float center_bias, void* stream) {
    DIR_TRY
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(DIR_ERR_INVALID, "global_pool: bad argument");
    return global_pool_f32(x, out, C, B, H, W, C, pooling, p, eps, center_bias, (hipStream_t)stream);
    DIR_CATCH
}

int dir_upsample_add_f32(const float* x, const float* low, float* y, int B, int H, int W, int h, int w, int C,
                         void* stream) {
    DIR_TRY
    if (!x || !low || !y || B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || C <= 0)
        return fail(DIR_ERR_INVALID, "upsample_add: bad argument");
    return upsample_add_f32(x, low, y, B, H, W, h, w, C, (hipStream_t)stream);
    DIR_CATCH
}

int dir_conv_bn_act_pair(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias,
                         const void* res_hi, const void* res_lo, void* y_hi, void* y_lo, int B, int H, int W, int Cin,
                         int Cout, int R, int S, int stride, int pad, int OH, int OW, int relu, void* stream) {
    DIR_TRY
    if (!x_hi || !w_hi || !w_lo || !bias || !y_hi) return fail(DIR_ERR_INVALID, "conv_bn_act_pair: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0 || pad < 0)
        return fail(DIR_ERR_INVALID, "conv_bn_act_pair: bad dimension");
    if (OH != (H + 2 * pad - R) / stride + 1 || OW != (W + 2 * pad - S) / stride + 1 || OH <= 0 || OW <= 0)
        return fail(DIR_ERR_INVALID, "conv_bn_act_pair: OH/OW do not match the conv geometry");
    ConvArgs a;
    conv_args_init(a, {B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu ? 1 : 0}, (const uint16_t*)x_hi, (const uint16_t*)w_hi,
                   bias, (const uint16_t*)res_hi, (uint16_t*)y_hi);
    a.x_lo = (const uint16_t*)x_lo;
    a.w_lo = (const uint16_t*)w_lo;
    a.res_lo = (const uint16_t*)res_lo;
    a.y_lo = (uint16_t*)y_lo;
    a.ovf = op_ovf();
    return conv_pair_launch(a, (hipStream_t)stream);
    DIR_CATCH
}

int dir_conv_pair_dual(const void* t2_hi, const void* t2_lo, const void* x_hi, const void* x_lo, const void* wcat_hi,
                       const void* wcat_lo, const float* bias, void* y_hi, void* y_lo, int B, int H, int W, int Cin,
                       int Cout, int relu, void* stream) {
    DIR_TRY
    if (!t2_hi || !t2_lo || !x_hi || !x_lo || !wcat_hi || !wcat_lo || !bias || !y_hi)
        return fail(DIR_ERR_INVALID, "conv_pair_dual: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail(DIR_ERR_INVALID, "conv_pair_dual: bad dimension");
    ConvArgs a;
    conv_args_init(a, {B, H, W, Cin, Cout, 1, 1, 1, 0, H, W, relu ? 1 : 0}, (const uint16_t*)t2_hi, (const uint16_t*)wcat_hi, bias,
                   nullptr, (uint16_t*)y_hi);
    a.x_lo = (const uint16_t*)t2_lo;
    a.w_lo = (const uint16_t*)wcat_lo;
    a.y_lo = (uint16_t*)y_lo;
    conv_args_second_source(a, (const uint16_t*)x_hi, (const uint16_t*)x_lo, Cin);
    a.ovf = op_ovf();
    return conv_pair_launch(a, (hipStream_t)stream);
    DIR_CATCH
}

int dir_prep_input_pair(const void* img, int img_format, const float* mean3, const float* std3, void* out_hi,
                        void* out_lo, int B, int H, int W, void* stream) {
    DIR_TRY
    if (B <= 0 || H <= 0 || W <= 0) return fail(DIR_ERR_INVALID, "prep_input_pair: bad dimension");
    return prep_input_pair(img, img_format, mean3, std3, out_hi, out_lo, B, H, W, (hipStream_t)stream);
    DIR_CATCH
}

int dir_stem_pool_pair(const void* s2d_hi, const void* s2d_lo, const void* w_hi, const void* w_lo, const float* bias,
                       void* y_hi, void* y_lo, int B, int H2, int W2, int OH, int OW, void* stream) {
    DIR_TRY
    if (!s2d_hi || !s2d_lo || !w_hi || !w_lo || !bias || !y_hi || !y_lo) return fail(DIR_ERR_INVALID, "stem_pool_pair: null pointer");
    if (B <= 0 || H2 <= 0 || W2 <= 0 || OH <= 0 || OW <= 0) return fail(DIR_ERR_INVALID, "stem_pool_pair: bad dimension");
    // the 7x7 s2 p3 conv of an H x W image has (H - 1) / 2 + 1 = (H + 1) / 2 output rows - the rows of its space-to-depth
    // grid, for even and odd H alike; any other OH / OW would size the grid and the stores beyond the caller's buffers
    if (OH != H2 || OW != W2)
        return fail(DIR_ERR_INVALID, "stem_pool_pair: OH x OW must equal the space-to-depth grid H2 x W2 (conv 7x7 s2 p3)");
    return stem_pool_pair_launch(s2d_hi, s2d_lo, w_hi, w_lo, bias, y_hi, y_lo, B, H2, W2, OH, OW, (hipStream_t)stream,
                                 op_ovf());
    DIR_CATCH
}

int dir_stem_pool_u8(const void* img_u8, const float* w_oihw, const float* bn_scale, const float* bn_bias, const float* mean3,
                     const float* std3, void* s2d_ws, void* y_hi, void* y_lo, int B, int H, int W, int seg_tiles, void* stream) {
    DIR_TRY
    if (!img_u8 || !w_oihw || !bn_scale || !bn_bias || !mean3 || !std3 || !s2d_ws || !y_hi || !y_lo)
        return fail(DIR_ERR_INVALID, "stem_pool_u8: null pointer");
    if (B <= 0 || H < 7 || W < 7) return fail(DIR_ERR_INVALID, "stem_pool_u8: bad dimension (the image must hold the 7x7 filter)");
    std::vector<uint16_t> hi, lo;
    std::vector<float> b2, corr;
    DIR_CHECK(fold_stem_u8(w_oihw, bn_scale, bn_bias, mean3, std3, hi, lo, b2, corr));
    // (a per-call upload: this is the parity entry point; the engine folds once at finalize and keeps the tables)
    char* d = nullptr;
    const size_t nw = hi.size() * 2, nb = b2.size() * 4, nc = corr.size() * 4;
    DIR_HIP_CHECK(hipMalloc((void**)&d, 2 * nw + nb + nc));
    hipError_t e = hipMemcpy(d, hi.data(), nw, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + nw, lo.data(), nw, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * nw, b2.data(), nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * nw + nb, corr.data(), nc, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(DIR_ERR_HIP, std::string("stem_pool_u8 upload: ") + hipGetErrorString(e));
    }
    const bool raw = stem_pool_u8_raw_ok(img_u8, B, H, W);
    int rc = raw ? DIR_OK : prep_input_u8(img_u8, s2d_ws, B, H, W, (hipStream_t)stream);
    if (rc == DIR_OK)
        rc = stem_pool_u8_launch(raw ? img_u8 : nullptr, s2d_ws, d, d + nw, (const float*)(d + 2 * nw), (const float*)(d + 2 * nw + nb), y_hi, y_lo, B, H, W,
                                 (hipStream_t)stream, op_ovf(), seg_tiles);
    e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d);
    if (rc != DIR_OK) return rc;
    if (e != hipSuccess) return fail(DIR_ERR_HIP, std::string("stem_pool_u8: ") + hipGetErrorString(e));
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_overflow(dir_engine* e, void* stream, int* overflowed) {
    DIR_TRY
    if (!e || !overflowed) return fail(DIR_ERR_INVALID, "overflow: null argument");
    return e->overflow((hipStream_t)stream, overflowed);
    DIR_CATCH
}

int dir_forward_features(dir_engine* e, const void* img, int B, int H, int W, int fmt,
                         void* feat_out, int* h, int* w, int* c, void* ws, size_t ws_bytes,
                         void* stream) {
    DIR_TRY
    if (!e || !img || !feat_out) return fail(DIR_ERR_INVALID, "forward_features: null argument");
    return e->forward(img, B, H, W, fmt, nullptr, feat_out, h, w, c, ws, ws_bytes,
                      (hipStream_t)stream);
    DIR_CATCH
}

int dir_engine_autotune(dir_engine* e, int B, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    DIR_TRY
    if (!e) return fail(DIR_ERR_INVALID, "autotune: null engine");
    if (e->dtype == DIR_F32) return DIR_OK;   // the strict path has one kernel per conv: nothing to choose
    const bool was_prof = e->profiling;
    e->profiling = false;
    e->tuning = true;
    int rc = e->forward(nullptr, B, H, W, DIR_IMG_F32_NCHW, nullptr, nullptr, nullptr, nullptr,
                        nullptr, ws, ws_bytes, (hipStream_t)stream);
    e->tuning = false;
    e->profiling = was_prof;
    if (rc != DIR_OK) return rc;
    DIR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_tuning_export(const dir_engine* e, char* buf, size_t cap, size_t* needed) {
    DIR_TRY
    if (!e || !needed) return fail(DIR_ERR_INVALID, "tuning_export: null argument");
    std::string out;
    for (const ConvLayer& L : e->convs)
        for (const auto& kv : L.tuned)
            out += L.name + " " + std::to_string(kv.first) + " " + conv_variant(kv.second).name + "\n";
    *needed = out.size() + 1;
    if (buf && cap >= out.size() + 1) memcpy(buf, out.c_str(), out.size() + 1);
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_tuning_import(dir_engine* e, const char* text) {
    DIR_TRY
    if (!e || !text) return fail(DIR_ERR_INVALID, "tuning_import: null argument");
    std::string s(text);
    size_t pos = 0;
    while (pos < s.size()) {
        size_t eol = s.find('\n', pos);
        if (eol == std::string::npos) eol = s.size();
        const std::string line = s.substr(pos, eol - pos);
        pos = eol + 1;
        if (line.empty()) continue;
        const size_t a = line.find(' '), b = line.rfind(' ');
        if (a == std::string::npos || b == a) return fail(DIR_ERR_INVALID, "tuning_import: bad line: " + line);
        const std::string lname = line.substr(0, a), vname = line.substr(b + 1);
        const long M = atol(line.substr(a + 1, b - a - 1).c_str());
        int variant = -1;
        for (int v = 0; v < conv_variant_count(); ++v)
            if (vname == conv_variant(v).name) variant = v;
        if (variant < 0) continue;   // a variant this build no longer has: fall back to the heuristic
        for (ConvLayer& L : e->convs)
            if (L.name == lname) L.tuned[M] = variant;
    }
    return DIR_OK;
    DIR_CATCH
}

int dir_engine_set_profiling(dir_engine* e, int enabled) {
    if (!e) return fail(DIR_ERR_INVALID, "set_profiling: null engine");
    e->profiling = enabled != 0;
    e->prof_paused = false;
    e->prof_used = 0;
    // enabled > 1: pre-create that many event pairs so none is created inside a timed region
    while ((int)e->prof.size() < enabled && enabled > 1) {
        ProfSlot s;
        DIR_HIP_CHECK(hipEventCreate(&s.start));
        DIR_HIP_CHECK(hipEventCreate(&s.stop));
        e->prof.push_back(s);
    }
    return DIR_OK;
}

int dir_engine_profile_pause(dir_engine* e, int paused) {
    if (!e) return fail(DIR_ERR_INVALID, "profile_pause: null engine");
    e->prof_paused = paused != 0;
    return DIR_OK;
}

int dir_engine_get_profile(dir_engine* e, dir_prof_record* out, int cap, int* n) {
    DIR_TRY
    if (!e || !n) return fail(DIR_ERR_INVALID, "get_profile: null argument");
    const int have = (int)e->prof_used;
    for (int i = 0; i < have; ++i) {
        ProfSlot& s = e->prof[i];
        DIR_HIP_CHECK(hipEventSynchronize(s.stop));
        if (out && i < cap) {
            float ms = 0.f;
            DIR_HIP_CHECK(hipEventElapsedTime(&ms, s.start, s.stop));
            dir_prof_record& r = out[i];
            memset(&r, 0, sizeof(r));
            strncpy(r.name, s.name.c_str(), sizeof(r.name) - 1);
            strncpy(r.kernel, s.kernel.c_str(), sizeof(r.kernel) - 1);
            r.flops = s.flops;
            r.bytes = s.bytes;
            r.ms = ms;
        }
    }
    *n = have;
    e->prof_used = 0;
    return DIR_OK;
    DIR_CATCH
}

// ---- per-op entry points --------------------------------------------------------------------------
int dir_conv_variant_count(void) { return conv_variant_count(); }
int dir_conv_variant_name(int variant, char* buf, int cap) {
    if (variant < 0 || variant >= conv_variant_count() || !buf || cap <= 0)
        return fail(DIR_ERR_INVALID, "variant_name: bad argument");
    strncpy(buf, conv_variant(variant).name, cap - 1);
    buf[cap - 1] = 0;
    return DIR_OK;
}

// Validates the arguments every 16-bit per-op conv shares and builds its ConvArgs (partial stays null here; ovf is the
// word of dir_op_overflow_word, null unless a host set one).
static int fill_conv_args(ConvArgs& a, const void* x, const void* w, const float* bias,
                          const void* res, void* y, int B, int H, int W, int Cin, int Cout, int R,
                          int S, int stride, int pad, int OH, int OW, int relu) {
    if (!x || !w || !bias || !y) return fail(DIR_ERR_INVALID, "conv: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0 ||
        pad < 0 || OH <= 0 || OW <= 0)
        return fail(DIR_ERR_INVALID, "conv: bad dimension");
    conv_args_init(a, {B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu ? 1 : 0}, (const uint16_t*)x, (const uint16_t*)w, bias,
                   (const uint16_t*)res, (uint16_t*)y);
    a.ovf = op_ovf();
    return DIR_OK;
}

// The shape-only queries below decide on the host: their ConvArgs carries pointers that only have to be non-null (never dereferenced).
static int shape_only_conv_args(ConvArgs& a, int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int OH,
                                int OW, int has_residual) {
    static const float dummy = 0.f;
    return fill_conv_args(a, &dummy, &dummy, &dummy, has_residual ? &dummy : nullptr, (void*)&dummy, B, H, W, Cin, Cout, R, S,
                          stride, pad, OH, OW, 1);
}

int dir_conv_heuristic(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int OH,
                       int OW, int has_residual, char* name, int cap, int* ksplit) {
    DIR_TRY
    if (!name || cap <= 0) return fail(DIR_ERR_INVALID, "conv_heuristic: null name buffer");
    ConvArgs a;
    DIR_CHECK(shape_only_conv_args(a, B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, has_residual));
    const int v = conv_pick_variant(a);
    if (v < 0) return fail(DIR_ERR_INVALID, "conv_heuristic: no admissible variant for this shape");
    strncpy(name, conv_variant(v).name, cap - 1);
    name[cap - 1] = 0;
    if (ksplit) *ksplit = conv_splitk_factor(v, a);
    return DIR_OK;
    DIR_CATCH
}

int dir_conv_variant_admissible(int variant, int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                int OH, int OW, int has_residual, int* admissible) {
    DIR_TRY
    if (!admissible) return fail(DIR_ERR_INVALID, "conv_variant_admissible: null result pointer");
    if (variant < 0 || variant >= conv_variant_count()) return fail(DIR_ERR_INVALID, "conv_variant_admissible: no such variant");
    ConvArgs a;
    DIR_CHECK(shape_only_conv_args(a, B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, has_residual));
    *admissible = conv_variant_admissible(variant, a) ? 1 : 0;
    return DIR_OK;
    DIR_CATCH
}

int dir_conv_variant_splitk(int variant, int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                            int OH, int OW, int has_residual, int* ksplit) {
    DIR_TRY
    if (!ksplit) return fail(DIR_ERR_INVALID, "conv_variant_splitk: null result pointer");
    ConvArgs a;
    DIR_CHECK(shape_only_conv_args(a, B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, has_residual));
    if (!conv_variant_admissible(variant, a)) return fail(DIR_ERR_INVALID, "conv_variant_splitk: variant not admissible for this shape");
    const int s = conv_splitk_factor(variant, a);
    *ksplit = s > 1 ? s : 1;
    return DIR_OK;
    DIR_CATCH
}

int dir_conv_bn_act(const void* x, const void* w, const float* bias, const void* res, void* y,
                    int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                    int OH, int OW, int relu, int dtype, int variant, void* stream) {
    DIR_TRY
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, x, w, bias, res, y, B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu));
    return conv_launch(a, dtype, variant, (hipStream_t)stream);
    DIR_CATCH
}

int dir_conv_bn_act_splitk(const void* x, const void* w, const float* bias, const void* res, void* y,
                           int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                           int OH, int OW, int relu, int dtype, int variant, int ksplit, void* scratch,
                           size_t scratch_bytes, int* ksplit_used, void* stream) {
    DIR_TRY
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, x, w, bias, res, y, B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu));
    if (variant < 0) variant = conv_pick_variant(a);
    a.ksplit = ksplit < 0 ? conv_splitk_factor(variant, a) : ksplit;
    a.partial = (float*)scratch;
    if (a.ksplit > 1 && conv_splitk_bytes(a, a.ksplit) > scratch_bytes)
        return fail(DIR_ERR_WORKSPACE, "conv: split-K scratch too small");
    if (ksplit_used) *ksplit_used = a.ksplit > 1 ? a.ksplit : 1;
    return conv_launch(a, dtype, variant, (hipStream_t)stream);
    DIR_CATCH
}

// How the four seam entry points end: every tensor 16-byte aligned, then the launch, its hipError_t mapped to a dir_status.
static int launch_c3c1(const char* who, const ConvArgs& a, int dtype, void* stream, std::initializer_list<const void*> tensors) {
    for (const void* q : tensors)
        if ((uintptr_t)q & 15) return fail(DIR_ERR_INVALID, std::string(who) + ": tensors must be 16-byte aligned");
    hipError_t e = conv_c3c1_launch(a, dtype, (hipStream_t)stream);
    if (e != hipSuccess) return fail(DIR_ERR_HIP, std::string(who) + " launch: " + hipGetErrorString(e));
    return DIR_OK;
}

// (keep_stride: ConvArgs::y_keep_stride - 0 from the plain entry points, the caller's from the _keep ones)
static int conv_c3c1_entry(const void* t2, const void* w3, const float* bias3, const void* res, void* y, const void* w1,
                           const float* bias1, void* t1, int B, int H, int W, int P, int P2, int relu3, int relu1,
                           int keep_stride, int dtype, void* stream) {
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, t2, w3, bias3, res, y, B, H, W, P, 4 * P, 1, 1, 1, 0, H, W, relu3));
    if (!w1 || !bias1 || !t1 || !res) return fail(DIR_ERR_INVALID, "conv_c3c1: null pointer");
    if (dtype != DIR_BF16 && dtype != DIR_FP16) return fail(DIR_ERR_INVALID, "conv_c3c1: bad dtype");
    if (keep_stride < 0) return fail(DIR_ERR_INVALID, "conv_c3c1: negative keep_stride");
    conv_args_next_conv1(a, (const uint16_t*)w1, nullptr, bias1, (uint16_t*)t1, P2, relu1 ? 1 : 0);
    a.y_keep_stride = keep_stride;
    if (!conv_c3c1_admissible(a))
        return fail(DIR_ERR_INVALID, "conv_c3c1: planes must be 64, 128 (P2 = P, or 128 after 64) or 256 (P2 = 256, B*H*W % 64 == 0; no keep_stride)");
    return launch_c3c1("conv_c3c1", a, dtype, stream, {t2, w3, res, y, w1, t1, bias3, bias1});
}

int dir_conv_c3c1(const void* t2, const void* w3, const float* bias3, const void* res, void* y, const void* w1,
                  const float* bias1, void* t1, int B, int H, int W, int P, int P2, int relu3, int relu1, int dtype,
                  void* stream) {
    DIR_TRY
    return conv_c3c1_entry(t2, w3, bias3, res, y, w1, bias1, t1, B, H, W, P, P2, relu3, relu1, 0, dtype, stream);
    DIR_CATCH
}

int dir_conv_c3c1_keep(const void* t2, const void* w3, const float* bias3, const void* res, void* y, const void* w1,
                       const float* bias1, void* t1, int B, int H, int W, int P, int P2, int relu3, int relu1,
                       int keep_stride, int dtype, void* stream) {
    DIR_TRY
    return conv_c3c1_entry(t2, w3, bias3, res, y, w1, bias1, t1, B, H, W, P, P2, relu3, relu1, keep_stride, dtype, stream);
    DIR_CATCH
}

int dir_conv_c3c1_ds(const void* t2, const void* x, const void* wcat, const float* bias, void* y, const void* w1,
                     const float* bias1, void* t1, int B, int H, int W, int relu3, int relu1, int dtype,
                     void* stream) {
    DIR_TRY
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, t2, wcat, bias, nullptr, y, B, H, W, 64, 256, 1, 1, 1, 0, H, W, relu3));
    if (!x || !w1 || !bias1 || !t1) return fail(DIR_ERR_INVALID, "conv_c3c1_ds: null pointer");
    if (dtype != DIR_BF16 && dtype != DIR_FP16) return fail(DIR_ERR_INVALID, "conv_c3c1_ds: bad dtype");
    a.x2 = (const uint16_t*)x;
    a.Cin2 = 64;
    conv_args_next_conv1(a, (const uint16_t*)w1, nullptr, bias1, (uint16_t*)t1, 64, relu1 ? 1 : 0);
    if (!conv_c3c1_admissible(a)) return fail(DIR_ERR_INVALID, "conv_c3c1_ds: shape not admissible");
    return launch_c3c1("conv_c3c1_ds", a, dtype, stream, {t2, x, wcat, y, w1, t1, bias, bias1});
    DIR_CATCH
}

static int conv_c3c1_wpair_entry(const void* t2, const void* w3, const void* w3_lo, const float* bias3, const void* res, void* y,
                                 const void* w1, const void* w1_lo, const float* bias1, void* t1, int B, int H, int W, int P2,
                                 int relu3, int relu1, int keep_stride, void* stream) {
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, t2, w3, bias3, res, y, B, H, W, 64, 256, 1, 1, 1, 0, H, W, relu3));
    if (!w3_lo || !w1 || !bias1 || !t1 || !res) return fail(DIR_ERR_INVALID, "conv_c3c1_wpair: null pointer");
    if (keep_stride < 0) return fail(DIR_ERR_INVALID, "conv_c3c1_wpair: negative keep_stride");
    a.w_lo = (const uint16_t*)w3_lo;
    conv_args_next_conv1(a, (const uint16_t*)w1, (const uint16_t*)w1_lo, bias1, (uint16_t*)t1, P2, relu1 ? 1 : 0);
    a.y_keep_stride = keep_stride;
    if (!conv_c3c1_admissible(a))
        return fail(DIR_ERR_INVALID, "conv_c3c1_wpair: planes 64; P2 = 64 (w1_lo required) or 128 (w1_lo optional)");
    return launch_c3c1("conv_c3c1_wpair", a, DIR_FP16, stream, {t2, w3, w3_lo, res, y, w1, w1_lo, t1, bias3, bias1});
}

int dir_conv_c3c1_wpair(const void* t2, const void* w3, const void* w3_lo, const float* bias3, const void* res, void* y,
                        const void* w1, const void* w1_lo, const float* bias1, void* t1, int B, int H, int W, int P2,
                        int relu3, int relu1, void* stream) {
    DIR_TRY
    return conv_c3c1_wpair_entry(t2, w3, w3_lo, bias3, res, y, w1, w1_lo, bias1, t1, B, H, W, P2, relu3, relu1, 0, stream);
    DIR_CATCH
}

int dir_conv_c3c1_wpair_keep(const void* t2, const void* w3, const void* w3_lo, const float* bias3, const void* res, void* y,
                             const void* w1, const void* w1_lo, const float* bias1, void* t1, int B, int H, int W, int P2,
                             int relu3, int relu1, int keep_stride, void* stream) {
    DIR_TRY
    return conv_c3c1_wpair_entry(t2, w3, w3_lo, bias3, res, y, w1, w1_lo, bias1, t1, B, H, W, P2, relu3, relu1, keep_stride,
                                 stream);
    DIR_CATCH
}

int dir_conv_c3c1_ds_wpair(const void* t2, const void* x, const void* x_lo, const void* wcat, const void* wcat_lo,
                           const float* bias, void* y, const void* w1, const void* w1_lo, const float* bias1, void* t1,
                           int B, int H, int W, int relu3, int relu1, void* stream) {
    DIR_TRY
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, t2, wcat, bias, nullptr, y, B, H, W, 64, 256, 1, 1, 1, 0, H, W, relu3));
    if (!x || !x_lo || !wcat_lo || !w1 || !w1_lo || !bias1 || !t1) return fail(DIR_ERR_INVALID, "conv_c3c1_ds_wpair: null pointer");
    a.x2 = (const uint16_t*)x;
    a.x2_lo = (const uint16_t*)x_lo;
    a.Cin2 = 64;
    a.w_lo = (const uint16_t*)wcat_lo;
    conv_args_next_conv1(a, (const uint16_t*)w1, (const uint16_t*)w1_lo, bias1, (uint16_t*)t1, 64, relu1 ? 1 : 0);
    if (!conv_c3c1_admissible(a)) return fail(DIR_ERR_INVALID, "conv_c3c1_ds_wpair: shape not admissible");
    return launch_c3c1("conv_c3c1_ds_wpair", a, DIR_FP16, stream, {t2, x, x_lo, wcat, wcat_lo, y, w1, w1_lo, t1, bias, bias1});
    DIR_CATCH
}

int dir_conv_dual(const void* t2, const void* x, const void* wcat, const float* bias, void* y, int B, int OH, int OW,
                  int Cin, int Cout, int Cin2, int H2, int W2, int stride2, int relu, int dtype, void* stream) {
    DIR_TRY
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, t2, wcat, bias, nullptr, y, B, OH, OW, Cin, Cout, 1, 1, 1, 0, OH, OW, relu));
    if (!x || Cin2 <= 0 || H2 <= 0 || W2 <= 0 || stride2 <= 0) return fail(DIR_ERR_INVALID, "conv_dual: bad argument");
    if ((OH - 1) * stride2 >= H2 || (OW - 1) * stride2 >= W2)
        return fail(DIR_ERR_INVALID, "conv_dual: the strided pixel map leaves the second source");
    if (Cin % 64 || Cin2 % 64) return fail(DIR_ERR_INVALID, "conv_dual: channel counts must be multiples of 64");
    conv_args_second_source(a, (const uint16_t*)x, nullptr, Cin2);
    a.H2 = H2;
    a.W2 = W2;
    a.stride2 = stride2;
    if (((uintptr_t)t2 & 15) || ((uintptr_t)wcat & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15))
        return fail(DIR_ERR_INVALID, "conv_dual: tensors must be 16-byte aligned");
    if ((long)a.M * Cout >= (1L << 30) || (long)a.M * Cin >= (1L << 30))
        return fail(DIR_ERR_INVALID, "conv_dual: tensor exceeds 2^31 bytes; lower the batch");
    if (dtype != DIR_BF16 && dtype != DIR_FP16) return fail(DIR_ERR_INVALID, "conv_dual: bad dtype");
    // (small shapes included: the op-level entry point runs the form wherever the tile divides Cout)
    // what the engine runs at batch size: the persistent two-source ring (conv_persist.hip DUAL)
    const int variant = conv_pick_dual_variant(a, true);
    if (variant < 0) return fail(DIR_ERR_INVALID, "conv_dual: Cout must be a multiple of 256");
    return conv_launch(a, dtype, variant, (hipStream_t)stream);
    DIR_CATCH
}

int dir_conv_bn_act_naive(const void* x, const void* w, const float* bias, const void* res, void* y,
                          int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                          int OH, int OW, int relu, int dtype, void* stream) {
    DIR_TRY
    ConvArgs a;
    DIR_CHECK(fill_conv_args(a, x, w, bias, res, y, B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu));
    if (dtype != DIR_BF16 && dtype != DIR_FP16) return fail(DIR_ERR_INVALID, "conv: bad dtype");
    return conv_launch_naive(a, dtype, (hipStream_t)stream);
    DIR_CATCH
}

int dir_prep_input(const void* img, int fmt, const float* mean3, const float* std3, void* out,
                   int B, int H, int W, int dtype, void* stream) {
    DIR_TRY
    if (!img || !out || B <= 0 || H <= 0 || W <= 0) return fail(DIR_ERR_INVALID, "prep_input: bad argument");
    return prep_input(img, fmt, mean3, std3, out, B, H, W, dtype, (hipStream_t)stream);
    DIR_CATCH
}

int dir_stem_pool(const void* s2d, const void* w, const float* bias, void* y, int B, int H2, int W2,
                  int OH, int OW, int dtype, void* stream) {
    DIR_TRY
    if (!s2d || !w || !bias || !y || B <= 0 || H2 <= 0 || W2 <= 0 || OH <= 0 || OW <= 0)
        return fail(DIR_ERR_INVALID, "stem_pool: bad argument");
    if (OH != H2 || OW != W2)   // (conv 7x7 s2 p3: (H - 1) / 2 + 1 == (H + 1) / 2 for every H; see dir_stem_pool_pair)
        return fail(DIR_ERR_INVALID, "stem_pool: OH x OW must equal the space-to-depth grid H2 x W2 (conv 7x7 s2 p3)");
    return stem_pool_launch(s2d, w, bias, y, B, H2, W2, OH, OW, dtype, (hipStream_t)stream, op_ovf());
    DIR_CATCH
}

int dir_maxpool_3x3s2(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
    DIR_TRY
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(DIR_ERR_INVALID, "maxpool: bad argument");
    return maxpool_3x3s2(x, y, B, H, W, C, dtype, (hipStream_t)stream);
    DIR_CATCH
}

int dir_global_pool(const void* x, float* out, int B, int H, int W, int C, int pooling, float p,
                    float eps, float center_bias, int dtype, void* stream) {
    DIR_TRY
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(DIR_ERR_INVALID, "global_pool: bad argument");
    return global_pool(x, out, C, B, H, W, C, pooling, p, eps, center_bias, dtype, (hipStream_t)stream);
    DIR_CATCH
}

int dir_resize_workspace_bytes(int B, int H, int W, int OH, int OW, size_t* bytes) {
    DIR_TRY
    if (!bytes || B <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0)
        return fail(DIR_ERR_INVALID, "resize_workspace_bytes: bad argument");
    *bytes = resize_workspace_bytes(B, H, W, OH, OW);
    return DIR_OK;
    DIR_CATCH
}

int dir_resize_bilinear_u8(const void* src, void* dst, int B, int H, int W, int OH, int OW, void* workspace,
                           size_t workspace_bytes, void* stream) {
    DIR_TRY
    if (!src || !dst || B <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0)
        return fail(DIR_ERR_INVALID, "resize_bilinear_u8: bad argument");
    return resize_bilinear_u8((const uint8_t*)src, (uint8_t*)dst, B, H, W, OH, OW, workspace, workspace_bytes,
                              (hipStream_t)stream);
    DIR_CATCH
}

int dir_upsample_add(const void* x, const void* low, void* y, int B, int H, int W, int h, int w, int C,
                     int dtype, void* stream) {
    DIR_TRY
    if (!x || !low || !y || B <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || C <= 0)
        return fail(DIR_ERR_INVALID, "upsample_add: bad argument");
    return upsample_add(x, low, y, B, H, W, h, w, C, dtype, (hipStream_t)stream, op_ovf());
    DIR_CATCH
}

int dir_l2norm_rows(float* x, int rows, int cols, float eps, void* stream) {
    DIR_TRY
    if (!x || rows < 0 || cols <= 0) return fail(DIR_ERR_INVALID, "l2norm_rows: bad argument");
    return l2norm_rows(x, rows, cols, eps, (hipStream_t)stream);
    DIR_CATCH
}

/* host-only: the number of K slices dir_gemm_nt_f32 runs a shape with (1 = no split) */
int dir_gemm_splitk_factor(int NP, int NQ, int K) { return gemm_splitk_factor(NP, NQ, K); }

int dir_gemm_nt_f32(const float* P, int ldp, const float* Q, int ldq, float* out, int ldo, int NP,
                    int NQ, int K, const float* qsub, const float* bias, const float* alpha,
                    void* stream) {
    DIR_TRY
    if (NP < 0 || NQ < 0) return fail(DIR_ERR_INVALID, "gemm_nt_f32: negative size");
    if (NP == 0 || NQ == 0) return DIR_OK;
    if (!P || !Q || !out) return fail(DIR_ERR_INVALID, "gemm_nt_f32: null pointer");
    if (ldo < NP) return fail(DIR_ERR_INVALID, "gemm_nt_f32: ldo < NP");
    return gemm_nt_f32(P, ldp, Q, ldq, out, ldo, NP, NQ, K, qsub, bias, alpha, (hipStream_t)stream);
    DIR_CATCH
}

/* host-only: R, the rows one fp32 chain of dir_cov_accumulate runs over before it is folded into fp64 */
int dir_cov_chain_rows(void) { return cov_chain_rows(); }

int dir_cov_accumulate(const float* X, int ldx, int N, int D, const float* shift, double* gram, double* sums,
                       void* stream) {
    DIR_TRY
    return cov_accumulate(X, ldx, N, D, shift, gram, sums, (hipStream_t)stream);   // (validates its arguments before any HIP call)
    DIR_CATCH
}

int dir_fc_l2(const float* x, int B, int K, const float* W, const float* b, int D, float* out,
              void* stream) {
    DIR_TRY
    if (!x || !W || !out || B <= 0 || K <= 0 || D <= 0) return fail(DIR_ERR_INVALID, "fc_l2: bad argument");
    DIR_CHECK(gemm_nt_f32(W, K, x, K, out, D, D, B, K, nullptr, b, nullptr, (hipStream_t)stream));
    return l2norm_rows(out, B, D, 1e-12f, (hipStream_t)stream);
    DIR_CATCH
}

static int pca_whiten_impl(const float* X, int N, int D, const float* mean, const float* components, int v, const float* scale,
                           int l2norm, float* out, void* stream, bool unit_range) {
    if (N < 0 || D <= 0 || v <= 0) return fail(DIR_ERR_INVALID, "pca_whiten_l2: bad size");
    if (N == 0) return DIR_OK;
    if (!X || !components || !out) return fail(DIR_ERR_INVALID, "pca_whiten_l2: null pointer");
    int rc = DIR_OK;
    bool done = false;
    // Large sets whose operands the caller knows to be bounded (dir_pca_whiten_l2_unit): two fp16 planes per operand, three
    // plane products on the fp16 matrix cores (sim_split.hip whiten_split) - 8.4 TFLOP of fp32 MFMA chain at config D otherwise
    if (unit_range && !dir::env().sim_exact && N >= kSimSplitMinRows && whiten_split_admissible(X, D, N, D, v)) {
        const size_t bytes = whiten_split_workspace_bytes(v, D);
        void* ws = nullptr;
        if (hipMallocAsync(&ws, bytes, (hipStream_t)stream) == hipSuccess) {
            rc = whiten_split(X, D, N, components, D, v, D, mean, scale, out, v, ws, bytes, (hipStream_t)stream);
            const hipError_t fe = hipFreeAsync(ws, (hipStream_t)stream);
            if (rc != DIR_OK) return rc;
            DIR_HIP_CHECK(fe);
            done = true;
        } else {
            (void)hipGetLastError();   // no memory pool / out of memory: the exact chain below needs no scratch
        }
    }
    if (!done) rc = gemm_nt_f32(components, D, X, D, out, v, v, N, D, mean, nullptr, scale, (hipStream_t)stream);
    if (rc != DIR_OK || !l2norm) return rc;
    return l2norm_rows(out, N, v, 1e-12f, (hipStream_t)stream);
}

int dir_pca_whiten_l2(const float* X, int N, int D, const float* mean, const float* components, int v,
                      const float* scale, int l2norm, float* out, void* stream) {
    DIR_TRY
    return pca_whiten_impl(X, N, D, mean, components, v, scale, l2norm, out, stream, false);
    DIR_CATCH
}

int dir_pca_whiten_l2_unit(const float* X, int N, int D, const float* mean, const float* components, int v,
                           const float* scale, int l2norm, float* out, void* stream) {
    DIR_TRY
    return pca_whiten_impl(X, N, D, mean, components, v, scale, l2norm, out, stream, true);
    DIR_CATCH
}

static int similarity_impl(const float* queries, int Q, const float* database, int N, int D, float* scores, void* stream,
                           bool unit_range) {
    if (Q < 0 || N < 0 || D <= 0) return fail(DIR_ERR_INVALID, "similarity: bad size");
    if (Q == 0 || N == 0) return DIR_OK;
    if (!queries || !database || !scores) return fail(DIR_ERR_INVALID, "similarity: null pointer");
    // Large databases (the 10^6-distractor protocol): three-plane bf16 split on the matrix cores, fp32-accurate
    // products, ~2x the speed of the exact fp32 MFMA chain (sim_split.hip) - or, for operands the caller knows to be
    // bounded (dir_similarity_unit), two fp16 planes and half the products.  Small ones, odd widths and
    // DIRTORCH_AMD_SIM_EXACT=1 keep the k-ordered fmaf chain of gemm_nt_f32.
    const bool exact = dir::env().sim_exact;
    if (!exact && N >= kSimSplitMinRows && similarity_split_admissible(database, D, queries, D, N, Q, D)) {
        const size_t bytes = similarity_split_workspace_bytes(Q, D);
        void* ws = nullptr;
        if (hipMallocAsync(&ws, bytes, (hipStream_t)stream) == hipSuccess) {   // stream-ordered: freed after the kernels
            const int rc = similarity_split(database, D, queries, D, scores, N, N, Q, D, ws, bytes, (hipStream_t)stream,
                                            unit_range);
            const hipError_t fe = hipFreeAsync(ws, (hipStream_t)stream);
            if (rc != DIR_OK) return rc;
            DIR_HIP_CHECK(fe);
            return DIR_OK;
        }
        (void)hipGetLastError();   // no memory pool / out of memory: the exact chain below needs no scratch
    }
    return gemm_nt_f32(database, D, queries, D, scores, N, N, Q, D, nullptr, nullptr, nullptr,
                       (hipStream_t)stream);
}

int dir_similarity(const float* queries, int Q, const float* database, int N, int D, float* scores,
                   void* stream) {
    DIR_TRY
    return similarity_impl(queries, Q, database, N, D, scores, stream, false);
    DIR_CATCH
}

int dir_similarity_unit(const float* queries, int Q, const float* database, int N, int D, float* scores,
                        void* stream) {
    DIR_TRY
    return similarity_impl(queries, Q, database, N, D, scores, stream, true);
    DIR_CATCH
}

int dir_rank_counts(const float* scores, int lds, int Q, int N, const int* probe_idx, int P,
                    int* counts, float* probe_scores, void* stream) {
    DIR_TRY
    if (Q < 0 || N < 0 || P < 0) return fail(DIR_ERR_INVALID, "rank_counts: negative size");
    if (Q == 0 || N == 0 || P == 0) return DIR_OK;
    if (!scores || !probe_idx || !counts || !probe_scores)
        return fail(DIR_ERR_INVALID, "rank_counts: null pointer");
    return rank_counts(scores, lds, Q, N, probe_idx, P, counts, probe_scores, (hipStream_t)stream);
    DIR_CATCH
}

int dir_revisitop_ap(const int* probe_idx, int Q, int P, const int* counts, const float* probe_scores,
                     const int* pos_off, const int* pos_list, const int* junk_off, const int* junk_list,
                     int modes, double* terms, double* ap_out, void* stream) {
    DIR_TRY
    if (Q < 0 || P < 0 || modes < 0) return fail(DIR_ERR_INVALID, "revisitop_ap: negative size");
    if (Q == 0 || modes == 0) return DIR_OK;
    if (!probe_idx || !counts || !probe_scores || !pos_off || !pos_list || !junk_off || !junk_list || !terms ||
        !ap_out)
        return fail(DIR_ERR_INVALID, "revisitop_ap: null pointer");
    return revisitop_ap(probe_idx, Q, P, counts, probe_scores, pos_off, pos_list, junk_off, junk_list, modes,
                        terms, ap_out, (hipStream_t)stream);
    DIR_CATCH
}

int dir_label_rank(const float* scores, int lds, int Q, int N, const int* labels, const int* class_off,
                   const int* class_members, int C, const int* qclass, const int* qself, double* ap, int* best_rank,
                   void* stream) {
    DIR_TRY
    if (Q < 0 || N < 0 || C < 0) return fail(DIR_ERR_INVALID, "label_rank: negative size");
    if (Q == 0) return DIR_OK;
    if (!class_off || !qclass || !qself || !ap || !best_rank || (N > 0 && (!scores || !labels || !class_members)))
        return fail(DIR_ERR_INVALID, "label_rank: null pointer");
    return label_rank(scores, lds, Q, N, labels, class_off, class_members, C, qclass, qself, ap, best_rank,
                      (hipStream_t)stream);
    DIR_CATCH
}

int dir_index_i8_max_dim(void) { return index_i8_max_dim(); }
int dir_index_fp4_max_dim(void) { return index_fp4_max_dim(); }
int dir_index_bin_max_dim(void) { return index_bin_max_dim(); }

// 1 <= D <= the widest row of a code format; max_name: the host query that gives it
static int check_dim(const char* who, int D, int max, const char* max_name) {
    if (D < 1) return fail(DIR_ERR_INVALID, std::string(who) + ": D < 1");
    if (D > max) return fail(DIR_ERR_INVALID, std::string(who) + ": D exceeds " + max_name);
    return DIR_OK;
}
static int index_check_dim(const char* who, int D) { return check_dim(who, D, index_i8_max_dim(), "dir_index_i8_max_dim()"); }
static int fp4_check_dim(const char* who, int D) { return check_dim(who, D, index_fp4_max_dim(), "dir_index_fp4_max_dim()"); }
static int bin_check_dim(const char* who, int D) { return check_dim(who, D, index_bin_max_dim(), "dir_index_bin_max_dim()"); }

extern "C++" {   // (templates: the findings are callables)
// What the entries of the three row quantisers check alike, in one order: the size, D (check_dim), ldx, the pitches of the
// outputs (pitch_error() -> the entry's finding, or null) and - where there are rows - the pointers (null_pointer: one of the
// entry's is missing) and the alignment of the store (align_error() -> the entry's finding, or null).  The two findings are
// callables: they are worked out only behind the D check, so no width is computed from a D out of range.  An empty call
// passes: the launcher returns on it.
template <class Pitch, class Align>
static int quantize_rows_check(const char* who, int (*check_dim)(const char*, int), int N, int D, int ldx, Pitch&& pitch_error,
                               bool null_pointer, Align&& align_error) {
    auto bad = [who](const char* what) { return fail(DIR_ERR_INVALID, std::string(who) + ": " + what); };
    if (N < 0) return bad("negative size");
    DIR_CHECK(check_dim(who, D));
    if (ldx < D) return bad("ldx < D");
    if (const char* what = pitch_error()) return bad(what);
    if (N == 0) return DIR_OK;
    if (null_pointer) return bad("null pointer");
    if (const char* what = align_error()) return bad(what);
    return DIR_OK;
}

// ... and the entries of the three flat scans: the sizes, D, the pitches of the operands, lds and - where there is work - the
// pointers and the admission rule of the scan (admission_error() -> the entry's finding, or null).
template <class Pitch, class Admission>
static int flat_scan_check(const char* who, int (*check_dim)(const char*, int), int Q, int N, int D, int lds, Pitch&& pitch_error,
                           bool null_pointer, Admission&& admission_error) {
    auto bad = [who](const char* what) { return fail(DIR_ERR_INVALID, std::string(who) + ": " + what); };
    if (Q < 0 || N < 0) return bad("negative size");
    DIR_CHECK(check_dim(who, D));
    if (const char* what = pitch_error()) return bad(what);
    if (lds < N) return bad("lds < N");
    if (Q == 0 || N == 0) return DIR_OK;
    if (null_pointer) return bad("null pointer");
    if (const char* what = admission_error()) return bad(what);
    return DIR_OK;
}

}  // extern "C++"

int dir_quantize_rows_i8(const float* X, int ldx, int N, int D, int8_t* codes, int ldc, float* scales, void* stream) {
    DIR_TRY
    DIR_CHECK(quantize_rows_check(
        "quantize_rows_i8", index_check_dim, N, D, ldx,
        [&]() -> const char* { return ldc < pad64(D) ? "ldc < D rounded up to a multiple of 64" : nullptr; },
        !X || !codes || !scales,
        [&]() -> const char* { return (ldc & 3) != 0 || ((uintptr_t)codes & 3) != 0 ? "ldc % 4 == 0 and 4-byte aligned codes" : nullptr; }));
    return quantize_rows_i8(X, ldx, N, D, codes, ldc, scales, (hipStream_t)stream);
    DIR_CATCH
}

int dir_similarity_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                      const float* bscales, int N, int D, float* scores, int lds, void* stream) {
    DIR_TRY
    DIR_CHECK(flat_scan_check(
        "similarity_i8", index_check_dim, Q, N, D, lds,
        [&]() -> const char* {
            return ldq < D ? "ldq < D" : ldb < pad64(D) ? "ldb < D rounded up to a multiple of 64" : nullptr;
        },
        !qcodes || !qscales || !bcodes || !bscales || !scores,
        [&]() -> const char* {
            return similarity_i8_admissible(bcodes, ldb, D) ? nullptr : "ldb % 16 == 0, ldb < 2^23 and 16-byte aligned bcodes";
        }));
    return similarity_i8(qcodes, ldq, qscales, Q, bcodes, ldb, bscales, N, D, scores, lds, (hipStream_t)stream);
    DIR_CATCH
}

int dir_quantize_rows_fp4(const float* X, int ldx, int N, int D, uint8_t* codes, int ldc, uint8_t* exps, int lde,
                          float* scales, void* stream) {
    DIR_TRY
    DIR_CHECK(quantize_rows_check(
        "quantize_rows_fp4", fp4_check_dim, N, D, ldx,
        [&]() -> const char* {
            return ldc < pad64(D) / 2        ? "ldc < half of D rounded up to a multiple of 64"
                   : lde < fp4_exp_bytes(D) ? "lde < 8 * ceil(D / 256)"
                                            : nullptr;
        },
        !X || !codes || !exps || !scales,
        [&]() -> const char* { return (ldc & 1) != 0 || ((uintptr_t)codes & 1) != 0 ? "ldc % 2 == 0 and 2-byte aligned codes" : nullptr; }));
    return quantize_rows_fp4(X, ldx, N, D, codes, ldc, exps, lde, scales, (hipStream_t)stream);
    DIR_CATCH
}

int dir_similarity_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                       const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, int N, int D,
                       float* scores, int lds, void* stream) {
    DIR_TRY
    DIR_CHECK(flat_scan_check(
        "similarity_fp4", fp4_check_dim, Q, N, D, lds,
        [&]() -> const char* {
            return ldq < (D + 1) / 2          ? "ldq < ceil(D / 2)"
                   : ldqe < ceil_div(D, 32)   ? "ldqe < ceil(D / 32)"
                   : ldb < pad64(D) / 2       ? "ldb < half of D rounded up to a multiple of 64"
                   : ldbe < fp4_exp_bytes(D) ? "ldbe < 8 * ceil(D / 256)"
                                              : nullptr;
        },
        !qcodes || !qexps || !qscales || !bcodes || !bexps || !bscales || !scores,
        [&]() -> const char* {
            return similarity_fp4_admissible(bcodes, ldb, bexps, ldbe, D)
                       ? nullptr
                       : "ldb % 16 == 0, ldb < 2^23 and 16-byte aligned bcodes, ldbe % 8 == 0 and 8-byte aligned bexps";
        }));
    return similarity_fp4(qcodes, ldq, qexps, ldqe, qscales, Q, bcodes, ldb, bexps, ldbe, bscales, N, D, scores, lds,
                          (hipStream_t)stream);
    DIR_CATCH
}

int dir_quantize_rows_bin(const float* X, int ldx, int N, int D, uint8_t* bits, int ldb, float* scales, void* stream) {
    DIR_TRY
    DIR_CHECK(quantize_rows_check(
        "quantize_rows_bin", bin_check_dim, N, D, ldx,
        [&]() -> const char* { return ldb < bin_row_bytes(D) ? "ldb < D rounded up to a multiple of 128, divided by 8" : nullptr; },
        !X || !bits || !scales,
        [&]() -> const char* { return (ldb & 3) != 0 || ((uintptr_t)bits & 3) != 0 ? "ldb % 4 == 0 and 4-byte aligned bits" : nullptr; }));
    return quantize_rows_bin(X, ldx, N, D, bits, ldb, scales, (hipStream_t)stream);
    DIR_CATCH
}

int dir_similarity_bin(const int8_t* qcodes, int ldq, const float* qscales, int Q, const uint8_t* bits, int ldb,
                       const float* bscales, int N, int D, float* scores, int lds, void* stream) {
    DIR_TRY
    DIR_CHECK(flat_scan_check(
        "similarity_bin", bin_check_dim, Q, N, D, lds,
        [&]() -> const char* {
            return ldq < D ? "ldq < D" : ldb < bin_row_bytes(D) ? "ldb < D rounded up to a multiple of 128, divided by 8" : nullptr;
        },
        !qcodes || !qscales || !bits || !bscales || !scores,
        [&]() -> const char* { return flat_scan_admissible(bits, ldb) ? nullptr : "ldb % 16 == 0, ldb < 2^23 and 16-byte aligned bits"; }));
    return similarity_bin(qcodes, ldq, qscales, Q, bits, ldb, bscales, N, D, scores, lds, (hipStream_t)stream);
    DIR_CATCH
}

int dir_gather_scores(const float* queries, int ldq, int Q, const float* database, int ldb, int N, int D, const int* cand,
                      int ldcand, int R, float* scores, int ldsc, void* stream) {
    DIR_TRY
    if (Q < 0 || N < 0 || R < 0) return fail(DIR_ERR_INVALID, "gather_scores: negative size");
    if (D < 1) return fail(DIR_ERR_INVALID, "gather_scores: D < 1");
    if (ldq < D || ldb < D) return fail(DIR_ERR_INVALID, "gather_scores: ldq, ldb < D");
    if (ldcand < R || ldsc < R) return fail(DIR_ERR_INVALID, "gather_scores: ldcand, ldsc < R");
    if (Q == 0 || N == 0 || R == 0) return DIR_OK;
    if (!queries || !database || !cand || !scores) return fail(DIR_ERR_INVALID, "gather_scores: null pointer");
    return gather_scores(queries, ldq, Q, database, ldb, D, cand, ldcand, R, scores, ldsc, (hipStream_t)stream);
    DIR_CATCH
}

int dir_segment_sums(const float* X, int ldx, int N, int D, const int* order, const int* seg_off, int S, float* sums,
                     int lds, void* stream) {
    DIR_TRY
    if (N < 0 || S < 0) return fail(DIR_ERR_INVALID, "segment_sums: negative size");
    if (D < 1) return fail(DIR_ERR_INVALID, "segment_sums: D < 1");
    if (ldx < D || lds < D) return fail(DIR_ERR_INVALID, "segment_sums: ldx, lds < D");
    if (S == 0) return DIR_OK;
    if (!seg_off || !sums || (N > 0 && (!X || !order))) return fail(DIR_ERR_INVALID, "segment_sums: null pointer");
    return segment_sums(X, ldx, N, D, order, seg_off, S, sums, lds, (hipStream_t)stream);
    DIR_CATCH
}

// What the entries of the three list-major scans check alike, in one order: the sizes, D (check_dim), the pitches
// (pitch_error: the entry's finding, or null), lds, the outputs, and - where there is work - a list, the inputs (null_input:
// one of the entry's pointers is missing) and the admission rule (admission_error: the entry's finding, or null).  An empty
// call passes: the launcher returns on it.
static int ivf_scan_check(const char* who, int (*check_dim)(const char*, int), int D, int Q, int N, int nlist, int items,
                          int width, int lds, const char* pitch_error, const void* scores, const void* out_ids, bool null_input,
                          const char* admission_error) {
    auto bad = [who](const char* what) { return fail(DIR_ERR_INVALID, std::string(who) + ": " + what); };
    if (Q < 0 || N < 0 || nlist < 0 || items < 0 || width < 0) return bad("negative size");
    DIR_CHECK(check_dim(who, D));
    if (pitch_error) return bad(pitch_error);
    if (lds < width) return bad("lds < width");
    if (Q == 0 || width == 0) return DIR_OK;
    if (!scores || !out_ids) return bad("null pointer");
    if (items > 0 && N > 0) {
        if (nlist < 1) return bad("items without a list");
        if (null_input) return bad("null pointer");
        if (admission_error) return bad(admission_error);
    }
    return DIR_OK;
}

int dir_ivf_scan_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                    const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                    const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                    int lds, int width, void* stream) {
    DIR_TRY
    DIR_CHECK(ivf_scan_check(
        "ivf_scan_i8", index_check_dim, D, Q, N, nlist, items, width, lds,
        ldq < pad64(D) || ldb < pad64(D) ? "ldq, ldb < D rounded up to a multiple of 64" : nullptr, scores, out_ids,
        !qcodes || !qscales || !bcodes || !bscales || !ids || !list_off || !pair_off || !pair_q || !pair_col || !item_off,
        ivf_scan_admissible(qcodes, ldq, Q, bcodes, ldb) ? nullptr
                                                         : "ldq, ldb % 16 == 0, ldb < 2^23, Q * ldq < 2^31 and 16-byte aligned codes"));
    return ivf_scan_i8(qcodes, ldq, qscales, Q, bcodes, ldb, bscales, ids, N, D, list_off, nlist, pair_off, pair_q, pair_col,
                       item_off, items, scores, out_ids, lds, width, (hipStream_t)stream);
    DIR_CATCH
}

int dir_ivf_scan_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                     const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, const int* ids, int N,
                     int D, const int* list_off, int nlist, const int* pair_off, const int* pair_q, const int* pair_col,
                     const int* item_off, int items, float* scores, int* out_ids, int lds, int width, void* stream) {
    DIR_TRY
    DIR_CHECK(ivf_scan_check(
        "ivf_scan_fp4", fp4_check_dim, D, Q, N, nlist, items, width, lds,
        ldq < pad64(D) / 2 || ldb < pad64(D) / 2           ? "ldq, ldb < half of D rounded up to a multiple of 64"
        : ldqe < fp4_exp_bytes(D) || ldbe < fp4_exp_bytes(D) ? "ldqe, ldbe < 8 * ceil(D / 256)"
                                                               : nullptr,
        scores, out_ids,
        !qcodes || !qexps || !qscales || !bcodes || !bexps || !bscales || !ids || !list_off || !pair_off || !pair_q || !pair_col ||
            !item_off,
        ivf_scan_fp4_admissible(qcodes, ldq, qexps, ldqe, Q, bcodes, ldb, bexps, ldbe, D)
            ? nullptr
            : "ldq, ldb % 16 == 0, ldb < 2^23, Q * ldq < 2^31 and 16-byte aligned codes, "
              "ldqe, ldbe % 8 == 0 and 8-byte aligned block bytes"));
    return ivf_scan_fp4(qcodes, ldq, qexps, ldqe, qscales, Q, bcodes, ldb, bexps, ldbe, bscales, ids, N, D, list_off, nlist,
                        pair_off, pair_q, pair_col, item_off, items, scores, out_ids, lds, width, (hipStream_t)stream);
    DIR_CATCH
}

int dir_code_sums(const int8_t* qcodes, int ldq, int Q, int D, int* qsums, void* stream) {
    DIR_TRY
    if (Q < 0) return fail(DIR_ERR_INVALID, "code_sums: negative size");
    DIR_CHECK(bin_check_dim("code_sums", D));
    if (ldq < D) return fail(DIR_ERR_INVALID, "code_sums: ldq < D");
    if (Q == 0) return DIR_OK;
    if (!qcodes || !qsums) return fail(DIR_ERR_INVALID, "code_sums: null pointer");
    return code_sums(qcodes, ldq, Q, D, qsums, (hipStream_t)stream);
    DIR_CATCH
}

int dir_ivf_scan_bin(const int8_t* qcodes, int ldq, const float* qscales, const int* qsums, int Q, const uint8_t* bits, int ldb,
                     const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                     const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                     int lds, int width, void* stream) {
    DIR_TRY
    DIR_CHECK(ivf_scan_check(
        "ivf_scan_bin", bin_check_dim, D, Q, N, nlist, items, width, lds,
        ldq < pad64(D)        ? "ldq < D rounded up to a multiple of 64"
        : ldb < bin_row_bytes(D) ? "ldb < D rounded up to a multiple of 128, divided by 8"
                             : nullptr,
        scores, out_ids,
        !qcodes || !qscales || !qsums || !bits || !bscales || !ids || !list_off || !pair_off || !pair_q || !pair_col || !item_off,
        ivf_scan_admissible(qcodes, ldq, Q, bits, ldb)
            ? nullptr
            : "ldq, ldb % 16 == 0, ldb < 2^23, Q * ldq < 2^31 and 16-byte aligned codes and bits"));
    return ivf_scan_bin(qcodes, ldq, qscales, qsums, Q, bits, ldb, bscales, ids, N, D, list_off, nlist, pair_off, pair_q, pair_col,
                        item_off, items, scores, out_ids, lds, width, (hipStream_t)stream);
    DIR_CATCH
}

int dir_ivf_plan_max_pairs(void) { return ivf_plan_max_pairs(); }

int dir_ivf_plan(const int* probe, int Q, int nprobe, const int* list_off, int nlist, int* col_off, int* pair_off, int* pair_q,
                 int* pair_col, int* item_off, int* counts, void* stream) {
    DIR_TRY
    if (Q < 0 || nprobe < 0 || nlist < 0) return fail(DIR_ERR_INVALID, "ivf_plan: negative size");
    if (nlist > 65535) return fail(DIR_ERR_INVALID, "ivf_plan: more than 65535 lists");
    if ((long)Q * nprobe > ivf_plan_max_pairs())
        return fail(DIR_ERR_INVALID, "ivf_plan: Q * nprobe exceeds dir_ivf_plan_max_pairs(): cut the queries");
    if (Q == 0) return DIR_OK;
    if (nlist < 1) return fail(DIR_ERR_INVALID, "ivf_plan: queries without a list");
    if (!list_off || !pair_off || !item_off || !counts || (nprobe > 0 && (!probe || !col_off || !pair_q || !pair_col)))
        return fail(DIR_ERR_INVALID, "ivf_plan: null pointer");
    return ivf_plan(probe, Q, nprobe, list_off, nlist, col_off, pair_off, pair_q, pair_col, item_off, counts,
                    (hipStream_t)stream);
    DIR_CATCH
}

int dir_topk_max_k(void) { return topk_max_k(); }

static int topk_check_sizes(int Q, int N, int k) {
    if (Q < 0 || N < 0) return fail(DIR_ERR_INVALID, "topk: negative size");
    if (k < 1) return fail(DIR_ERR_INVALID, "topk: k < 1");
    if (k > N || k > topk_max_k()) return fail(DIR_ERR_INVALID, "topk: k exceeds min(N, dir_topk_max_k())");
    return DIR_OK;
}

int dir_topk_workspace_bytes(int Q, int N, int k, size_t* bytes) {
    DIR_TRY
    if (!bytes) return fail(DIR_ERR_INVALID, "topk_workspace_bytes: null pointer");
    DIR_CHECK(topk_check_sizes(Q, N, k));
    *bytes = topk_workspace_bytes(Q, N, k);
    return DIR_OK;
    DIR_CATCH
}

int dir_topk(const float* scores, int lds, int Q, int N, int k, const int* ids, const int* exclude, int* out_idx,
             float* out_score, void* workspace, size_t workspace_bytes, void* stream) {
    DIR_TRY
    DIR_CHECK(topk_check_sizes(Q, N, k));
    if (lds < N) return fail(DIR_ERR_INVALID, "topk: lds < N");
    if (Q == 0) return DIR_OK;
    if (!scores || !out_idx || !out_score) return fail(DIR_ERR_INVALID, "topk: null pointer");
    const size_t need = topk_workspace_bytes(Q, N, k);
    if (workspace_bytes < need || (need > 0 && !workspace))
        return fail(DIR_ERR_INVALID, "topk: workspace smaller than dir_topk_workspace_bytes");
    return topk(scores, lds, Q, N, k, ids, exclude, out_idx, out_score, workspace, workspace_bytes, (hipStream_t)stream);
    DIR_CATCH
}

int dir_pq_max_m(void) { return pq_max_m(); }

// D and M of a product quantiser: 1 <= M <= dir_pq_max_m(), M divides D, D within the int8 index's widest row
static int pq_check_dims(const char* who, int D, int M) {
    DIR_CHECK(index_check_dim(who, D));
    if (M < 1 || M > pq_max_m()) return fail(DIR_ERR_INVALID, std::string(who) + ": M outside 1 .. dir_pq_max_m()");
    if (D % M != 0) return fail(DIR_ERR_INVALID, std::string(who) + ": M does not divide D");
    return DIR_OK;
}

int dir_pq_encode(const float* X, int ldx, int N, int D, int M, const float* codebooks, uint8_t* codes, int ldc, void* stream) {
    DIR_TRY
    if (N < 0) return fail(DIR_ERR_INVALID, "pq_encode: negative size");
    DIR_CHECK(pq_check_dims("pq_encode", D, M));
    if (ldx < D) return fail(DIR_ERR_INVALID, "pq_encode: ldx < D");
    if (ldc < M || ldc % 4 != 0) return fail(DIR_ERR_INVALID, "pq_encode: ldc < M or ldc % 4 != 0");
    if (N == 0) return DIR_OK;
    if (!X || !codebooks || !codes) return fail(DIR_ERR_INVALID, "pq_encode: null pointer");
    return pq_encode(X, ldx, N, D, M, codebooks, codes, ldc, (hipStream_t)stream);
    DIR_CATCH
}

int dir_pq_lut(const float* queries, int ldq, int Q, int D, int M, const float* codebooks, float* lut, void* stream) {
    DIR_TRY
    if (Q < 0) return fail(DIR_ERR_INVALID, "pq_lut: negative size");
    DIR_CHECK(pq_check_dims("pq_lut", D, M));
    if (ldq < D) return fail(DIR_ERR_INVALID, "pq_lut: ldq < D");
    if (Q == 0) return DIR_OK;
    if (!queries || !codebooks || !lut) return fail(DIR_ERR_INVALID, "pq_lut: null pointer");
    return pq_lut(queries, ldq, Q, D, M, codebooks, lut, (hipStream_t)stream);
    DIR_CATCH
}

int dir_pq_scan(const float* lut, int Q, int M, const uint8_t* codes, int ldc, int N, float* scores, int lds, void* stream) {
    DIR_TRY
    if (Q < 0 || N < 0) return fail(DIR_ERR_INVALID, "pq_scan: negative size");
    if (M < 1 || M > pq_max_m()) return fail(DIR_ERR_INVALID, "pq_scan: M outside 1 .. dir_pq_max_m()");
    if (ldc < M || ldc % 4 != 0) return fail(DIR_ERR_INVALID, "pq_scan: ldc < M or ldc % 4 != 0");
    if (lds < N) return fail(DIR_ERR_INVALID, "pq_scan: lds < N");
    if (Q == 0 || N == 0) return DIR_OK;
    if (!lut || !codes || !scores) return fail(DIR_ERR_INVALID, "pq_scan: null pointer");
    if ((((uintptr_t)lut) & 15) != 0 || (((uintptr_t)codes) & 3) != 0)
        return fail(DIR_ERR_INVALID, "pq_scan: a 16-byte aligned lut and 4-byte aligned codes expected");
    return pq_scan(lut, Q, M, codes, ldc, N, scores, lds, (hipStream_t)stream);
    DIR_CATCH
}

int dir_ivfpq_scan_cols(void) { return ivfpq_scan_cols(); }

int dir_ivfpq_base(const float* queries, int ldq, int Q, const float* centroids, int ldc, int nlist, int D, int M,
                   const int* probe, int nprobe, float* base, void* stream) {
    DIR_TRY
    if (Q < 0 || nlist < 0 || nprobe < 0) return fail(DIR_ERR_INVALID, "ivfpq_base: negative size");
    DIR_CHECK(pq_check_dims("ivfpq_base", D, M));
    if (ldq < D || ldc < D) return fail(DIR_ERR_INVALID, "ivfpq_base: ldq, ldc < D");
    if (Q == 0 || nprobe == 0) return DIR_OK;
    if (!queries || !probe || !base || (nlist > 0 && !centroids)) return fail(DIR_ERR_INVALID, "ivfpq_base: null pointer");
    return ivfpq_base(queries, ldq, Q, centroids, ldc, nlist, D, M, probe, nprobe, base, (hipStream_t)stream);
    DIR_CATCH
}

int dir_ivfpq_scan(const float* lut, const float* base, int Q, int M, const uint8_t* codes, int ldc, const int* ids, int N,
                   const int* list_off, int nlist, const int* probe, const int* col_off, int nprobe, float* scores,
                   int* out_ids, int lds, int width, void* stream) {
    DIR_TRY
    if (Q < 0 || N < 0 || nlist < 0 || nprobe < 0 || width < 0) return fail(DIR_ERR_INVALID, "ivfpq_scan: negative size");
    if (M < 1 || M > pq_max_m()) return fail(DIR_ERR_INVALID, "ivfpq_scan: M outside 1 .. dir_pq_max_m()");
    if (ldc < M || ldc % 4 != 0) return fail(DIR_ERR_INVALID, "ivfpq_scan: ldc < M or ldc % 4 != 0");
    if (lds < width) return fail(DIR_ERR_INVALID, "ivfpq_scan: lds < width");
    if (Q == 0 || width == 0) return DIR_OK;
    if (!lut || !scores || !out_ids) return fail(DIR_ERR_INVALID, "ivfpq_scan: null pointer");
    if (nprobe > 0 && (!base || !probe || !col_off)) return fail(DIR_ERR_INVALID, "ivfpq_scan: null pointer");
    if (nprobe > 0 && nlist > 0 && N > 0 && (!codes || !ids || !list_off)) return fail(DIR_ERR_INVALID, "ivfpq_scan: null pointer");
    if ((((uintptr_t)lut) & 15) != 0 || (((uintptr_t)codes) & 3) != 0)
        return fail(DIR_ERR_INVALID, "ivfpq_scan: a 16-byte aligned lut and 4-byte aligned codes expected");
    return ivfpq_scan(lut, base, Q, M, codes, ldc, ids, N, list_off, nlist, probe, col_off, nprobe, scores, out_ids, lds, width,
                      (hipStream_t)stream);
    DIR_CATCH
}

int dir_expand_descriptors(const float* descs, int n, const float* db, int m, int D, int k, float alpha,
                           int self_set, float* out, float* sim, size_t sim_bytes, void* stream) {
    DIR_TRY
    if (n < 0 || m < 0 || D <= 0) return fail(DIR_ERR_INVALID, "expand_descriptors: bad size");
    if (n == 0) return DIR_OK;
    if (!descs || !db || !out || !sim) return fail(DIR_ERR_INVALID, "expand_descriptors: null pointer");
    return expand_descriptors(descs, n, db, m, D, k, alpha, self_set, out, sim, sim_bytes, (hipStream_t)stream);
    DIR_CATCH
}

int dir_expand_lists(const float* descs, int ldd, int n, const float* db, int ldb, int m, int D, const int* idx,
                     const float* vals, int ldl, int k, float alpha, float* out, int ldo, void* stream) {
    DIR_TRY
    if (n < 0 || m < 0 || k < 0) return fail(DIR_ERR_INVALID, "expand_lists: negative size");
    if (D < 1) return fail(DIR_ERR_INVALID, "expand_lists: D < 1");
    if (ldd < D || ldb < D || ldo < D) return fail(DIR_ERR_INVALID, "expand_lists: ldd, ldb, ldo < D");
    if (ldl < k) return fail(DIR_ERR_INVALID, "expand_lists: ldl < k");
    if (!(alpha >= 0.f)) return fail(DIR_ERR_INVALID, "expand_lists: alpha must be non-negative");
    if (n == 0) return DIR_OK;
    if (!descs || !db || !out || (k > 0 && (!idx || !vals))) return fail(DIR_ERR_INVALID, "expand_lists: null pointer");
    return expand_lists(descs, ldd, n, db, ldb, D, idx, vals, ldl, k, alpha, out, ldo, (hipStream_t)stream);
    DIR_CATCH
}

int dir_diffusion_slab_rows(void) { return diffusion_slab_rows(); }

// gamma of the graph and of the seeds: non-negative, not a NaN
static int diffusion_check_gamma(const char* who, float gamma) {
    if (!(gamma >= 0.f)) return fail(DIR_ERR_INVALID, std::string(who) + ": gamma must be non-negative");
    return DIR_OK;
}

int dir_knn_graph(const int* idx, const float* vals, int ldl, int N, int k, float gamma, float* S, int lds, void* stream) {
    DIR_TRY
    if (N < 0 || k < 0) return fail(DIR_ERR_INVALID, "knn_graph: negative size");
    if (k > topk_max_k()) return fail(DIR_ERR_INVALID, "knn_graph: k exceeds dir_topk_max_k()");
    if (ldl < k || lds < k) return fail(DIR_ERR_INVALID, "knn_graph: ldl, lds < k");
    DIR_CHECK(diffusion_check_gamma("knn_graph", gamma));
    if (N == 0 || k == 0) return DIR_OK;
    if (!idx || !vals || !S) return fail(DIR_ERR_INVALID, "knn_graph: null pointer");
    return knn_graph(idx, vals, ldl, N, k, gamma, S, lds, (hipStream_t)stream);
    DIR_CATCH
}

int dir_diffusion_seed(const int* qidx, const float* qvals, int ldq, int Q, int kq, int N, float gamma, float* Y, int ldy,
                       void* stream) {
    DIR_TRY
    if (Q < 0 || kq < 0 || N < 0) return fail(DIR_ERR_INVALID, "diffusion_seed: negative size");
    if (kq > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_seed: kq exceeds dir_topk_max_k()");
    if (ldq < kq) return fail(DIR_ERR_INVALID, "diffusion_seed: ldq < kq");
    if (ldy < Q) return fail(DIR_ERR_INVALID, "diffusion_seed: ldy < Q");
    DIR_CHECK(diffusion_check_gamma("diffusion_seed", gamma));
    if (Q == 0 || N == 0) return DIR_OK;
    if (!Y || (kq > 0 && (!qidx || !qvals))) return fail(DIR_ERR_INVALID, "diffusion_seed: null pointer");
    return diffusion_seed(qidx, qvals, ldq, Q, kq, N, gamma, Y, ldy, (hipStream_t)stream);
    DIR_CATCH
}

int dir_diffusion_workspace_bytes(int N, int Q, size_t* bytes) {
    DIR_TRY
    if (!bytes) return fail(DIR_ERR_INVALID, "diffusion_workspace_bytes: null pointer");
    if (N < 0 || Q < 0) return fail(DIR_ERR_INVALID, "diffusion_workspace_bytes: negative size");
    *bytes = diffusion_workspace_bytes(N, Q);
    return DIR_OK;
    DIR_CATCH
}

int dir_diffusion_solve(const int* idx, int ldl, const float* S, int lds, int N, int k, const float* Y, int ldy, int Q,
                        float alpha, int iters, float* F, int ldf, void* workspace, size_t workspace_bytes, void* stream) {
    DIR_TRY
    if (N < 0 || k < 0 || Q < 0 || iters < 0) return fail(DIR_ERR_INVALID, "diffusion_solve: negative size");
    if (k > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_solve: k exceeds dir_topk_max_k()");
    if (ldl < k || lds < k) return fail(DIR_ERR_INVALID, "diffusion_solve: ldl, lds < k");
    if (ldy < Q || ldf < Q) return fail(DIR_ERR_INVALID, "diffusion_solve: ldy, ldf < Q");
    if (!(alpha >= 0.f && alpha < 1.f)) return fail(DIR_ERR_INVALID, "diffusion_solve: alpha outside [0, 1)");
    if (N == 0 || Q == 0) return DIR_OK;
    if (!Y || !F || (k > 0 && (!idx || !S))) return fail(DIR_ERR_INVALID, "diffusion_solve: null pointer");
    if (iters > 0) {
        if (!workspace || workspace_bytes < diffusion_workspace_bytes(N, Q))
            return fail(DIR_ERR_INVALID, "diffusion_solve: workspace smaller than dir_diffusion_workspace_bytes");
        if ((((uintptr_t)workspace) & 15) != 0) return fail(DIR_ERR_INVALID, "diffusion_solve: a 16-byte aligned workspace expected");
    }
    return diffusion_solve(idx, ldl, S, lds, N, k, Y, ldy, Q, alpha, iters, F, ldf, workspace, (hipStream_t)stream);
    DIR_CATCH
}

int dir_diffusion_local_max_rows(void) { return topk_max_k(); }

int dir_diffusion_subgraph(const int* idx, int ldl, const float* S, int lds, int N, int k, const int* cidx, const float* cvals,
                           int ldc, int Q, int T, int kq, float gamma, int one_hot, int* cid, int* lidx, float* lw, float* y,
                           int ldt, void* stream) {
    DIR_TRY
    if (N < 0 || k < 0 || Q < 0 || T < 0 || kq < 0) return fail(DIR_ERR_INVALID, "diffusion_subgraph: negative size");
    if (k > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_subgraph: k exceeds dir_topk_max_k()");
    if (T < 1 || T > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_subgraph: 1 <= T <= dir_diffusion_local_max_rows() expected");
    if (ldl < k || lds < k) return fail(DIR_ERR_INVALID, "diffusion_subgraph: ldl, lds < k");
    if (ldc < T || ldt < T) return fail(DIR_ERR_INVALID, "diffusion_subgraph: ldc, ldt < T");
    DIR_CHECK(diffusion_check_gamma("diffusion_subgraph", gamma));
    if (Q == 0) return DIR_OK;
    if (!cidx || !cid || !y || (k > 0 && (!lidx || !lw)) || (k > 0 && N > 0 && (!idx || !S)) || (!one_hot && kq > 0 && !cvals))
        return fail(DIR_ERR_INVALID, "diffusion_subgraph: null pointer");
    return diffusion_subgraph(idx, ldl, S, lds, N, k, cidx, cvals, ldc, Q, T, kq, gamma, one_hot, cid, lidx, lw, y, ldt,
                              (hipStream_t)stream);
    DIR_CATCH
}

int dir_diffusion_solve_local(const int* lidx, const float* lw, int k, const float* y, const int* cid, int ldt, int Q, int T,
                              float alpha, int iters, float* f, int ldf, void* stream) {
    DIR_TRY
    if (k < 0 || Q < 0 || T < 0 || iters < 0) return fail(DIR_ERR_INVALID, "diffusion_solve_local: negative size");
    if (k > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_solve_local: k exceeds dir_topk_max_k()");
    if (T < 1 || T > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_solve_local: 1 <= T <= dir_diffusion_local_max_rows() expected");
    if (ldt < T || ldf < T) return fail(DIR_ERR_INVALID, "diffusion_solve_local: ldt, ldf < T");
    if (!(alpha >= 0.f && alpha < 1.f)) return fail(DIR_ERR_INVALID, "diffusion_solve_local: alpha outside [0, 1)");
    if (Q == 0) return DIR_OK;
    if (!y || !f || (k > 0 && (!lidx || !lw))) return fail(DIR_ERR_INVALID, "diffusion_solve_local: null pointer");
    return diffusion_solve_local(lidx, lw, k, y, cid, ldt, Q, T, alpha, iters, f, ldf, (hipStream_t)stream);
    DIR_CATCH
}

int dir_diffusion_spread(float* scores, int lds, int Q, int N, const int* cid, const float* f, int ldt, int T, void* stream) {
    DIR_TRY
    if (Q < 0 || N < 0 || T < 0) return fail(DIR_ERR_INVALID, "diffusion_spread: negative size");
    if (T > topk_max_k()) return fail(DIR_ERR_INVALID, "diffusion_spread: T exceeds dir_diffusion_local_max_rows()");
    if (lds < N) return fail(DIR_ERR_INVALID, "diffusion_spread: lds < N");
    if (ldt < T) return fail(DIR_ERR_INVALID, "diffusion_spread: ldt < T");
    if (Q == 0 || N == 0) return DIR_OK;
    if (!scores || (T > 0 && (!cid || !f))) return fail(DIR_ERR_INVALID, "diffusion_spread: null pointer");
    return diffusion_spread(scores, lds, Q, N, cid, f, ldt, T, (hipStream_t)stream);
    DIR_CATCH
}

int dir_multiscale_pool(const float* x, float* out, int S, int N, int D, int mode, float gemp,
                        void* stream) {
    DIR_TRY
    if (!x || !out || N < 0 || D < 0) return fail(DIR_ERR_INVALID, "multiscale_pool: bad argument");
    return multiscale_pool(x, out, S, N, D, mode, gemp, (hipStream_t)stream);
    DIR_CATCH
}

}  // extern "C"
