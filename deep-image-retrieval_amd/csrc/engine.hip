// engine.hip — ResNet_RMAC descriptor extraction on one MI355X.
//
// What the reference does in Python with torch.nn modules
//   ResNet.forward        dirtorch/nets/backbones/resnet.py:157-174
//   Bottleneck.forward    dirtorch/nets/backbones/resnet.py:67-87   (BasicBlock :29-44)
//   ResNet_RMAC.forward   dirtorch/nets/rmac_resnet.py:39-69
// becomes a fixed launch sequence over caller-owned workspace:
//   prep (s2d) -> stem conv(+BN+ReLU) -> maxpool -> [bottleneck: 1x1 -> 3x3(s) -> 1x1 (+ds) +res +ReLU]*
//   -> global pool (GeM/max/avg, fp32) -> (L2) -> FC (fp32 MFMA) -> L2.
// Eval-mode BatchNorm (eps 1e-5) is folded into the conv weights and a per-channel fp32 bias at
// finalize(); activations stay NHWC 16-bit between kernels, every reduction is fp32.
#include "engine.h"

#include <math.h>
#include <algorithm>

namespace dir {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
const char* last_error() { return g_err.c_str(); }


static Env read_env() {
    Env e;
    auto on = [](const char* k) { return getenv(k) != nullptr; };
    const char* mode = getenv("DIRTORCH_AMD_C3C1");
    e.c3c1_off = mode && mode[0] == '0';
    e.c3c1_force = mode && mode[0] == 'f';
    e.no_ds_seam = on("DIRTORCH_AMD_NO_DS_SEAM");
    e.no_dual = on("DIRTORCH_AMD_NO_DUAL");
    e.rev_conv1 = on("DIRTORCH_AMD_REV_CONV1");
    e.rev_conv3 = on("DIRTORCH_AMD_REV_CONV3");
    e.unfused_stem = on("DIRTORCH_AMD_UNFUSED_STEM");
    e.stem_v1 = on("DIRTORCH_AMD_STEM_V1");
    e.no_patchlc = on("DIRTORCH_AMD_NO_PATCHLC");
    e.no_wreg = on("DIRTORCH_AMD_NO_WREG");
    e.no_wregd = on("DIRTORCH_AMD_NO_WREGD");
    e.no_smallmap = on("DIRTORCH_AMD_NO_SMALLMAP");
    e.no_c3c1lc = on("DIRTORCH_AMD_NO_C3C1LC");
    e.lc1x1 = on("DIRTORCH_AMD_LC1X1");
    e.x3_k2048 = on("DIRTORCH_AMD_X3_K2048");
    e.no_patchs2 = on("DIRTORCH_AMD_NO_PATCHS2");
    e.small_k2 = on("DIRTORCH_AMD_SMALL_K2");
    e.patchw_pack = on("DIRTORCH_AMD_PATCHW_PACK");
    e.no_patchw_pack = on("DIRTORCH_AMD_NO_PATCHW_PACK");
    e.no_patchw = on("DIRTORCH_AMD_NO_PATCHW");
    e.no_x3 = on("DIRTORCH_AMD_NO_X3");
    e.no_patchs = on("DIRTORCH_AMD_NO_PATCHS");
    e.no_patchw_lc = on("DIRTORCH_AMD_NO_PATCHW_LC");
    e.no_xcdmap = on("DIRTORCH_AMD_NO_XCDMAP");
    e.no_pair_patch = on("DIRTORCH_AMD_NO_PAIR_PATCH");
    e.pair_acts = on("DIRTORCH_AMD_PAIR_ACTS");
    if (const char* s = getenv("DIRTORCH_AMD_PAIR_STAGES")) e.pair_stages = atoi(s);
    e.sim_v1 = on("DIRTORCH_AMD_SIM_V1");
    e.sim_exact = on("DIRTORCH_AMD_SIM_EXACT");
    e.experiments = on("DIRTORCH_AMD_EXPERIMENTS");
    e.no_inplace = on("DIRTORCH_AMD_NO_INPLACE");
    e.seam_full_store = on("DIRTORCH_AMD_SEAM_FULL_STORE");
    e.no_stem_u8 = on("DIRTORCH_AMD_NO_STEM_U8");
    e.stem_u8_wg8 = on("DIRTORCH_AMD_STEM_U8_WG8");
    e.stem_u8_prep = on("DIRTORCH_AMD_STEM_U8_PREP");
    e.stem_pair_old = on("DIRTORCH_AMD_STEM_PAIR_OLD");
    if (const char* s = getenv("DIRTORCH_AMD_STEM_U8_SEG")) e.stem_u8_seg = atoi(s);
    return e;
}
// Two snapshots and an atomic index: dir_reload_env fills the idle one and publishes it with one store, so a launch that reads
// env() concurrently sees the old set or the new one, never a torn struct (round-5 advice).  (A reader that still holds a reference
// while a SECOND reload recycles its slot is the remaining window: reloads are a test / A-B tool, two per launch do not happen.)
static Env g_env[2];
static std::atomic<int> g_env_cur{-1};
static std::atomic_flag g_env_lock = ATOMIC_FLAG_INIT;
static void publish_env() {
    while (g_env_lock.test_and_set(std::memory_order_acquire)) {
    }
    const int cur = g_env_cur.load(std::memory_order_relaxed);
    const int nxt = cur < 0 ? 0 : 1 - cur;
    g_env[nxt] = read_env();
    g_env_cur.store(nxt, std::memory_order_release);
    g_env_lock.clear(std::memory_order_release);
}
const Env& env() {
    int cur = g_env_cur.load(std::memory_order_acquire);
    if (cur < 0) {
        static const bool once = (publish_env(), true);   // (thread-safe first use)
        (void)once;
        cur = g_env_cur.load(std::memory_order_acquire);
    }
    return g_env[cur];
}
void reload_env() { publish_env(); }   // host-driven (dir_reload_env)

static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// Deterministic noise in [-1, 1) for autotune inputs (no host RNG, no cuRAND analogue needed).
__global__ void fill_noise_kernel(uint16_t* p, long n, int dtype) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t h = (uint32_t)i * 2654435761u + 12345u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    const float f = (float)(h & 0xffff) / 32768.f - 1.f;
    p[i] = dtype == DIR_BF16 ? f32_to_bf16_bits(f) : f32_to_f16_bits(f);
}

}  // namespace dir

using namespace dir;

// ---- graph ------------------------------------------------------------------------------------
int dir_engine::build_graph() {
    convs.clear();
    blocks.clear();
    const int expansion = desc.bottleneck ? 4 : 1;
    auto add_conv = [&](const std::string& name, const std::string& wkey, const std::string& bn,
                        int cin, int cout, int k, int stride, int pad, bool relu) {
        ConvLayer L;
        L.name = name;
        L.wkey = wkey;
        L.bnprefix = bn;
        L.Cin = cin;
        L.Cout = cout;
        L.R = L.S = k;
        L.stride = stride;
        L.pad = pad;
        L.relu = relu;
        convs.push_back(L);
        return (int)convs.size() - 1;
    };
    // stem: 7x7 s2 p3, 3 -> 64 (resnet.py:115-118); executed as 4x4 s1 over the s2d image.
    {
        int i = add_conv("conv1", "conv1.weight", "bn1", 3, 64, 7, 2, 3, true);
        convs[i].stem = true;
    }
    int inplanes = 64;
    const int planes_of[4] = {64, 128, 256, 512};
    for (int s = 0; s < 4; ++s) {
        const int planes = planes_of[s];
        const int nblk = desc.layers[s];
        if (nblk <= 0) return fail(DIR_ERR_INVALID, "model desc: layers[] must be positive");
        for (int j = 0; j < nblk; ++j) {
            const int stride = (j == 0 && s > 0) ? 2 : 1;
            const std::string pre = "layer" + std::to_string(s + 1) + "." + std::to_string(j);
            BlockDef bd;
            bd.stride = stride;
            if (desc.bottleneck) {
                bd.conv1 = add_conv(pre + ".conv1", pre + ".conv1.weight", pre + ".bn1", inplanes,
                                    planes, 1, 1, 0, true);
                bd.conv2 = add_conv(pre + ".conv2", pre + ".conv2.weight", pre + ".bn2", planes,
                                    planes, 3, stride, 1, true);
                bd.conv3 = add_conv(pre + ".conv3", pre + ".conv3.weight", pre + ".bn3", planes,
                                    planes * 4, 1, 1, 0, true);  // ReLU after the residual add
            } else {
                bd.conv1 = add_conv(pre + ".conv1", pre + ".conv1.weight", pre + ".bn1", inplanes,
                                    planes, 3, stride, 1, true);
                bd.conv2 = add_conv(pre + ".conv2", pre + ".conv2.weight", pre + ".bn2", planes,
                                    planes, 3, 1, 1, true);  // ReLU after the residual add
            }
            if (j == 0 && (stride != 1 || inplanes != planes * expansion)) {
                // resnet.py:134-141: 1x1 conv (stride) + BN, no ReLU
                bd.down = add_conv(pre + ".downsample", pre + ".downsample.0.weight",
                                   pre + ".downsample.1", inplanes, planes * expansion, 1, stride, 0,
                                   false);
            }
            inplanes = planes * expansion;
            blocks.push_back(bd);
        }
    }
    feat_dim = inplanes;
    head_dim = feat_dim;
    x4_dim = 0;
    x4_block = conv1x5 = conv3c4 = -1;
    if (desc.head == DIR_HEAD_FPN || desc.head == DIR_HEAD_FPN0) {
        // rmac_resnet_fpn.py:24-32: dim1 = layer3 width, dim2 = layer4 width
        x4_dim = 256 * expansion;
        head_dim = x4_dim + feat_dim;
        x4_block = desc.layers[0] + desc.layers[1] + desc.layers[2] - 1;
        if (desc.head == DIR_HEAD_FPN) {
            // 1x1 conv commutes with the nearest upsample, so it runs on the small x5 grid
            conv1x5 = add_conv("conv1x5", "conv1x5.weight", "", feat_dim, x4_dim, 1, 1, 0, true);
            conv3c4 = add_conv("conv3c4", "conv3c4.weight", "", x4_dim, x4_dim, 3, 1, 1, true);
        }
    }
    return DIR_OK;
}

// ---- weights ------------------------------------------------------------------------------------
static const HostTensor* find(const std::map<std::string, HostTensor>& st, const std::string& k) {
    auto it = st.find(k);
    return it == st.end() ? nullptr : &it->second;
}

int dir_engine::finalize(int dt) {
    if (dt != DIR_BF16 && dt != DIR_FP16 && dt != DIR_F32 && dt != DIR_FP16P)
        return fail(DIR_ERR_INVALID, "finalize: bad dtype");
    DIR_HIP_CHECK(hipSetDevice(device));
    release();
    dtype = dt;
    auto to16 = [&](float f) { return dt == DIR_BF16 ? f32_to_bf16_bits(f) : f32_to_f16_bits(f); };
    // DIR_FP16P: the stem and the first pair_blocks residual blocks keep their weights as fp16 PAIRS (conv_pair.hip).
    // Default = all of layer1 (where tests/precision_decomposition.py puts the 16-bit error of a conditioned network);
    // DIRTORCH_AMD_PAIR_STAGES = 1..4 moves the boundary to the end of that stage.  Which weights: every conv of those
    // blocks with pair_acts (engine.h), else their 1x1s only.
    pair_blocks = 0;
    pair_acts = !desc.bottleneck || sw.pair_acts;
    std::vector<char> is_pair(convs.size(), 0);
    if (dt == DIR_FP16P) {
        const int stages = sw.pair_stages;
        if (stages < 1 || stages > 4) return fail(DIR_ERR_INVALID, "finalize: DIRTORCH_AMD_PAIR_STAGES must be 1..4");
        for (int s = 0; s < stages; ++s) pair_blocks += desc.layers[s];
        if (x4_block >= 0 && pair_blocks > x4_block)
            return fail(DIR_ERR_INVALID, "finalize: the FPN heads keep layer3's output as a single fp16 plane; "
                                         "DIRTORCH_AMD_PAIR_STAGES must stay below 3 for them");
        is_pair[0] = 1;
        for (int bi = 0; bi < pair_blocks; ++bi) {
            const BlockDef& bd = blocks[bi];
            for (int ci : {bd.conv1, bd.conv2, bd.conv3, bd.down})
                if (ci >= 0 && (pair_acts || (convs[ci].R == 1 && convs[ci].S == 1))) is_pair[ci] = 1;
        }
    }

    for (size_t li = 0; li < convs.size(); ++li) {
        ConvLayer& L = convs[li];
        const HostTensor* w = find(state, L.wkey);
        const HostTensor* g = find(state, L.bnprefix + ".weight");
        const HostTensor* bt = find(state, L.bnprefix + ".bias");
        const HostTensor* mu = find(state, L.bnprefix + ".running_mean");
        const HostTensor* var = find(state, L.bnprefix + ".running_var");
        if (!w) return fail(DIR_ERR_MISSING, "missing tensor " + L.wkey);
        const bool has_bn = !L.bnprefix.empty();
        if (has_bn && (!g || !bt || !mu || !var))
            return fail(DIR_ERR_MISSING, "missing BatchNorm tensors " + L.bnprefix + ".*");
        const int64_t want[4] = {L.Cout, L.Cin, L.R, L.S};
        if (w->shape.size() != 4 || !std::equal(want, want + 4, w->shape.begin()))
            return fail(DIR_ERR_INVALID, "bad shape for " + L.wkey);
        if (has_bn && ((int)g->data.size() != L.Cout || (int)bt->data.size() != L.Cout ||
                       (int)mu->data.size() != L.Cout || (int)var->data.size() != L.Cout))
            return fail(DIR_ERR_INVALID, "bad BatchNorm shape for " + L.bnprefix);

        std::vector<float> scale(L.Cout, 1.f), bias(L.Cout, 0.f);
        for (int o = 0; has_bn && o < L.Cout; ++o) {
            // BatchNorm2d eval: y = (x - mean) / sqrt(var + eps) * gamma + beta, eps = 1e-5
            const float inv = 1.0f / sqrtf(var->data[o] + 1e-5f);
            scale[o] = g->data[o] * inv;
            bias[o] = bt->data[o] - mu->data[o] * scale[o];
        }
        // packed in fp32 first ([Cout][R][S][Cin], BatchNorm scale folded in with one fp32 multiply); the
        // 16-bit formats round that, the strict path (DIR_F32, conv_f32.hip) uploads it as is
        std::vector<float> packed;
        if (L.stem) {
            // 7x7 s2 p3 over 3 channels == 4x4 s1 (pad 2 top/left) over the 2x2 space-to-depth
            // image with 12 (+4 zero) channels: tap r = 2R + dy - 1, s = 2S + dx - 1.
            packed.assign((size_t)L.Cout * 4 * 4 * 16, 0.f);
            for (int o = 0; o < L.Cout; ++o)
                for (int R = 0; R < 4; ++R)
                    for (int S = 0; S < 4; ++S)
                        for (int dy = 0; dy < 2; ++dy)
                            for (int dx = 0; dx < 2; ++dx) {
                                const int r = 2 * R + dy - 1, s = 2 * S + dx - 1;
                                if (r < 0 || s < 0 || r >= 7 || s >= 7) continue;
                                for (int c = 0; c < 3; ++c) {
                                    const float v =
                                        w->data[(((size_t)o * 3 + c) * 7 + r) * 7 + s] * scale[o];
                                    packed[(((size_t)o * 4 + R) * 4 + S) * 16 + (dy * 2 + dx) * 3 + c] = v;
                                }
                            }
        } else {
            packed.resize((size_t)L.Cout * L.R * L.S * L.Cin);
            for (int o = 0; o < L.Cout; ++o)
                for (int c = 0; c < L.Cin; ++c)
                    for (int r = 0; r < L.R; ++r)
                        for (int s = 0; s < L.S; ++s) {
                            const float v =
                                w->data[(((size_t)o * L.Cin + c) * L.R + r) * L.S + s] * scale[o];
                            packed[(((size_t)o * L.R + r) * L.S + s) * L.Cin + c] = v;
                        }
        }
        DIR_CHECK(upload(&L.dev.bias, bias));
        L.tuned.clear();
        if (dt == DIR_F32) {
            DIR_CHECK(upload(&L.dev.wf, packed));
            continue;
        }
        std::vector<uint16_t> packed16(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) {
            packed16[i] = to16(packed[i]);
            // fp16 saturates at 65504: a folded weight beyond that would become inf here, on the host, where no
            // kernel's overflow word can see it (and inf * 0 = NaN is then flushed to 0 by the next fused ReLU)
            // (DIR_FP16P packs the same fp16 hi plane: hi = inf would make lo = fp16(w - inf) = -inf and hi + lo = NaN)
            if (dt != DIR_BF16 && (packed16[i] & 0x7c00u) == 0x7c00u && std::isfinite(packed[i]))
                return fail(DIR_ERR_RANGE, "finalize: a BatchNorm-folded weight of " + L.name + " (" +
                                               std::to_string(packed[i]) + ") exceeds the fp16 range; use DIR_BF16 or DIR_F32");
        }
        DIR_CHECK(upload(&L.dev.w, packed16));
        if (!L.stem && L.R == 3 && L.S == 3 && L.stride == 1 && L.pad == 1 && L.Cin % 32 == 0 && L.Cin >= 64 && L.Cout % 128 == 0) {
            // conv2 of layers 2-4: conv_patchw.hip's loaders copy their 24 KB weight stages as contiguous KBs from this copy
            DIR_CHECK(alloc(&L.dev.w_pw, packed16.size()));
            DIR_HIP_CHECK(conv_patch3x3w_pack(L.dev.w, L.dev.w_pw, L.Cout, L.Cin, nullptr));
        }
        if (!L.stem && L.R == 3 && L.S == 3 && L.stride == 2 && L.pad == 1 && L.Cin % 64 == 0 && L.Cout % 128 == 0) {
            // conv2 of a stage's first block: conv_patchs2.hip reads its weight fragments as contiguous KBs from this copy
            DIR_CHECK(alloc(&L.dev.w_s2, packed16.size()));
            DIR_HIP_CHECK(conv_patch3x3s2_pack(L.dev.w, L.dev.w_s2, L.Cout, L.Cin, nullptr));
        }
        if (L.stem && dt == DIR_FP16P) {   // (after the range check above: a weight the plain form refuses is reported as that layer's)
            DIR_CHECK(fold_stem_u8(L, w->data.data(), scale.data(), bias.data()));
        }
        if (is_pair[li]) {   // lo plane: what the hi plane's rounding left over, itself rounded to fp16
            std::vector<uint16_t> lo16(packed.size());
            for (size_t i = 0; i < packed.size(); ++i) {
                lo16[i] = f32_to_f16_bits(packed[i] - f16_bits_to_f32(packed16[i]));
                if ((lo16[i] & 0x7c00u) == 0x7c00u && std::isfinite(packed[i]))   // (unreachable once hi is finite: |lo| <= ulp(hi) / 2)
                    return fail(DIR_ERR_RANGE, "finalize: the lo plane of a paired weight of " + L.name + " is not finite");
            }
            DIR_CHECK(upload(&L.dev.w_lo, lo16));
            L.h_w_lo.swap(lo16);
        }
        L.h_w.swap(packed16);
        L.h_bias.swap(bias);
    }
    // First block of every stage (bottleneck nets): the residual is a 1x1 downsample conv of the block
    // input.  Its weights are appended to conv3's along K and the biases summed, so that
    // relu([W3 | Wds] . [t2 ; x_s] + b3 + bds) is ONE GEMM and the Cout-wide residual tensor is never
    // materialised: conv_c3c1's DS form (layer1: 64 + 64 channels, stride 1) or the two-source form of the
    // persistent 1x1 kernel (conv_persist.hip DUAL: layers 2-4, stride 2).
    for (const BlockDef& bd : blocks) {
        if (!desc.bottleneck || bd.down < 0 || bd.conv3 < 0 || dt == DIR_F32) continue;
        ConvLayer& c3 = convs[bd.conv3];
        const ConvLayer& ds = convs[bd.down];
        if (ds.R != 1 || ds.S != 1 || ds.pad != 0 || ds.Cout != c3.Cout || ds.Cin % 64 != 0 || c3.Cin % 64 != 0) continue;
        // paired head: conv_pair.hip's two-source form takes pixel-aligned sources of equal width only (layer1's first block)
        if (is_pair[bd.conv3] && (ds.stride != 1 || ds.Cin != c3.Cin || c3.Cout % 128 != 0)) continue;
        const int K3 = c3.Cin, Kd = ds.Cin, N = c3.Cout;
        std::vector<uint16_t> cat((size_t)N * (K3 + Kd));
        std::vector<float> bsum(N);
        for (int o = 0; o < N; ++o) {
            memcpy(&cat[(size_t)o * (K3 + Kd)], &c3.h_w[(size_t)o * K3], K3 * 2);
            memcpy(&cat[(size_t)o * (K3 + Kd) + K3], &ds.h_w[(size_t)o * Kd], Kd * 2);
            bsum[o] = c3.h_bias[o] + ds.h_bias[o];
        }
        DIR_CHECK(upload(&c3.dev.w_ds, cat));
        DIR_CHECK(upload(&c3.dev.bias_ds, bsum));
        if (is_pair[bd.conv3]) {   // the lo planes, concatenated the same way
            for (int o = 0; o < N; ++o) {
                memcpy(&cat[(size_t)o * (K3 + Kd)], &c3.h_w_lo[(size_t)o * K3], K3 * 2);
                memcpy(&cat[(size_t)o * (K3 + Kd) + K3], &ds.h_w_lo[(size_t)o * Kd], Kd * 2);
            }
            DIR_CHECK(upload(&c3.dev.w_ds_lo, cat));
        }
    }
    for (ConvLayer& L : convs) {
        std::vector<uint16_t>().swap(L.h_w_lo);
        std::vector<uint16_t>().swap(L.h_w);
        std::vector<float>().swap(L.h_bias);
    }

    const bool fpn = desc.head == DIR_HEAD_FPN || desc.head == DIR_HEAD_FPN0;
    if (desc.pooling == DIR_POOL_GEM && desc.head != DIR_HEAD_CLASSIFIER) {
        const char* keys[2] = {fpn ? "adpoolx5.p" : "adpool.p", "adpoolc4.p"};
        float* dst[2] = {&gem_p, &gem_p4};
        for (int i = 0; i < (fpn ? 2 : 1); ++i) {
            const HostTensor* p = find(state, keys[i]);
            if (!p || p->data.empty()) return fail(DIR_ERR_MISSING, std::string("missing tensor ") + keys[i]);
            *dst[i] = p->data[0];
            if (!(*dst[i] > 0.f)) return fail(DIR_ERR_INVALID, std::string(keys[i]) + " must be positive");
        }
    }
    if (!desc.without_fc) {
        const HostTensor* fw = find(state, "fc.weight");
        const HostTensor* fb = find(state, "fc.bias");
        if (!fw || !fb) return fail(DIR_ERR_MISSING, "missing tensor fc.weight / fc.bias");
        if (fw->shape.size() != 2 || fw->shape[0] != desc.out_dim || fw->shape[1] != head_dim ||
            (int)fb->data.size() != desc.out_dim)
            return fail(DIR_ERR_INVALID, "bad shape for fc.weight / fc.bias");
        DIR_CHECK(upload(&dev.fc_w, fw->data));
        DIR_CHECK(upload(&dev.fc_b, fb->data));
    }
    DIR_CHECK(alloc(&dev.ovf, 256 / sizeof(int)));
    DIR_HIP_CHECK(hipMemset(dev.ovf, 0, 256));
    DIR_HIP_CHECK(hipDeviceSynchronize());
    finalized = true;
    return DIR_OK;
}

// ---- the stem for the RAW uint8 feed (stem_u8.hip) ------------------------------------------------------------------------
// ToTensor + Normalize (dirtorch/utils/transforms.py:617-623: x = (u / 255 - mean_c) / std_c) folded into conv1 + bn1
// (resnet.py:115-117).  The image plane holds u / 256 (exact in fp16), so
//   w'[o][tap][c] = w . bn_scale[o] . 256 / (255 std_c)                       an fp16 pair, packed like the s2d stem filter
//   b'[o]         = bn_bias[o] - sum_{all 147 taps} w . bn_scale[o] . mean_c / std_c
//   corr[rc][cc][o] = + sum_{taps OUTSIDE the image for border class (rc, cc)} w . bn_scale[o] . mean_c / std_c
// (a padded tap is zero in normalised space, i.e. it must NOT contribute its - mean / std; classes as stem_u8.hip's
// border_class: 0 all taps r = 0..6 inside, 1: r >= 3, 2: r >= 1, 3 / 4 / 5: r <= 5 / 4 / 3).  Sums in double.
int dir_engine::fold_stem_u8(ConvLayer& L, const float* w, const float* scale, const float* bias) {
    (void)L;
    std::vector<uint16_t> hi, lo;
    std::vector<float> b2, corr;
    const int rc = dir::fold_stem_u8(w, scale, bias, desc.mean, desc.std, hi, lo, b2, corr);
    // a preprocess whose 1 / (255 std) pushes a folded weight out of the fp16 range (or a std <= 0) only rules the uint8 stem out:
    // the tables stay null and dir_forward keeps the generic paired stem (normalisation in prep_input_pair) for that engine
    if (rc == DIR_ERR_RANGE || rc == DIR_ERR_INVALID) return DIR_OK;
    DIR_CHECK(rc);
    DIR_CHECK(upload(&dev.stem_u8_w, hi));
    DIR_CHECK(upload(&dev.stem_u8_w_lo, lo));
    DIR_CHECK(upload(&dev.stem_u8_bias, b2));
    return upload(&dev.stem_u8_corr, corr);
}

// ---- device memory: every allocation is registered, release() frees the list -----------------------------------------------
int dir_engine::alloc_bytes(void** out, size_t bytes) {
    owned.push_back(nullptr);   // (registered first: a failed push_back must not strand a live allocation)
    DIR_HIP_CHECK(hipMalloc(&owned.back(), bytes));
    *out = owned.back();
    return DIR_OK;
}

void dir_engine::release() {
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
    for (ConvLayer& L : convs) L.dev = {};
    dev = {};
    finalized = false;
}

// ---- fp16 overflow word ------------------------------------------------------------------------------
// Reads (and clears) the word the kernels OR into whenever they store an fp16 inf / NaN.  Synchronises `stream`.
int dir_engine::overflow(hipStream_t stream, int* overflowed) {
    if (!finalized) return fail(DIR_ERR_STATE, "overflow query before finalize");
    int host = 0;
    DIR_HIP_CHECK(hipMemcpyAsync(&host, dev.ovf, sizeof(int), hipMemcpyDeviceToHost, stream));
    DIR_HIP_CHECK(hipMemsetAsync(dev.ovf, 0, sizeof(int), stream));
    DIR_HIP_CHECK(hipStreamSynchronize(stream));
    *overflowed = host != 0;
    return DIR_OK;
}

// ---- workspace plan ---------------------------------------------------------------------------
static inline int conv_out(int h, int k, int stride, int pad) { return (h + 2 * pad - k) / stride + 1; }

int dir_engine::plan(int B, int H, int W, Plan* p) const {
    if (B <= 0 || H <= 0 || W <= 0) return fail(DIR_ERR_INVALID, "forward: B, H, W must be positive");
    if (H < 7 || W < 7) return fail(DIR_ERR_INVALID, "forward: image smaller than the 7x7 stem");
    p->H2 = (H + 1) / 2;
    p->W2 = (W + 1) / 2;
    p->OH1 = conv_out(H, 7, 2, 3);
    p->OW1 = conv_out(W, 7, 2, 3);
    p->PH = conv_out(p->OH1, 3, 2, 1);
    p->PW = conv_out(p->OW1, 3, 2, 1);
    const size_t es = dtype == DIR_F32 ? 4 : 2;   // bytes per stored activation
    // One walk over blocks [0, nb) at `eb` bytes per element: the widest t1 / t2 / downsample tensor and block output (io),
    // layer3's kept output (x4) and the map size after the last block.  Run for the activations of the whole net and again
    // for the lo planes of the paired head, which only use t1 / t2 / ds of it.
    struct Extents {
        size_t t1 = 0, t2 = 0, ds = 0, io = 0, x4 = 0;
        int h = 0, w = 0;
    };
    auto block_extents = [&](size_t eb, size_t nb) {
        Extents e;
        e.h = p->PH;
        e.w = p->PW;
        e.io = (size_t)B * e.h * e.w * 64 * eb;
        for (size_t bi = 0; bi < nb; ++bi) {
            const BlockDef& bd = blocks[bi];
            const int oh = conv_out(e.h, 3, bd.stride, 1), ow = conv_out(e.w, 3, bd.stride, 1);
            const ConvLayer& c1 = convs[bd.conv1];
            const ConvLayer& cl = convs[desc.bottleneck ? bd.conv3 : bd.conv2];
            if (desc.bottleneck) {
                e.t1 = std::max(e.t1, (size_t)B * e.h * e.w * c1.Cout * eb);
                e.t2 = std::max(e.t2, (size_t)B * oh * ow * convs[bd.conv2].Cout * eb);
            } else {
                e.t1 = std::max(e.t1, (size_t)B * oh * ow * c1.Cout * eb);
            }
            if (bd.down >= 0) e.ds = std::max(e.ds, (size_t)B * oh * ow * convs[bd.down].Cout * eb);
            e.io = std::max(e.io, (size_t)B * oh * ow * cl.Cout * eb);
            e.h = oh;
            e.w = ow;
            if ((int)bi == x4_block) e.x4 = (size_t)B * e.h * e.w * x4_dim * eb;
        }
        return e;
    };
    Extents act = block_extents(es, blocks.size());
    act.t2 = std::max(act.t2, act.x4);   // FPN heads keep x4; the lateral path reuses t1 / t2 / a ping-pong buffer
    if (conv1x5 >= 0) act.t1 = std::max(act.t1, (size_t)B * act.h * act.w * x4_dim * es);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += align_up(bytes);
        return o;
    };
    p->s2d = take((size_t)B * p->H2 * p->W2 * 16 * es);
    p->stem = take((size_t)B * p->OH1 * p->OW1 * 64 * es);
    p->bufA = take(act.io);
    p->bufB = take(act.io);
    p->t1 = take(act.t1);
    p->t2 = take(act.t2 ? act.t2 : 256);
    p->ds = take(act.ds ? act.ds : 256);
    p->x4 = take(act.x4 ? act.x4 : 256);
    p->lo_s2d = p->lo_stem = p->lo_t1 = p->lo_t2 = p->lo_ds = 0;
    if (dtype == DIR_FP16P) {   // lo planes of the paired head: image, stem output [, t1 / t2 / downsample of its blocks]
        const Extents lo = block_extents(2, pair_acts ? std::min((size_t)pair_blocks, blocks.size()) : 0);
        p->lo_s2d = take((size_t)B * p->H2 * p->W2 * 16 * 2);
        p->lo_stem = take((size_t)B * p->PH * p->PW * 64 * 2);
        p->lo_t1 = take(lo.t1 ? lo.t1 : 256);
        p->lo_t2 = take(lo.t2 ? lo.t2 : 256);
        p->lo_ds = take(lo.ds ? lo.ds : 256);
    }
    p->splitk = take(kSplitKMaxBytes);   // fp32 partial sums of split-K convs (small-M layers)
    p->pooled = take((size_t)B * head_dim * 4);
    p->fcout = take((size_t)B * std::max(desc.out_dim, head_dim) * 4);
    p->total = off;
    return DIR_OK;
}

// ---- profiling --------------------------------------------------------------------------------
int dir_engine::prof_slot(ProfSlot** slot) {
    if (prof_used == prof.size()) {
        ProfSlot s;
        DIR_HIP_CHECK(hipEventCreate(&s.start));
        DIR_HIP_CHECK(hipEventCreate(&s.stop));
        prof.push_back(s);
    }
    *slot = &prof[prof_used];
    return DIR_OK;
}

// ---- one convolution ----------------------------------------------------------------------------
// A layer on a (B, H, W) input as the kernels see it.  The stem runs in its space-to-depth form: 4x4 stride 1 over the 16
// channels of the s2d image, and (H, W) is that grid.
static ConvGeom layer_geom(const ConvLayer& L, int B, int H, int W, int OH, int OW) {
    const int relu = L.relu ? 1 : 0;
    if (L.stem) return {B, H, W, 16, L.Cout, 4, 4, 1, 2, OH, OW, relu};
    return {B, H, W, L.Cin, L.Cout, L.R, L.S, L.stride, L.pad, OH, OW, relu};
}

// Autotune: time every admissible variant on the live input, keep the fastest.
int dir_engine::tune_conv(ConvLayer& L, ConvArgs& a, hipStream_t stream, int* variant) {
    hipEvent_t e0, e1;
    DIR_HIP_CHECK(hipEventCreate(&e0));
    DIR_HIP_CHECK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int v = 0; v < conv_variant_count(); ++v) {
        a.ksplit = 0;   // (the previous candidate's split must not decide this one's admissibility: conv_small, conv_patchs2
                        // and conv_persistlc refuse a.ksplit > 1)
        if (!conv_variant_admissible(v, a)) continue;
        a.ksplit = conv_splitk_factor(v, a);
        DIR_CHECK(conv_launch(a, kdtype(), v, stream));  // warm-up (also sets func attributes)
        float ms = 1e30f;
        for (int round = 0; round < 2; ++round) {  // best of two timings of 3 launches
            DIR_HIP_CHECK(hipEventRecord(e0, stream));
            for (int rep = 0; rep < 3; ++rep) DIR_CHECK(conv_launch(a, kdtype(), v, stream));
            DIR_HIP_CHECK(hipEventRecord(e1, stream));
            DIR_HIP_CHECK(hipEventSynchronize(e1));
            float t = 0.f;
            DIR_HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
            ms = t < ms ? t : ms;
        }
        if (ms < best) {
            best = ms;
            *variant = v;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    L.tuned[a.M] = *variant;
    return DIR_OK;
}

int dir_engine::run_conv(ConvLayer& L, const uint16_t* x, const uint16_t* res, uint16_t* y, int B,
                         int H, int W, int OH, int OW, hipStream_t stream, bool rev_m) {
    // DIR_FP16P: a layer whose weights are a pair multiplies both planes (conv_pair.hip; single-plane input and output here)
    if (dtype == DIR_FP16P && L.dev.w_lo && !L.stem)
        return run_conv_pair(L, x, nullptr, res, nullptr, y, nullptr, B, H, W, OH, OW, stream);
    ConvArgs a;
    conv_args_init(a, layer_geom(L, B, H, W, OH, OW), x, L.dev.w, L.dev.bias, res, y);
    a.rev_m = rev_m ? 1 : 0;
    a.w_s2 = L.dev.w_s2;
    a.w_pw = env().no_patchw_pack ? nullptr : L.dev.w_pw;
    a.ovf = dev.ovf;
    a.partial = splitk_scratch;
    const double macs = (double)a.M * L.Cout * (double)(L.R * L.S * L.Cin);  // true taps (stem: 147)
    const double bytes = 2.0 * ((double)B * H * W * a.Cin + (double)a.M * L.Cout * (res ? 2 : 1) +
                                (double)L.Cout * a.Ktot);

    int variant = -1;
    auto it = L.tuned.find(a.M);
    if (it != L.tuned.end()) variant = it->second;
    if (tuning && it == L.tuned.end()) DIR_CHECK(tune_conv(L, a, stream, &variant));
    // a tuning table written for another architecture shares layer names (resnet18 / resnet101 both
    // have layer1.0.conv1): an entry that does not fit this layer's shape is dropped, not an error
    a.ksplit = 0;   // (judged as a plain launch, like dir_conv_variant_admissible: not with the last timed candidate's split)
    if (variant >= 0 && !conv_variant_admissible(variant, a)) {
        L.tuned.erase(a.M);
        variant = -1;
    }
    if (variant < 0) variant = conv_pick_variant(a);
    a.ksplit = conv_splitk_factor(variant, a);
    return profiled(
        [&](std::string& name, std::string& kernel) {   // (the label strings are only built when somebody will read them)
            name = L.name;
            kernel = std::string("conv_igemm<") + conv_variant(variant).name + (a.ksplit > 1 ? "/k" + std::to_string(a.ksplit) : "") + ">";
        },
        2.0 * macs, bytes, stream, [&] { return conv_launch(a, kdtype(), variant, stream); });
}

// ---- one convolution on fp16 pairs (DIR_FP16P head, conv_pair.hip) -------------------------------------------------
int dir_engine::run_conv_pair(ConvLayer& L, const uint16_t* x, const uint16_t* x_lo, const uint16_t* res,
                              const uint16_t* res_lo, uint16_t* y, uint16_t* y_lo, int B, int H, int W, int OH, int OW,
                              hipStream_t stream, const uint16_t* x2, const uint16_t* x2_lo) {
    if (!L.dev.w_lo) return fail(DIR_ERR_STATE, "paired conv on a layer without a lo weight plane: " + L.name);
    if (x2 && !L.dev.w_ds_lo) return fail(DIR_ERR_STATE, "two-source paired conv without concatenated weights: " + L.name);
    ConvArgs a;
    conv_args_init(a, layer_geom(L, B, H, W, OH, OW), x, L.dev.w, L.dev.bias, res, y);
    a.x_lo = x_lo;
    a.w_lo = L.dev.w_lo;
    a.res_lo = res_lo;
    a.y_lo = y_lo;
    a.ovf = dev.ovf;
    if (x2) {   // conv3 + the block's stride-1 downsample: K = [t2 ; block input], weights / biases concatenated at finalize
        conv_args_second_source(a, x2, x2_lo, a.Cin);
        a.w = L.dev.w_ds;
        a.w_lo = L.dev.w_ds_lo;
        a.bias = L.dev.bias_ds;
    }
    const double macs = (double)a.M * L.Cout * (double)a.Ktot;
    // every tensor a pair: twice the bytes of the 16-bit form (single-plane operands counted once)
    const double bytes = 2.0 * ((double)B * H * W * a.Cin * (x_lo ? 2 : 1) * (x2 ? 2 : 1) + (double)a.M * L.Cout * (y_lo ? 2 : 1) +
                                (double)a.M * L.Cout * (res ? (res_lo ? 2 : 1) : 0) + 2.0 * L.Cout * a.Ktot);
    return profiled(
        [&](std::string& name, std::string& kernel) {
            name = x2 ? L.name.substr(0, L.name.rfind('.')) + ".ds+conv3" : L.name;
            kernel = std::string("conv_pair<") + conv_pair_variant_name(a) + ">";
        },
        2.0 * macs, bytes, stream, [&] { return conv_pair_launch(a, stream); });
}

// ---- DIR_FP16P: image -> stem -> the paired residual blocks ---------------------------------------------------------
// The reference's op sequence (ResNet.forward resnet.py:157-161, Bottleneck.forward :67-87 / BasicBlock :29-44), nothing
// fused across layers; every tensor two fp16 planes (hi in the ordinary workspace regions, lo in the lo_* regions).
int dir_engine::forward_pair_stem(const void* img, int B, int H, int W, int fmt, char* base, const Plan& p,
                                  hipStream_t stream) {
    uint16_t* s2d = (uint16_t*)(base + p.s2d);
    uint16_t* s2d_lo = (uint16_t*)(base + p.lo_s2d);
    uint16_t* y = (uint16_t*)(base + p.bufA);
    uint16_t* y_lo = (uint16_t*)(base + p.lo_stem);
    const double stem_flops = 2.0 * B * p.OH1 * p.OW1 * 64.0 * 147.0;
    const double out_bytes = 4.0 * ((double)B * p.PH * p.PW * 64 + 64 * 256);
    if (img && fmt == DIR_IMG_U8_NHWC && dev.stem_u8_w && !sw.no_stem_u8) {
        // the raw uint8 image is exact in ONE fp16 plane: Normalize folded into the filter pair and the bias, two MFMAs per
        // term, pooled in registers (stem_u8.hip)
        const bool raw = stem_pool_u8_raw_ok(img, B, H, W);   // the stem reads the image itself: no prep launch, no s2d plane
        if (!raw)
            DIR_CHECK(profiled("prep_input", "prep_input_u8", 0, (double)B * H * W * 3 + (double)B * p.H2 * p.W2 * 32, stream,
                               [&] { return prep_input_u8(img, s2d, B, H, W, stream); }));
        return profiled("conv1+maxpool", "stem_pool_u8", stem_flops,
                        (raw ? (double)B * H * W * 3 : 2.0 * (double)B * p.H2 * p.W2 * 16) + out_bytes, stream, [&] {
                            return stem_pool_u8_launch(raw ? img : nullptr, s2d, dev.stem_u8_w, dev.stem_u8_w_lo, dev.stem_u8_bias,
                                                       dev.stem_u8_corr, y, y_lo, B, H, W, stream, dev.ovf, sw.stem_u8_seg);
                        });
    }
    const bool raw_f32 = img && fmt == DIR_IMG_F32_NCHW && stem_pool_pair_raw_ok(img, B, H, W);   // the stem splits the fp32 image itself
    if (img && !raw_f32) {
        DIR_CHECK(profiled("prep_input", "prep_input_pair", 0,
                           (double)B * H * W * 3 * (fmt == DIR_IMG_U8_NHWC ? 1 : 4) + (double)B * p.H2 * p.W2 * 64, stream,
                           [&] { return prep_input_pair(img, fmt, desc.mean, desc.std, s2d, s2d_lo, B, H, W, stream); }));
    } else if (!img) {   // autotune: synthetic noise (the paired kernels themselves have nothing to tune)
        const long n = (long)B * p.H2 * p.W2 * 16;
        hipLaunchKernelGGL(fill_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, s2d, n, DIR_FP16);
        DIR_HIP_CHECK(hipGetLastError());
        DIR_HIP_CHECK(hipMemsetAsync(s2d_lo, 0, (size_t)n * 2, stream));
    }
    const ConvLayer::Dev& c = convs[0].dev;
    return profiled("conv1+maxpool", "stem_pool_pair", stem_flops,
                    (raw_f32 ? (double)B * H * W * 12 : 4.0 * (double)B * p.H2 * p.W2 * 16) + out_bytes, stream, [&] {
                        return raw_f32 ? stem_pool_pair_walk_launch(nullptr, nullptr, c.w, c.w_lo, c.bias, y, y_lo, B, p.H2, p.W2,
                                                                    p.OH1, p.OW1, stream, dev.ovf, img, H, W)
                                       : stem_pool_pair_launch(s2d, s2d_lo, c.w, c.w_lo, c.bias, y, y_lo, B, p.H2, p.W2, p.OH1,
                                                               p.OW1, stream, dev.ovf);
                    });
}

int dir_engine::forward_pair_head(const void* img, int B, int H, int W, int fmt, char* base, const Plan& p,
                                  hipStream_t stream, uint16_t** cur_out, int* h_out, int* w_out, size_t* next_block) {
    uint16_t* const pp[2] = {(uint16_t*)(base + p.bufA), (uint16_t*)(base + p.bufB)};
    uint16_t* stem_lo = (uint16_t*)(base + p.lo_stem);
    uint16_t* t1 = (uint16_t*)(base + p.t1);
    uint16_t* t2 = (uint16_t*)(base + p.t2);
    uint16_t* ds = (uint16_t*)(base + p.ds);
    uint16_t* t1_lo = (uint16_t*)(base + p.lo_t1);
    uint16_t* t2_lo = (uint16_t*)(base + p.lo_t2);
    uint16_t* ds_lo = (uint16_t*)(base + p.lo_ds);
    DIR_CHECK(forward_pair_stem(img, B, H, W, fmt, base, p, stream));
    int cur = 0;

    // pair_acts form.  Which tensors are pairs (tests/precision_decomposition.py prices every storage point): the image,
    // the stem output and everything INSIDE a block (t1, t2, the downsample branch) - the block outputs, 4P wide and read three times
    // each, are single fp16 planes: their rounding costs 7e-6 of the 1e-4 budget and a third of the head's bytes.
    int h = p.PH, w = p.PW;
    const size_t nb = std::min((size_t)pair_blocks, blocks.size());
    for (size_t bi = 0; bi < nb; ++bi) {
        BlockDef& bd = blocks[bi];
        const int oh = conv_out(h, 3, bd.stride, 1), ow = conv_out(w, 3, bd.stride, 1);
        const int nxt = cur ^ 1;
        const uint16_t* x = pp[cur];
        const uint16_t* x_lo = bi == 0 ? stem_lo : nullptr;
        const uint16_t *resid = x, *resid_lo = x_lo;
        // first block of a stage: the downsample rides in conv3's GEMM when it is pixel-aligned with t2 (stride 1, same
        // width: layer1); otherwise it is its own paired conv
        const bool fuse_ds = bd.down >= 0 && desc.bottleneck && convs[bd.conv3].dev.w_ds_lo != nullptr && x_lo != nullptr;
        if (bd.down >= 0 && !fuse_ds) {
            DIR_CHECK(run_conv_pair(convs[bd.down], x, x_lo, nullptr, nullptr, ds, ds_lo, B, h, w, oh, ow, stream));
            resid = ds;
            resid_lo = ds_lo;
        }
        if (desc.bottleneck) {
            DIR_CHECK(run_conv_pair(convs[bd.conv1], x, x_lo, nullptr, nullptr, t1, t1_lo, B, h, w, h, w, stream));
            DIR_CHECK(run_conv_pair(convs[bd.conv2], t1, t1_lo, nullptr, nullptr, t2, t2_lo, B, h, w, oh, ow, stream));
            if (fuse_ds)
                DIR_CHECK(run_conv_pair(convs[bd.conv3], t2, t2_lo, nullptr, nullptr, pp[nxt], nullptr, B, oh, ow, oh, ow, stream,
                                        x, x_lo));
            else
                DIR_CHECK(run_conv_pair(convs[bd.conv3], t2, t2_lo, resid, resid_lo, pp[nxt], nullptr, B, oh, ow, oh, ow, stream));
        } else {
            DIR_CHECK(run_conv_pair(convs[bd.conv1], x, x_lo, nullptr, nullptr, t1, t1_lo, B, h, w, oh, ow, stream));
            DIR_CHECK(run_conv_pair(convs[bd.conv2], t1, t1_lo, resid, resid_lo, pp[nxt], nullptr, B, oh, ow, oh, ow, stream));
        }
        cur = nxt;
        h = oh;
        w = ow;
    }
    *cur_out = pp[cur];
    *h_out = h;
    *w_out = w;
    *next_block = nb;
    return DIR_OK;
}

// ---- fused bottleneck seam ----------------------------------------------------------------------------
// The persistent seam kernel pays for loading both weight sets into registers once per workgroup: it wins from
// about 8 pixel tiles of 64 per workgroup (A/B at 1024^2: batch 1 = 1024 tiles: -2 %, batch 2: equal, batch 4:
// +4 %, batch 32: +6 %).
static constexpr long kSeamMinTiles = 2048;
static constexpr long kSeam3MinTiles = 768;   // conv_seam3.hip: three 64-pixel tiles per CU

// No side effects: builds the kernel's arguments in *a and says whether it takes this shape (forward asks before it launches
// the downsample that the DS form would fold in).
bool dir_engine::pick_seam(const ConvLayer& c3, const ConvLayer& c1, const uint16_t* t2, const uint16_t* res, uint16_t* y,
                           uint16_t* t1, int B, int H, int W, const uint16_t* block_in, const uint16_t* block_in_lo,
                           ConvArgs* ap, int y_keep_stride) const {
    ConvArgs& a = *ap;
    // DIRTORCH_AMD_C3C1: "0" = never (A/B and bisecting), "force" = whenever the shapes qualify, default =
    // when every persistent workgroup gets at least ~8 pixel tiles to amortise loading both weight sets
    if (sw.c3c1_off) return false;
    conv_args_init(a, layer_geom(c3, B, H, W, H, W), t2, c3.dev.w, c3.dev.bias, res, y);
    a.w_lo = c3.dev.w_lo;       // DIR_FP16P: the weights of layer1's 1x1s are pairs (conv_c3c1.hip WP3 / WP1)
    a.y_keep_stride = y_keep_stride;   // a stage exit: only the pixels the next block's strided downsample reads (forward decides)
    if (block_in) {   // DS form: the residual is the downsample conv of the block input, folded into this GEMM
        if (!c3.dev.w_ds || c3.Cin != 64) return false;   // (the caller checks the downsample's own shape)
        a.w = c3.dev.w_ds;
        a.w_lo = c3.dev.w_ds_lo;
        a.bias = c3.dev.bias_ds;
        a.res = nullptr;
        a.x2 = block_in;
        a.x2_lo = block_in_lo;
        a.Cin2 = 64;
        if ((c3.dev.w_lo != nullptr) != (a.w_lo != nullptr)) return false;   // (a paired conv3 without the concatenated lo plane)
    }
    conv_args_next_conv1(a, c1.dev.w, c1.dev.w_lo, c1.dev.bias, t1, c1.Cout, c1.relu ? 1 : 0);
    a.ovf = dev.ovf;
    if (c1.R != 1 || c1.S != 1 || c1.stride != 1 || c1.pad != 0 || c1.Cin != c3.Cout || !conv_c3c1_admissible(a))
        return false;
    // (the layer3 form streams its weights per tile anyway: it only needs a few tiles per persistent workgroup)
    if (!sw.c3c1_force && (a.M + 63) / 64 < (a.Cin == 256 ? kSeam3MinTiles : kSeamMinTiles)) return false;
    if (a.Cin == 256 && !sw.experiments) return false;   // conv_seam3.hip: experiments builds only (it loses: profiles/r04_seam3_ablation.txt)
    return true;
}

int dir_engine::run_seam(const ConvLayer& c3, const ConvLayer& c1, const ConvArgs& a, hipStream_t stream) {
    const bool ds = a.x2 != nullptr;
    const double macs = (double)a.M * ((double)c3.Cout * (c3.Cin + a.Cin2) + (double)c1.Cout * c1.Cin);
    // (block-output pixels actually stored: all of them, or every y_keep_stride-th row and column of each image)
    const int ks = a.y_keep_stride > 1 ? a.y_keep_stride : 1;
    const double m_stored = (double)a.B * ((a.H + ks - 1) / ks) * ((a.W + ks - 1) / ks);
    const double bytes = 2.0 * ((double)a.M * (c3.Cin + a.Cin2 * (a.x2_lo ? 2 : 1) + (ds ? 0.0 : 1.0) * c3.Cout + c1.Cout) +
                                m_stored * c3.Cout +
                                (double)c3.Cout * (c3.Cin + a.Cin2) * (a.w_lo ? 2 : 1) + (double)c1.Cout * c1.Cin * (a.w2_lo ? 2 : 1));
    return profiled(
        [&](std::string& name, std::string& kernel) {   // profile row "layerS.J.c3c1": conv3 of block J + conv1 of block J+1
            name = c3.name.substr(0, c3.name.rfind('.')) + (ds ? ".ds+c3c1" : ".c3c1");
            kernel = (c3.Cin == 256 ? "conv_seam3<" : "conv_c3c1<") + std::to_string(c3.Cin) + (ds ? ",ds" : "") +
                     (a.w_lo ? ",wp>" : ">");
        },
        2.0 * macs, bytes, stream, [&]() -> int {
            hipError_t e = conv_c3c1_launch(a, kdtype(), stream);
            if (e != hipSuccess) return fail(DIR_ERR_HIP, std::string("conv_c3c1 launch: ") + hipGetErrorString(e));
            return DIR_OK;
        });
}

// ---- conv3 + downsample as one two-source GEMM ------------------------------------------------------------
int dir_engine::pick_conv_dual(const ConvLayer& c3, const ConvLayer& ds, const uint16_t* t2, const uint16_t* xin, uint16_t* y,
                               int B, int Hin, int Win, int OH, int OW, ConvArgs* a) const {
    if (!c3.dev.w_ds || sw.no_dual || c3.dev.w_lo) return -1;   // (paired weights: conv_pair.hip has no strided two-source form)
    conv_args_init(*a, {B, OH, OW, c3.Cin, c3.Cout, 1, 1, 1, 0, OH, OW, c3.relu ? 1 : 0}, t2, c3.dev.w_ds, c3.dev.bias_ds, nullptr, y);
    a->ovf = dev.ovf;
    conv_args_second_source(*a, xin, nullptr, ds.Cin);
    a->H2 = Hin;
    a->W2 = Win;
    a->stride2 = ds.stride;
    return conv_pick_dual_variant(*a);
}

int dir_engine::run_conv_dual(const ConvLayer& c3, const ConvLayer& ds, const ConvArgs& a, int variant, hipStream_t stream) {
    const double macs = (double)a.M * c3.Cout * (double)a.Ktot;
    const double bytes = 2.0 * ((double)a.M * (c3.Cin + ds.Cin + c3.Cout) + (double)c3.Cout * a.Ktot);
    return profiled(
        [&](std::string& name, std::string& kernel) {
            name = c3.name.substr(0, c3.name.rfind('.')) + ".ds+conv3";
            // ("conv_igemm<VARIANT>" is the family label of every entry of the variant table; the variant name says
            // which kernel file runs it: 256x256_persist1x1_x3 = conv_persist.hip's deep-X ring, DUAL form)
            kernel = std::string("conv_igemm<") + conv_variant(variant).name + "/dual>";
        },
        2.0 * macs, bytes, stream, [&] { return conv_launch(a, kdtype(), variant, stream); });
}

// ---- forward ------------------------------------------------------------------------------------
int dir_engine::forward(const void* img, int B, int H, int W, int fmt, float* desc_out,
                        void* feat_out, int* fh, int* fw, int* fc, void* ws, size_t ws_bytes,
                        hipStream_t stream) {
    if (!finalized) return fail(DIR_ERR_STATE, "forward before finalize");
    int cur_dev = -1;
    DIR_HIP_CHECK(hipGetDevice(&cur_dev));
    if (cur_dev != device)   // the weights live on `device`; launching elsewhere would fault
        return fail(DIR_ERR_STATE, "forward: the current HIP device (" + std::to_string(cur_dev) +
                                       ") is not the engine's device (" + std::to_string(device) + ")");
    Plan p;
    DIR_CHECK(plan(B, H, W, &p));
    if (!ws || ws_bytes < p.total)
        return fail(DIR_ERR_WORKSPACE, "workspace too small: need " + std::to_string(p.total) +
                                           " bytes, got " + std::to_string(ws_bytes));
    if (((uintptr_t)ws & 255) != 0) return fail(DIR_ERR_INVALID, "workspace must be 256-byte aligned");
    char* base = (char*)ws;
    splitk_scratch = (float*)(base + p.splitk);
    if (dtype == DIR_F32) return forward_f32(img, B, H, W, fmt, desc_out, feat_out, fh, fw, fc, base, p, stream);
    uint16_t* s2d = (uint16_t*)(base + p.s2d);
    uint16_t* stem = (uint16_t*)(base + p.stem);
    uint16_t* cur = (uint16_t*)(base + p.bufA);
    uint16_t* nxt = nullptr;
    uint16_t* t1 = (uint16_t*)(base + p.t1);
    uint16_t* t2 = (uint16_t*)(base + p.t2);
    uint16_t* ds = (uint16_t*)(base + p.ds);
    float* pooled = (float*)(base + p.pooled);
    float* fcout = (float*)(base + p.fcout);

    const int kd = kdtype();
    int h = 0, w = 0;
    size_t first_block = 0;
    const uint16_t* cur_lo = nullptr;   // lo plane of the block input (DIR_FP16P: the stem's pooled output)
    if (dtype == DIR_FP16P && pair_acts) {
        // 1-2'. paired head: image, stem and the first pair_blocks residual blocks on fp16 pairs (conv_pair.hip)
        DIR_CHECK(forward_pair_head(img, B, H, W, fmt, base, p, stream, &cur, &h, &w, &first_block));
    } else if (dtype == DIR_FP16P) {
        // 1-2''. image and stem on pairs; the blocks run below on single fp16 planes, with paired 1x1 WEIGHTS in layer1
        DIR_CHECK(forward_pair_stem(img, B, H, W, fmt, base, p, stream));
        cur_lo = (const uint16_t*)(base + p.lo_stem);
        h = p.PH;
        w = p.PW;
    } else {
        // 1. image -> space-to-depth NHWC16
        if (img) {
            DIR_CHECK(profiled("prep_input", "prep_input", 0,
                               (double)B * H * W * 3 * (fmt == DIR_IMG_U8_NHWC ? 1 : 4) + (double)B * p.H2 * p.W2 * 32, stream,
                               [&] { return prep_input(img, fmt, desc.mean, desc.std, s2d, B, H, W, kd, stream); }));
        } else {  // autotune: synthetic noise straight into the s2d buffer
            const long n = (long)B * p.H2 * p.W2 * 16;
            hipLaunchKernelGGL(fill_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                               s2d, n, kd);
            DIR_HIP_CHECK(hipGetLastError());
        }
        // 2. stem + maxpool: one kernel (stem_pool.hip) unless DIRTORCH_AMD_UNFUSED_STEM=1
        if (sw.unfused_stem) {
            DIR_CHECK(run_conv(convs[0], s2d, nullptr, stem, B, p.H2, p.W2, p.OH1, p.OW1, stream));
            DIR_CHECK(profiled("maxpool", "maxpool_3x3s2", 0, 2.0 * ((double)B * p.OH1 * p.OW1 * 64 + (double)B * p.PH * p.PW * 64),
                               stream, [&] { return maxpool_3x3s2(stem, cur, B, p.OH1, p.OW1, 64, kd, stream); }));
        } else {
            DIR_CHECK(profiled("conv1+maxpool", "stem_pool", 2.0 * B * p.OH1 * p.OW1 * 64.0 * 147.0,
                               2.0 * ((double)B * p.H2 * p.W2 * 16 + (double)B * p.PH * p.PW * 64 + 64 * 256), stream, [&] {
                                   return stem_pool_launch(s2d, convs[0].dev.w, convs[0].dev.bias, cur, B, p.H2, p.W2, p.OH1, p.OW1, kd,
                                                           stream, dev.ovf);
                               }));
        }
        h = p.PH;
        w = p.PW;
    }

    // 3. residual stages (two ping-pong buffers; the FPN heads park layer3's output in its own buffer)
    uint16_t* const pp[2] = {(uint16_t*)(base + p.bufA), (uint16_t*)(base + p.bufB)};
    uint16_t* x4 = nullptr;
    int h4 = 0, w4 = 0;
    bool t1_ready = false;
    for (size_t bi = first_block; bi < blocks.size(); ++bi) {
        BlockDef& bd = blocks[bi];
        const int oh = conv_out(h, 3, bd.stride, 1), ow = conv_out(w, 3, bd.stride, 1);
        const bool keep = (int)bi == x4_block;
        nxt = keep ? (uint16_t*)(base + p.x4) : (cur == pp[0] ? pp[1] : pp[0]);
        // The identity blocks of layers 2-4 write their output OVER their input (layers 3-4 since round 5; layer2 - its seams and
        // its last, plain conv3 - since the stage-exit store; DIRTORCH_AMD_NO_INPLACE restores the
        // ping-pong).  Safe and bit-identical: conv3 reads every residual element it adds before it stores that element - conv_wreg
        // and the seam (conv_c3c1.hip) one strip ahead in registers, conv_persist / conv_pair / the tiled kernels the whole tile
        // before the K loop, the split-K finalize
        // element by element - and no other workgroup touches it (conv3's INPUT is t2).  Layer1's seams were measured in place as
        // well and gain nothing (0.499-0.501 against 0.496-0.501 ms, profiles/seam_stores.txt): they keep the ping-pong.
        // Found while pricing Infinity-Cache
        // residency (profiles/r05_mall_probe.txt: the cache itself buys nothing), kept for what it does in HBM: a
        // read-modify-write stream gets 5.6-5.9 TB/s where a copy gets 5.2-5.4 - layer3's conv3 110 -> 104 us, step 14.03 -> 13.96 ms
        // (A/B on one box) - and layer3's footprint in the workspace halves.
        if (!sw.no_inplace && desc.bottleneck && bd.down < 0 && !keep && !tuning && convs[bd.conv3].Cin >= 128) nxt = cur;
        const uint16_t* resid = cur;
        // How a first block's downsample runs is decided here, before anything launches.  In layer1 it can ride in the seam
        // kernel as extra K (conv_c3c1.hip, DS form), if pick_seam says that kernel will run for this shape: the next
        // block's conv1 is 1x1 stride 1 even across a stage boundary (the stride sits in conv2), but the DS form needs it 64
        // wide, so a layer1 of a single block, followed by layer2's 128-wide conv1, does not qualify; nor does a batch too
        // large for the kernel, which is left to conv_launch's own 2^31-byte error.  Otherwise the downsample joins conv3 in a
        // two-source GEMM (pick_conv_dual), or else runs as its own launch.
        const bool seam_next = desc.bottleneck && bi + 1 < blocks.size() && !tuning;
        // A stage exit: when the seam produces the next block's conv1, the only reader left of this block's output is that
        // block's downsample - 1x1, no padding, stride s > 1: pixel (oh * s, ow * s) for output pixel (oh, ow), in every kernel
        // that can run it (the two-source forms of conv_wregd / conv_persist / conv_persistlc, or its own launch on conv_igemm's
        // tiles, conv_small or conv_pair).  The seam then stores only those pixels (ConvArgs::y_keep_stride;
        // DIRTORCH_AMD_SEAM_FULL_STORE: all of them again).  Not when the output is kept for the FPN head; the last block has no seam.
        int keep_stride = 0;
        // (planes <= 128: the register-stationary seam; the experiments builds' layer3 seam stores every pixel)
        if (seam_next && !keep && !sw.seam_full_store && bd.down < 0 && blocks[bi + 1].down >= 0 && convs[bd.conv3].Cin <= 128) {
            const ConvLayer& nd = convs[blocks[bi + 1].down];
            if (nd.R == 1 && nd.S == 1 && nd.pad == 0 && nd.stride > 1) keep_stride = nd.stride;
        }
        ConvArgs seam;
        bool ds_in_seam = false;
        if (bd.down >= 0 && seam_next && !sw.no_ds_seam && convs[bd.down].Cin == 64 && convs[bd.down].stride == 1)
            ds_in_seam = pick_seam(convs[bd.conv3], convs[blocks[bi + 1].conv1], t2, nullptr, nxt, t1, B, oh, ow, cur, cur_lo, &seam);
        ConvArgs dual;   // the other stages' first blocks (conv_persist.hip, DUAL)
        int dual_variant = -1;
        if (bd.down >= 0 && !ds_in_seam && desc.bottleneck && !tuning && !cur_lo)
            dual_variant = pick_conv_dual(convs[bd.conv3], convs[bd.down], t2, cur, nxt, B, h, w, oh, ow, &dual);
        if (bd.down >= 0 && !ds_in_seam && dual_variant < 0) {
            DIR_CHECK(cur_lo ? run_conv_pair(convs[bd.down], cur, cur_lo, nullptr, nullptr, ds, nullptr, B, h, w, oh, ow, stream)
                             : run_conv(convs[bd.down], cur, nullptr, ds, B, h, w, oh, ow, stream));
            resid = ds;
        }
        if (desc.bottleneck) {
            if (!t1_ready)   // (the previous block's fused seam kernel may have produced t1 already)
                DIR_CHECK(cur_lo ? run_conv_pair(convs[bd.conv1], cur, cur_lo, nullptr, nullptr, t1, nullptr, B, h, w, h, w, stream)
                                 : run_conv(convs[bd.conv1], cur, nullptr, t1, B, h, w, h, w, stream, sw.rev_conv1));
            t1_ready = false;
            DIR_CHECK(run_conv(convs[bd.conv2], t1, nullptr, t2, B, h, w, oh, ow, stream));
            if (dual_variant >= 0) {   // (block output written; the next block's conv1 still has to run)
                DIR_CHECK(run_conv_dual(convs[bd.conv3], convs[bd.down], dual, dual_variant, stream));
            } else if (seam_next && (ds_in_seam || pick_seam(convs[bd.conv3], convs[blocks[bi + 1].conv1], t2, resid, nxt, t1, B, oh,
                                                             ow, nullptr, nullptr, &seam, keep_stride))) {
                // conv3 + the next block's conv1 in one kernel: the block output is not re-read (conv_c3c1.hip)
                DIR_CHECK(run_seam(convs[bd.conv3], convs[blocks[bi + 1].conv1], seam, stream));
                t1_ready = true;
            } else {
                DIR_CHECK(run_conv(convs[bd.conv3], t2, resid, nxt, B, oh, ow, oh, ow, stream, sw.rev_conv3));
            }
        } else {
            DIR_CHECK(run_conv(convs[bd.conv1], cur, nullptr, t1, B, h, w, oh, ow, stream));
            DIR_CHECK(run_conv(convs[bd.conv2], t1, resid, nxt, B, oh, ow, oh, ow, stream));
        }
        cur = nxt;
        cur_lo = nullptr;   // block outputs are single planes in every mode
        h = oh;
        w = ow;
        if (keep) {
            x4 = cur;
            h4 = h;
            w4 = w;
        }
    }
    if (feat_out) {
        DIR_HIP_CHECK(hipMemcpyAsync(feat_out, cur, (size_t)B * h * w * feat_dim * 2,
                                     hipMemcpyDeviceToDevice, stream));
        if (fh) *fh = h;
        if (fw) *fw = w;
        if (fc) *fc = feat_dim;
    }
    if (!desc_out) return DIR_OK;

    // 4. head (rmac_resnet.py:58-68; rmac_resnet_fpn.py:53-86; resnet.py:169-173)
    const bool fpn = x4 != nullptr;
    const bool classifier = desc.head == DIR_HEAD_CLASSIFIER;
    if (fpn) {
        const uint16_t* c4 = x4;
        if (conv1x5 >= 0) {
            uint16_t* sum = cur == pp[0] ? pp[1] : pp[0];
            DIR_CHECK(run_conv(convs[conv1x5], cur, nullptr, t1, B, h, w, h, w, stream));
            DIR_CHECK(profiled("x4+up(c5)", "upsample_add", 0, 2.0 * ((double)B * h4 * w4 * x4_dim * 2 + (double)B * h * w * x4_dim),
                               stream, [&] { return upsample_add(x4, t1, sum, B, h4, w4, h, w, x4_dim, kd, stream, dev.ovf); }));
            DIR_CHECK(run_conv(convs[conv3c4], sum, nullptr, t2, B, h4, w4, h4, w4, stream));
            c4 = t2;
        }
        DIR_CHECK(profiled("adpoolc4", "global_pool", 0, (double)B * h4 * w4 * x4_dim * 2, stream, [&] {
            return global_pool(c4, pooled, head_dim, B, h4, w4, x4_dim, DIR_POOL_GEM, gem_p4, 1e-6f, 0.f, kd, stream);
        }));
    }
    // the FPN forward never applies center_bias (rmac_resnet_fpn.py:50-86), the classifier averages
    DIR_CHECK(profiled(fpn ? "adpoolx5" : "adpool", "global_pool", 0, (double)B * h * w * feat_dim * 2 + (double)B * feat_dim * 4,
                       stream, [&] {
                           return global_pool(cur, pooled + (fpn ? x4_dim : 0), head_dim, B, h, w, feat_dim,
                                              classifier ? DIR_POOL_AVG : desc.pooling, gem_p, 1e-6f,
                                              (fpn || classifier) ? 0.f : desc.center_bias, kd, stream);
                       }));
    return finish_descriptor(pooled, fcout, B, desc_out, stream);
}

// ---- what follows pooling, in every dtype: (L2) -> FC (fp32 MFMA) -> L2 -> the caller's buffer ------------------------------
int dir_engine::finish_descriptor(float* pooled, float* fcout, int B, float* desc_out, hipStream_t stream) {
    const bool classifier = desc.head == DIR_HEAD_CLASSIFIER;
    if (desc.norm_features && !classifier) DIR_CHECK(l2norm_rows(pooled, B, head_dim, 1e-12f, stream));
    const int D = desc.without_fc ? head_dim : desc.out_dim;
    if (!desc.without_fc) {
        DIR_CHECK(profiled("fc", "gemm_nt_f32", 2.0 * B * head_dim * (double)D,
                           4.0 * ((double)D * head_dim + (double)B * (head_dim + D)), stream, [&] {
                               return gemm_nt_f32(dev.fc_w, head_dim, pooled, head_dim, fcout, D, D, B, head_dim, nullptr, dev.fc_b,
                                                  nullptr, stream, splitk_scratch, kSplitKMaxBytes);   // the convs are done with it
                           }));
    } else {
        fcout = pooled;
    }
    if (!classifier) DIR_CHECK(l2norm_rows(fcout, B, D, 1e-12f, stream));
    DIR_HIP_CHECK(hipMemcpyAsync(desc_out, fcout, (size_t)B * D * 4, hipMemcpyDeviceToDevice, stream));
    return DIR_OK;
}

// ---- the strict path: fp32 storage, fp32 matrix cores (conv_f32.hip) --------------------------------------------
// The reference's op sequence one to one (ResNet.forward resnet.py:157-174, Bottleneck.forward :67-87,
// ResNet_RMAC.forward rmac_resnet.py:39-69), eval-mode BatchNorm folded into fp32 weights, bias / residual / ReLU in
// the conv epilogue, nothing fused across layers.  Differences from the reference's fp32 CPU result are summation
// order only.
int dir_engine::run_conv_f32(ConvLayer& L, const float* x, const float* res, float* y, int B, int H, int W, int OH,
                             int OW, hipStream_t stream) {
    ConvF32Args a;
    conv_geom_fill(a, layer_geom(L, B, H, W, OH, OW), x, L.dev.wf, L.dev.bias, res, y);
    const double macs = (double)a.M * L.Cout * (double)(L.R * L.S * L.Cin);
    const double bytes = 4.0 * ((double)B * H * W * a.Cin + (double)a.M * L.Cout * (res ? 2 : 1) + (double)L.Cout * a.Ktot);
    return profiled(
        [&](std::string& name, std::string& kernel) {
            name = L.name;
            kernel = std::string("conv_f32<") + (L.Cout <= 64 ? "128x64" : "128x128") + ">";
        },
        2.0 * macs, bytes, stream, [&] { return conv_f32_launch(a, stream); });
}

int dir_engine::forward_f32(const void* img, int B, int H, int W, int fmt, float* desc_out, void* feat_out, int* fh,
                            int* fw, int* fc, char* base, const Plan& p, hipStream_t stream) {
    float* s2d = (float*)(base + p.s2d);
    float* stem = (float*)(base + p.stem);
    float* t1 = (float*)(base + p.t1);
    float* t2 = (float*)(base + p.t2);
    float* ds = (float*)(base + p.ds);
    float* pooled = (float*)(base + p.pooled);
    float* fcout = (float*)(base + p.fcout);
    float* const pp[2] = {(float*)(base + p.bufA), (float*)(base + p.bufB)};
    if (!img) return fail(DIR_ERR_INVALID, "autotune has nothing to choose in the fp32 path");
    DIR_CHECK(profiled("prep_input", "prep_input_f32", 0,
                       (double)B * H * W * 3 * (fmt == DIR_IMG_U8_NHWC ? 1 : 4) + (double)B * p.H2 * p.W2 * 64, stream,
                       [&] { return prep_input_f32(img, fmt, desc.mean, desc.std, s2d, B, H, W, stream); }));
    DIR_CHECK(run_conv_f32(convs[0], s2d, nullptr, stem, B, p.H2, p.W2, p.OH1, p.OW1, stream));
    float* cur = pp[0];
    DIR_CHECK(profiled("maxpool", "maxpool_f32", 0, 4.0 * ((double)B * p.OH1 * p.OW1 * 64 + (double)B * p.PH * p.PW * 64), stream,
                       [&] { return maxpool_3x3s2_f32(stem, cur, B, p.OH1, p.OW1, 64, stream); }));

    float* x4 = nullptr;
    int h = p.PH, w = p.PW, h4 = 0, w4 = 0;
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
        BlockDef& bd = blocks[bi];
        const int oh = conv_out(h, 3, bd.stride, 1), ow = conv_out(w, 3, bd.stride, 1);
        const bool keep = (int)bi == x4_block;
        float* nxt = keep ? (float*)(base + p.x4) : (cur == pp[0] ? pp[1] : pp[0]);
        const float* resid = cur;
        if (bd.down >= 0) {
            DIR_CHECK(run_conv_f32(convs[bd.down], cur, nullptr, ds, B, h, w, oh, ow, stream));
            resid = ds;
        }
        if (desc.bottleneck) {
            DIR_CHECK(run_conv_f32(convs[bd.conv1], cur, nullptr, t1, B, h, w, h, w, stream));
            DIR_CHECK(run_conv_f32(convs[bd.conv2], t1, nullptr, t2, B, h, w, oh, ow, stream));
            DIR_CHECK(run_conv_f32(convs[bd.conv3], t2, resid, nxt, B, oh, ow, oh, ow, stream));
        } else {
            DIR_CHECK(run_conv_f32(convs[bd.conv1], cur, nullptr, t1, B, h, w, oh, ow, stream));
            DIR_CHECK(run_conv_f32(convs[bd.conv2], t1, resid, nxt, B, oh, ow, oh, ow, stream));
        }
        cur = nxt;
        h = oh;
        w = ow;
        if (keep) {
            x4 = cur;
            h4 = h;
            w4 = w;
        }
    }
    if (feat_out) {
        DIR_HIP_CHECK(hipMemcpyAsync(feat_out, cur, (size_t)B * h * w * feat_dim * 4, hipMemcpyDeviceToDevice, stream));
        if (fh) *fh = h;
        if (fw) *fw = w;
        if (fc) *fc = feat_dim;
    }
    if (!desc_out) return DIR_OK;

    const bool fpn = x4 != nullptr;
    const bool classifier = desc.head == DIR_HEAD_CLASSIFIER;
    if (fpn) {
        const float* c4 = x4;
        if (conv1x5 >= 0) {
            float* sum = cur == pp[0] ? pp[1] : pp[0];
            DIR_CHECK(run_conv_f32(convs[conv1x5], cur, nullptr, t1, B, h, w, h, w, stream));
            DIR_CHECK(upsample_add_f32(x4, t1, sum, B, h4, w4, h, w, x4_dim, stream));
            DIR_CHECK(run_conv_f32(convs[conv3c4], sum, nullptr, t2, B, h4, w4, h4, w4, stream));
            c4 = t2;
        }
        DIR_CHECK(global_pool_f32(c4, pooled, head_dim, B, h4, w4, x4_dim, DIR_POOL_GEM, gem_p4, 1e-6f, 0.f, stream));
    }
    DIR_CHECK(profiled(fpn ? "adpoolx5" : "adpool", "global_pool_f32", 0, (double)B * h * w * feat_dim * 4 + (double)B * feat_dim * 4,
                       stream, [&] {
                           return global_pool_f32(cur, pooled + (fpn ? x4_dim : 0), head_dim, B, h, w, feat_dim,
                                                  classifier ? DIR_POOL_AVG : desc.pooling, gem_p, 1e-6f,
                                                  (fpn || classifier) ? 0.f : desc.center_bias, stream);
                       }));
    return finish_descriptor(pooled, fcout, B, desc_out, stream);
}
