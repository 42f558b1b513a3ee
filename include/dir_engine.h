/*
 * dir_engine.h — C ABI of the MI355X (gfx950) descriptor-extraction + ranking engine.
 *
 * The reference (naver/deep-image-retrieval, "dirtorch") has no FFI of its own: its seam is the
 * duck-typed Python object returned by dirtorch.nets.create_model (dirtorch/nets/__init__.py:24-64)
 * plus four free functions of dirtorch/utils/common.py.  Every entry point below names the
 * reference call it replaces.  The host side (Python, ctypes) lives in
 * deep-image-retrieval_amd/dirtorch_amd/ and mirrors the reference names one to one.
 *
 * Conventions
 *   - every function returns DIR_OK (0) or a negative dir_status; the message of the last error on
 *     the calling thread is returned by dir_last_error().  No C++ exception crosses this boundary.
 *   - all tensor pointers are DEVICE pointers owned by the caller unless the name says host_;
 *     `stream` is a hipStream_t passed as void* (NULL = the default stream).  Nothing here
 *     synchronises the device except dir_engine_finalize and the profiling getters.
 *   - activations are NHWC, 16-bit (bf16 or fp16; DIR_FP16P: pairs of fp16 planes in the stem and layer1) or fp32
 *     (DIR_F32, the strict path), chosen at finalize; accumulation is always fp32.
 *   - the engine owns only its packed weights; the caller owns images, descriptors and workspace.
 *   - one handle per device, ONE calling thread at a time (the reference calls net(x) from one thread,
 *     dirtorch/test_dir.py:67-81).  That thread may keep several dir_forward calls in flight on DIFFERENT streams of the
 *     device (the host mirror overlaps batch-1 forwards on four, dirtorch_amd/test_dir.py StreamPool): every per-forward
 *     mutable state is host-side and each call takes its own caller-owned workspace - one workspace per stream.  Two
 *     things are per handle, not per stream: the overflow word (join all streams before dir_engine_overflow) and the
 *     profile records (enable profiling with forwards on a single stream only - events of several streams interleave).
 */
#ifndef DIR_ENGINE_H
#define DIR_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dir_status {
    DIR_OK = 0,
    DIR_ERR_INVALID = -1,     /* bad argument / unsupported configuration            */
    DIR_ERR_STATE = -2,       /* call out of order (e.g. forward before finalize)    */
    DIR_ERR_MISSING = -3,     /* a state-dict tensor was never supplied              */
    DIR_ERR_WORKSPACE = -4,   /* workspace too small                                 */
    DIR_ERR_HIP = -5,         /* a HIP runtime call failed                           */
    DIR_ERR_NOMEM = -6,
    DIR_ERR_RANGE = -7        /* a finite fp32 weight does not fit the chosen 16-bit format  */
} dir_status;

/* Storage format of activations and weights, chosen at dir_engine_finalize (the C ABI has no default; the Python
 * host mirror defaults to fp16, bench.py measures bf16 = BASELINE configs[1] and reports the other two beside it).
 * Accumulation is fp32 in all three. */
typedef enum dir_dtype {
    DIR_BF16 = 0,             /* bf16 storage, bf16 MFMA: fp32's exponent range, 8-bit mantissa               */
    DIR_FP16 = 1,             /* fp16 storage, fp16 MFMA: 11-bit mantissa, saturates at 65504 (dir_engine_overflow) */
    DIR_F32 = 2,              /* STRICT: fp32 storage and products on the fp32 matrix cores (conv_f32.hip) - the
                                 reference's own arithmetic up to summation order; ~1/8 of the 16-bit throughput */
    DIR_FP16P = 3             /* fp16 with a PAIRED head: where a conditioned network makes ~94 % of its 16-bit rounding
                                 error (the image, the stem, layer1) values are kept as pairs of fp16 planes (v ~ hi + lo,
                                 ~22 bits) and multiplied with two or three fp16 MFMAs per term - the image, the stem's
                                 weights and pooled output, and the weights of layer1's 1x1 convs (conv_pair.hip,
                                 conv_c3c1.hip WP); everything else is DIR_FP16.  Meets the 1e-4 cosine bar on
                                 BatchNorm-calibrated checkpoints (3.3e-5 ... 4.3e-5) at ~94 % of the fp16 throughput.
                                 Read at finalize: DIRTORCH_AMD_PAIR_ACTS=1 also pairs layer1's 3x3 weights and the
                                 tensors inside its blocks (1.5e-5 ... 1.7e-5, ~83 %; always on for BasicBlock nets),
                                 DIRTORCH_AMD_PAIR_STAGES=1..4 extends the paired region to later stages. */
} dir_dtype;

typedef enum dir_img_format {
    DIR_IMG_F32_NCHW = 0,     /* what the reference feeds net(x): normalised fp32 NCHW
                                 (dirtorch/utils/transforms.py:617-623 ToTensor+Normalize) */
    DIR_IMG_U8_NHWC = 1       /* raw uint8 HWC pixels; (x/255-mean)/std is fused on device  */
} dir_img_format;

typedef enum dir_pooling {    /* dirtorch/nets/rmac_resnet.py:24-31                         */
    DIR_POOL_GEM = 0,
    DIR_POOL_MAX = 1,
    DIR_POOL_AVG = 2
} dir_pooling;

typedef enum dir_head {       /* what follows the trunk                                     */
    DIR_HEAD_RMAC = 0,        /* ResNet_RMAC: pool -> (L2) -> FC -> L2 (rmac_resnet.py:39-69)       */
    DIR_HEAD_FPN = 1,         /* ResNet_RMAC_FPN mode 1: c4 = relu(conv3c4(x4 + up(relu(conv1x5(x5)))));
                                 GeM(c4) ++ GeM(x5) -> (L2) -> FC -> L2 (rmac_resnet_fpn.py:50-86)  */
    DIR_HEAD_FPN0 = 2,        /* mode 0 (resnet101_fpn0_rmac): GeM(x4) ++ GeM(x5), no lateral convs */
    DIR_HEAD_CLASSIFIER = 3   /* plain ResNet: avgpool -> FC, no L2 (backbones/resnet.py:169-174)   */
} dir_head;

/* Mirrors the keyword arguments of ResNet_RMAC.__init__ (dirtorch/nets/rmac_resnet.py:15-17)
 * and the layer counts of the resnet{18,50,101,152}_rmac factories (:74-88). */
typedef struct dir_model_desc {
    int   bottleneck;         /* 1 = Bottleneck blocks (R50/101/152), 0 = BasicBlock (R18)  */
    int   layers[4];          /* blocks per stage, e.g. {3,4,23,3}                          */
    int   out_dim;            /* FC output size (2048)                                      */
    int   norm_features;      /* L2 over channels before the FC                             */
    int   pooling;            /* dir_pooling                                                */
    int   without_fc;         /* skip the FC                                                */
    float center_bias;        /* >0: bilinear 4x4 centre mask before pooling (:52-56)       */
    float mean[3];            /* used by DIR_IMG_U8_NHWC only                               */
    float std[3];
    int   head;               /* dir_head; FPN heads need pooling == DIR_POOL_GEM and read the
                                 keys conv1x5.weight, conv3c4.weight, adpoolx5.p, adpoolc4.p   */
} dir_model_desc;

typedef struct dir_engine dir_engine;

const char* dir_last_error(void);
/* "dir_engine <version> gfx950" — lets the host check it loaded the library it expects. */
const char* dir_version(void);
/* Launch extents (host-only query).  A dispatch holds gridDim.x * blockDim.x as a 32-bit count of threads, so no launch of
 * this library exceeds dir_launch_max_threads() = 2^32 - 256 threads, nor 65535 on gridDim.y.  An entry whose launch follows
 * a caller's size states the size it refuses below ("launch limit:"): such a call fails with DIR_ERR_INVALID and a message
 * that names the entry and the product, before anything is launched.  dir_gather_scores cuts its work into several launches
 * instead and takes any Q * R.  Entries that state none are held below the limit by their other rules (int sizes, k and M
 * maxima, the 2^31-byte rule of an engine call).
 * launch limit, per entry (L = dir_launch_max_threads(); "<=" is what a call may have):
 *   dir_prep_input           B * ceil(H / 2) * ceil(W / 2) <= L
 *   dir_maxpool_3x3s2        B * PH * PW * C / 8 <= L
 *   dir_global_pool          C * 4 <= L, B <= 65535
 *   dir_upsample_add         B * H * W * C / 8 <= L
 *   dir_resize_bilinear_u8   B * H * OW * 3 <= L where OW != W, B * OH * OW * 3 <= L where OH != H
 *   dir_l2norm_rows          rows * 256 <= L
 *   dir_multiscale_pool      N * D <= L
 *   dir_gemm_nt_f32          NP * 32 <= L on the few-row form (NQ <= 32, K <= 2048, aligned), else
 *                            ceil(NP / 128) * ceil(NQ / (32 .. 128)) * 256 <= L; dir_fc_l2, dir_pca_whiten_l2*, dir_similarity*
 *                            and dir_expand_descriptors inherit it (their split forms turn away what does not fit and leave
 *                            the shape to this one)
 *   dir_rank_counts          Q <= 65535
 *   dir_revisitop_ap         Q * 256 <= L, modes <= 65535
 *   dir_label_rank           Q * 512 <= L
 *   dir_expand_descriptors   min(n, rows the scratch holds) * 256 <= L
 *   dir_expand_lists         n * 256 <= L
 *   dir_quantize_rows_i8     N * 64 <= L (N rounded up to 4)
 *   dir_similarity_i8        N * 3 <= L (N rounded up to 256), Q <= 65535 * 96
 *   dir_gather_scores        none: several launches
 *   dir_quantize_rows_fp4    N * 64 <= L (N rounded up to 4)
 *   dir_similarity_fp4       N * 3 <= L (N rounded up to 256), Q <= 65535 * 96
 *   dir_quantize_rows_bin    N * 64 <= L (N rounded up to 4)
 *   dir_similarity_bin       N * 3 <= L (N rounded up to 256), Q <= 65535 * 96
 *   dir_segment_sums         S <= 65535
 *   dir_ivf_scan_i8          Q * width <= L, items * 768 <= L (refused, not cut: Q * width of 2^32 means 32 GiB of score and id
 *                            rows for one chunk; index.py's chunks are scratch_bytes / 8 slots, 2^25 by default)
 *   dir_ivf_scan_fp4         Q * width <= L, items * 768 <= L (refused, not cut, as dir_ivf_scan_i8)
 *   dir_code_sums            Q * 64 <= L (Q rounded up to 4)
 *   dir_ivf_scan_bin         Q * width <= L, items * 768 <= L (refused, not cut, as dir_ivf_scan_i8)
 *   dir_pq_encode            N * M <= L (N rounded up to 256)
 *   dir_pq_lut               Q * M * 8 <= L (Q rounded up to 32)
 *   dir_ivfpq_base           Q * nprobe * 128 <= L
 *   dir_ivfpq_scan           Q * width <= L (width rounded up to 1024)
 *   dir_knn_graph            N * k <= L
 *   dir_diffusion_seed       N * Q <= L
 *   dir_diffusion_solve      N * Q <= L, Q <= 65535 * 64
 *   dir_diffusion_subgraph   Q * 1024 <= L (a workgroup per query); dir_diffusion_solve_local the same
 *   dir_diffusion_spread     Q * N <= L, Q * T <= L */
int64_t dir_launch_max_threads(void);
/* The DIRTORCH_AMD_* A/B switches (kernel-selection toggles for bisecting; no reference counterpart - the reference reads no
 * environment on this path) are read from the environment ONCE, at the library's first use, and copied into an engine at
 * dir_engine_create.  A host that changes one of them afterwards (tests, A/B scripts) calls this to re-read them.  Two lifetimes:
 *   per ENGINE (copied at dir_engine_create; an existing engine keeps what it was created with):  _C3C1, _NO_DS_SEAM, _NO_DUAL,
 *       _REV_CONV1 / _REV_CONV3, _UNFUSED_STEM, _PAIR_ACTS, _PAIR_STAGES (the last two take effect at dir_engine_finalize),
 *       _NO_INPLACE, _SEAM_FULL_STORE, _NO_STEM_U8, _STEM_U8_SEG, _EXPERIMENTS (which kernels a forward may consider)
 *   per PROCESS (read from the current snapshot at every launch, by engines and by the per-op entry points alike):  the kernel
 *       pickers' _NO_PATCHLC / _NO_WREG / _NO_WREGD / _NO_SMALLMAP / _SMALL_K2 / _NO_C3C1LC / _LC1X1 / _X3_K2048 / _NO_PATCHS2 / _PATCHW_PACK / _NO_PATCHW_PACK / _NO_PATCHW / _NO_PATCHW_LC / _NO_X3 / _NO_PATCHS / _NO_PAIR_PATCH / _NO_XCDMAP,
 *       _STEM_V1, _STEM_PAIR_OLD, _STEM_U8_PREP, _STEM_U8_WG8, _SIM_V1, _SIM_EXACT
 * The re-read builds a new snapshot and publishes it with one atomic store (a launch sees the old set or the new one, never a
 * mixture); still, do not call it while another thread is launching if that thread's A/B comparison matters. */
int dir_reload_env(void);

/* ---- model life cycle: replaces nets.create_model + net.load_state_dict + net.cuda() ------- */
/* dirtorch/nets/__init__.py:24-64, dirtorch/test_dir.py:183-191 */
int dir_engine_create(const dir_model_desc* desc, int device, dir_engine** out);
int dir_engine_destroy(dir_engine* e);
/* One call per state-dict entry, reference key names (conv1.weight, bn1.running_mean,
 * layer3.7.conv2.weight, layer2.0.downsample.1.bias, adpool.p, fc.weight, fc.bias, …), host fp32,
 * PyTorch layouts (OIHW for convs).  num_batches_tracked entries are accepted and ignored. */
int dir_engine_set_tensor(dir_engine* e, const char* ref_key, const float* host_data,
                          const int64_t* shape, int ndim);
/* Folds eval-mode BatchNorm (eps 1e-5, dirtorch/nets/backbones/resnet.py:117) into the conv
 * weights, repacks OIHW -> [Cout][R][S][Cin] 16-bit, uploads.  DIR_ERR_MISSING names the key. */
int dir_engine_finalize(dir_engine* e, int dtype /* dir_dtype */);
int dir_engine_out_dim(const dir_engine* e, int* out_dim);

/* ---- forward: replaces ResNet_RMAC.forward (dirtorch/nets/rmac_resnet.py:39-69) ------------ */
int dir_workspace_bytes(const dir_engine* e, int B, int H, int W, size_t* bytes);
/* desc_out: B x D fp32, unit L2 norm.  (The reference's squeeze_ to [D] at B == 1 is a host-side
 * view, rmac_resnet.py:64.)  img: B x 3 x H x W fp32 or B x H x W x 3 uint8, per img_format. */
int dir_forward(dir_engine* e, const void* img, int B, int H, int W, int img_format,
                float* desc_out, void* workspace, size_t workspace_bytes, void* stream);
/* Same, but also returns the trunk feature map (NHWC, B x h x w x C, 16-bit or fp32 per the dtype) for block-level
 * parity tests against ResNet.forward (dirtorch/nets/backbones/resnet.py:157-174). */
int dir_forward_features(dir_engine* e, const void* img, int B, int H, int W, int img_format,
                         void* feat_out, int* h, int* w, int* c,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Strict-path convolution (DIR_F32): y = act(conv(x, w) + bias (+ res)), everything fp32 NHWC / [Cout][R][S][Cin],
 * Cin % 4 == 0, Cout % 4 == 0; products on v_mfma_f32_32x32x2_f32 (an fmaf chain).  Replaces Conv2d + eval BatchNorm
 * (+ residual add) (+ ReLU) of dirtorch/nets/backbones/resnet.py:56-63,70-85 without any rounding of operands. */
int dir_conv_bn_act_f32(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int H,
                        int W, int Cin, int Cout, int R, int S, int stride, int pad, int OH, int OW, int relu,
                        void* stream);
/* Strict-path pointwise kernels (DIR_F32, csrc/conv_f32.hip): dir_prep_input, dir_maxpool_3x3s2, dir_global_pool and
 * dir_upsample_add with fp32 NHWC activations - the same contracts, argument order and checks without the dtype; channel
 * counts are multiples of 4 (maxpool, upsample_add) or 64 (global_pool).  Op-level entry points of what dir_forward runs
 * after dir_engine_finalize(e, DIR_F32). */
int dir_prep_input_f32(const void* img, int img_format, const float* mean3, const float* std3, float* out, int B, int H,
                       int W, void* stream);
int dir_maxpool_3x3s2_f32(const float* x, float* y, int B, int H, int W, int C, void* stream);
int dir_global_pool_f32(const float* x, float* out, int B, int H, int W, int C, int pooling, float p, float eps,
                        float center_bias, void* stream);
int dir_upsample_add_f32(const float* x, const float* low, float* y, int B, int H, int W, int h, int w, int C,
                         void* stream);
/* The paired-fp16 head of DIR_FP16P (csrc/conv_pair.hip).  Every operand is a PAIR of fp16 planes of the ordinary
 * layout, value = hi + lo with hi = fp16(v), lo = fp16(v - hi) (~22 significant bits); every product runs as three fp16
 * MFMAs into one fp32 accumulator (w_hi.x_hi + w_hi.x_lo + w_lo.x_hi).  Replaces, at ~fp32 accuracy,
 *   dir_conv_bn_act_pair  Conv2d + eval BatchNorm (+ residual add) (+ ReLU), dirtorch/nets/backbones/resnet.py:56-63,
 *                         70-85: x [B,H,W,Cin], w [Cout][R][S][Cin], res / y [B,OH,OW,Cout]; Cin % 32 == 0,
 *                         Cout % 64 == 0, R, S <= 4; x_lo / res_lo / y_lo may be NULL (single-plane operand / output)
 *   dir_conv_pair_dual    conv3 + bn3 + the block's STRIDE-1 downsample branch + add + ReLU of layer1's first bottleneck
 *                         as one GEMM over two pixel-aligned pair tensors of equal width (resnet.py:78-85 with :134-141):
 *                         y = act([w3 | wds] . [t2 ; x] + bias3 + bias_ds); t2, x [B,H,W,Cin], wcat [Cout][2 Cin],
 *                         Cout % 128 == 0; the 4P-wide downsample tensor is neither written nor read
 *   dir_prep_input_pair   ToTensor + Normalize (dirtorch/utils/transforms.py:617-623) -> space-to-depth pair
 *                         [B, ceil(H/2), ceil(W/2), 16] x 2
 *   dir_stem_pool_pair    conv 7x7 s2 + BN + ReLU + MaxPool 3x3 s2 (resnet.py:115-119) from that pair and the 4x4x16
 *                         packed filter pair to the pooled pair [B,PH,PW,64] x 2; the conv tile stays fp32 in LDS. */
int dir_conv_bn_act_pair(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias,
                         const void* res_hi, const void* res_lo, void* y_hi, void* y_lo, int B, int H, int W, int Cin,
                         int Cout, int R, int S, int stride, int pad, int OH, int OW, int relu, void* stream);
int dir_conv_pair_dual(const void* t2_hi, const void* t2_lo, const void* x_hi, const void* x_lo, const void* wcat_hi,
                       const void* wcat_lo, const float* bias, void* y_hi, void* y_lo, int B, int H, int W, int Cin,
                       int Cout, int relu, void* stream);
int dir_prep_input_pair(const void* img, int img_format, const float* mean3, const float* std3, void* out_hi,
                        void* out_lo, int B, int H, int W, void* stream);
int dir_stem_pool_pair(const void* s2d_hi, const void* s2d_lo, const void* w_hi, const void* w_lo, const float* bias,
                       void* y_hi, void* y_lo, int B, int H2, int W2, int OH, int OW, void* stream);
/* DIR_FP16P on the RAW uint8 feed (stem_u8.hip; what dir_forward runs for DIR_IMG_U8_NHWC input): ToTensor + Normalize
 * (dirtorch/utils/transforms.py:617-623) + conv1 7x7 s2 + bn1 + ReLU + MaxPool 3x3 s2 (dirtorch/nets/backbones/resnet.py:115-119,
 * 158-161) from the uint8 NHWC image to the pooled fp16 pair [B,PH,PW,64] x 2.  The integers 0..255 are exact in one fp16 plane, so
 * the image needs no lo plane: the normalisation is folded into the filter PAIR (w . bn_scale . 256 / (255 std_c)), the bias and a
 * per-border-class bias table (zero padding happens AFTER Normalize in the reference), two MFMAs per term.  w_oihw: conv1.weight
 * [64,3,7,7] fp32 (host); bn_scale / bn_bias: bn1 in eval mode folded to y = conv * scale + bias (host, 64 each); s2d_ws: device
 * scratch of B * ceil(H/2) * ceil(W/2) * 32 bytes; seg_tiles: 0 = the kernel's own segment length, 1 = independent tiles.
 * Synchronises `stream` (parity entry point: the engine folds once at dir_engine_finalize). */
int dir_stem_pool_u8(const void* img_u8, const float* w_oihw, const float* bn_scale, const float* bn_bias, const float* mean3,
                     const float* std3, void* s2d_ws, void* y_hi, void* y_lo, int B, int H, int W, int seg_tiles, void* stream);
/* fp16 range check.  The reference computes in fp32 and cannot overflow (dirtorch/nets/backbones/resnet.py:67-87);
 * DIR_FP16 storage saturates at 65504.  Every kernel that packs fp32 sums into fp16 for a store ORs into an
 * engine-owned device word when it stores an inf / NaN - the first overflow of a forward is always such a store,
 * so a later ReLU (hardware max drops NaN operands) or a fused consumer cannot hide it.  This call synchronises
 * `stream`, returns the word in *overflowed (0 = clean) and clears it; the word is sticky across forwards until then.
 * Bit 0: an fp16 store overflowed.  Bit 1 (round 6): a kernel whose wave roles meet on LDS counters (conv_c3c1lc.hip, conv_small.hip)
 * gave up a bounded wait - its results are invalid; it cannot happen on a healthy device and is reported instead of hanging it.
 * Always 0 for DIR_BF16 (fp32's exponent range).  The host mirror raises FloatingPointError naming the
 * DIRTORCH_AMD_DTYPE switch (dirtorch_amd/test_dir.py _check_finite). */
int dir_engine_overflow(dir_engine* e, void* stream, int* overflowed);
/* Diagnostic hook: the same word for the PER-OP entry points.  device_word: a zeroed device int the caller owns, or NULL to
 * clear the hook (the state at load).  While it is set, every 16-bit per-op launch (the conv, split-K, seam, two-source, paired,
 * stem and upsample-add entry points above and below) hands it to its kernel as an engine hands its own word: bit 0 = an fp16 store
 * overflowed, bit 1 = a bounded LDS-counter wait ran out.  The caller reads and zeroes the word itself (after synchronising the
 * streams it launched on) and must clear the hook before it frees the word.  Engines keep their own word and ignore this one.  The
 * pointer is PROCESS-WIDE, not thread-scoped - a tool for tests, not for concurrent hosts - and never takes part in picking a
 * kernel: with it unset every launch is what it was without the hook. */
int dir_op_overflow_word(int* device_word);

/* Tile-variant selection for the implicit-GEMM convolutions: run every admissible variant on each
 * layer shape of a B x H x W forward and keep the fastest (synchronises).  Optional. */
int dir_engine_autotune(dir_engine* e, int B, int H, int W, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Tuned choices as text, one "layer M variant-name" line each, so a later process (e.g. a
 * profiler run) can reuse them without re-timing.  export: *needed = bytes incl. NUL. */
int dir_engine_tuning_export(const dir_engine* e, char* buf, size_t cap, size_t* needed);
int dir_engine_tuning_import(dir_engine* e, const char* text);

/* ---- per-launch profile (HIP events on the launch stream) ---------------------------------- */
typedef struct dir_prof_record {
    char     name[48];        /* layer name, e.g. "layer3.4.conv2"                          */
    char     kernel[48];      /* kernel family + variant, e.g. "conv_igemm<128x128>"        */
    double   flops;           /* algorithmic FLOPs of this launch (2*MACs)                  */
    double   bytes;           /* algorithmic bytes (compulsory in + out + weights)          */
    float    ms;              /* event-measured duration                                    */
} dir_prof_record;
/* enabled: 0 off, 1 on, n > 1 on with n event pairs pre-created (keeps event creation out of
 * a timed region). */
int dir_engine_set_profiling(dir_engine* e, int enabled);
/* Suspend / resume recording without dropping what was recorded (sample every n-th step of a
 * timed loop so that the event records themselves stay out of most steps). */
int dir_engine_profile_pause(dir_engine* e, int paused);
/* Synchronises; copies up to `cap` records of the launches made since the last call. */
int dir_engine_get_profile(dir_engine* e, dir_prof_record* out, int cap, int* n);

/* ---- per-op entry points (op-level parity tests) ----------------------- */
/* K1/K2/K4-K7: conv + folded BN bias (+ residual) (+ ReLU); x NHWC [B,H,W,Cin] 16-bit,
 * w [Cout][R][S][Cin] 16-bit, bias fp32[Cout], res/y NHWC [B,OH,OW,Cout].
 * variant < 0: heuristic choice; otherwise index into dir_conv_variant_count(). Cin % 64 == 0,
 * or Cin == 16 with R == S == 4 (the space-to-depth stem). */
int dir_conv_variant_count(void);
int dir_conv_variant_name(int variant, char* buf, int cap);
int dir_conv_bn_act(const void* x, const void* w, const float* bias, const void* res, void* y,
                    int B, int H, int W, int Cin, int Cout, int R, int S, int stride,
                    int pad, int OH, int OW, int relu, int dtype, int variant, void* stream);
/* Which tile variant (and split-K factor) the engine picks for a layer shape that has not been autotuned.
 * Pure host logic - no GPU needed - exposed so that the choices distilled from the tuner stay pinned by
 * CPU tests (tests/test_capi_host.py). */
int dir_conv_heuristic(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int OH,
                       int OW, int has_residual, char* name, int cap, int* ksplit);
/* Would dir_conv_bn_act accept `variant` for this shape?  *admissible = 1 / 0.  Pure host logic (the predicate conv_launch
 * itself applies), exposed so that the GPU parity matrix is generated from admissible (variant, shape) pairs only and the
 * tests' own mirror of the rule is pinned on the CPU (tests/test_capi_host.py). */
int dir_conv_variant_admissible(int variant, int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                int OH, int OW, int has_residual, int* admissible);
/* How many K slices the engine (and its tuner) launches `variant` in on this shape: *ksplit = 1 (no split) or 2..8.  Pure host
 * logic (conv_splitk_factor, what dir_conv_bn_act_splitk applies for ksplit < 0), exposed so that a caller can reserve exactly
 * the scratch that factor needs (*ksplit * B*OH*OW * Cout floats when > 1, none otherwise) and the tests can group the tuner's
 * candidate launches by their split.  DIR_ERR_INVALID when the variant is not admissible for the shape. */
int dir_conv_variant_splitk(int variant, int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                            int OH, int OW, int has_residual, int* ksplit);
/* Same convolution with the K loop cut into `ksplit` slices that run as separate workgroups and meet in
 * an fp32 scratch buffer (ksplit * B*OH*OW * Cout floats; slices are added in a fixed order, then bias /
 * residual / ReLU) - what the engine does for layers with too few output tiles to fill 256 CUs (batch 1
 * at the deep stages).  ksplit < 0: the engine's own choice for that variant (reported in *ksplit_used);
 * variants without a split-K form accept only ksplit <= 1. */
int dir_conv_bn_act_splitk(const void* x, const void* w, const float* bias, const void* res, void* y,
                           int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                           int OH, int OW, int relu, int dtype, int variant, int ksplit, void* scratch,
                           size_t scratch_bytes, int* ksplit_used, void* stream);
/* The seam between two bottlenecks as ONE kernel (csrc/conv_c3c1.hip), planes P = 64 or 128:
 *   y  = act3(conv1x1(t2; w3 [4P][P]) + bias3 + res)      the conv3 + bn3 + add + ReLU that closes a block
 *   t1 = act1(conv1x1(y;  w1 [P2][4P]) + bias1)           the conv1 + bn1 + ReLU that opens the next one
 * (dirtorch/nets/backbones/resnet.py:78-85 then :70-72); P2 = P inside a stage, P2 = 128 after P = 64 for
 * the layer1 -> layer2 boundary.  t2 [B,H,W,P], res / y [B,H,W,4P], t1 [B,H,W,P2],
 * NHWC 16-bit; conv1 consumes the ROUNDED y, so the pair equals two dir_conv_bn_act calls up to fp32
 * summation order.  The engine uses it for the layer1 / layer2 seams when the map has >= 131072 pixels. */
int dir_conv_c3c1(const void* t2, const void* w3, const float* bias3, const void* res, void* y, const void* w1,
                  const float* bias1, void* t1, int B, int H, int W, int P, int P2, int relu3, int relu1, int dtype,
                  void* stream);
/* conv3 + bn3 + the block's downsample branch + add + ReLU of a stage's FIRST bottleneck as one GEMM over
 * two K sources (csrc/conv_persist.hip, DUAL form: the persistent deep-X ring with a second pixel source; dirtorch/nets/backbones/resnet.py:78-85 with :134-141):
 *   y[b,oh,ow,:] = act([w3 | wds] . [t2[b,oh,ow,:] ; x[b,oh*stride2,ow*stride2,:]] + bias),  bias = bias3 + bias_ds
 * t2 [B,OH,OW,Cin], x [B,H2,W2,Cin2] NHWC 16-bit, wcat [Cout][Cin + Cin2], Cout % 256 == 0, Cin, Cin2 % 64 == 0.
 * The Cout-wide residual tensor is neither written nor read. */
int dir_conv_dual(const void* t2, const void* x, const void* wcat, const float* bias, void* y, int B, int OH, int OW,
                  int Cin, int Cout, int Cin2, int H2, int W2, int stride2, int relu, int dtype, void* stream);
/* The same seam for the FIRST block of layer1 (planes 64), whose residual is the downsample branch
 * conv1x1(x; wds [256][64]) + bn of the 64-channel block input (resnet.py:134-141, 157-160): the
 * downsample is folded into the GEMM as 64 more K,
 *   y = act3([w3 | wds] . [t2 ; x] + (bias3 + bias_ds)),    wcat = [256][64 + 64], bias = the sum,
 * so the 256-wide residual tensor is never written or read.  t2, x [B,H,W,64]; y [B,H,W,256]; t1 [B,H,W,64]. */
int dir_conv_c3c1_ds(const void* t2, const void* x, const void* wcat, const float* bias, void* y, const void* w1,
                     const float* bias1, void* t1, int B, int H, int W, int relu3, int relu1, int dtype,
                     void* stream);
/* Both seams with PAIRED WEIGHTS (DIR_FP16P, fp16 only; csrc/conv_c3c1.hip WP3 / WP1): every weight matrix comes as two
 * fp16 planes, value = hi + lo with lo = fp16(w - hi) (~22 bits), and every product term costs two MFMAs instead of one -
 * no extra bytes on these HBM-bound kernels (measured: +6-9 % time, +35 % for the DS form with its third K block).  Activations are single fp16 planes, except the block input x of the DS form (the
 * stem's pooled output), which is a pair as well: [w3 | wds] . [t2 ; x_hi + x_lo] with the lo x lo term dropped.
 * P = 64 (layer1: dirtorch/nets/backbones/resnet.py:67-87, 134-141); P2 = 64 needs w1_lo, P2 = 128 (the layer1 ->
 * layer2 boundary, whose conv1 belongs to layer2) takes w1_lo = NULL for single-plane weights there. */
int dir_conv_c3c1_wpair(const void* t2, const void* w3, const void* w3_lo, const float* bias3, const void* res, void* y,
                        const void* w1, const void* w1_lo, const float* bias1, void* t1, int B, int H, int W, int P2,
                        int relu3, int relu1, void* stream);
int dir_conv_c3c1_ds_wpair(const void* t2, const void* x, const void* x_lo, const void* wcat, const void* wcat_lo,
                           const float* bias, void* y, const void* w1, const void* w1_lo, const float* bias1, void* t1,
                           int B, int H, int W, int relu3, int relu1, void* stream);
/* dir_conv_c3c1 / dir_conv_c3c1_wpair as the engine launches them at a stage exit and in place:
 *   keep_stride = s > 1: y receives only the pixels (b, h, w) with h % s == 0 && w % s == 0, at their places in the
 *       full-resolution [B,H,W,4P] layout - what a following 1x1 stride-s downsample reads; every other element of y is left
 *       untouched.  t1 is complete.  keep_stride 0 or 1: every pixel, as the entry points above.
 *   y may be res itself (an identity block written over its input): the result is the same, bit for bit. */
int dir_conv_c3c1_keep(const void* t2, const void* w3, const float* bias3, const void* res, void* y, const void* w1,
                       const float* bias1, void* t1, int B, int H, int W, int P, int P2, int relu3, int relu1,
                       int keep_stride, int dtype, void* stream);
int dir_conv_c3c1_wpair_keep(const void* t2, const void* w3, const void* w3_lo, const float* bias3, const void* res, void* y,
                             const void* w1, const void* w1_lo, const float* bias1, void* t1, int B, int H, int W, int P2,
                             int relu3, int relu1, int keep_stride, void* stream);
/* Slow, obviously-correct direct convolution with the same contract (device-side checker). */
int dir_conv_bn_act_naive(const void* x, const void* w, const float* bias, const void* res,
                          void* y, int B, int H, int W, int Cin, int Cout, int R, int S,
                          int stride, int pad, int OH, int OW, int relu, int dtype, void* stream);
/* Image -> space-to-depth stem input [B, ceil(H/2), ceil(W/2), 16] 16-bit (12 used channels). */
int dir_prep_input(const void* img, int img_format, const float* mean3, const float* std3,
                   void* out, int B, int H, int W, int dtype, void* stream);
/* K1+K2+K3 fused: the whole stem (conv 7x7 s2 + BN + ReLU + MaxPool 3x3 s2,
 * dirtorch/nets/backbones/resnet.py:115-119) from the space-to-depth image of dir_prep_input
 * [B,H2,W2,16] and the 4x4x16 packed stem filter to the pooled map [B,PH,PW,64]; OH x OW is the conv
 * output size the pool runs over.  What dir_forward uses. */
int dir_stem_pool(const void* s2d, const void* w, const float* bias, void* y, int B, int H2, int W2,
                  int OH, int OW, int dtype, void* stream);
/* The `Scale` test-time transform (dirtorch/utils/transforms.py:133-185 -> PIL
 * Image.resize(size, BILINEAR)) for uint8 NHWC RGB images already on the device: Pillow's
 * antialiased triangle filter with 22-bit fixed-point weights, horizontal then vertical pass, each
 * rounded to uint8 - bit-identical to Pillow (src/libImaging/Resample.c).  All B images share H x W.
 * workspace: dir_resize_workspace_bytes() bytes, 4-byte aligned; three async launches on `stream`. */
int dir_resize_workspace_bytes(int B, int H, int W, int OH, int OW, size_t* bytes);
int dir_resize_bilinear_u8(const void* src, void* dst, int B, int H, int W, int OH, int OW,
                           void* workspace, size_t workspace_bytes, void* stream);
/* K3: MaxPool2d(3, stride 2, pad 1) on NHWC (dirtorch/nets/backbones/resnet.py:119). */
int dir_maxpool_3x3s2(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
/* K8: global pooling over H*W of NHWC x -> fp32 [B,C] (dirtorch/nets/layers/pooling.py:38-40);
 * pooling = dir_pooling, p = GeM exponent (runtime scalar), eps = 1e-6 clamp;
 * center_bias > 0 applies the bilinear mask of rmac_resnet.py:52-56 first. */
int dir_global_pool(const void* x, float* out, int B, int H, int W, int C, int pooling, float p,
                    float eps, float center_bias, int dtype, void* stream);
/* FPN lateral merge: y = x + nearest_upsample(low) with x,y NHWC [B,H,W,C], low [B,h,w,C], 16-bit;
 * source index min(floor(dst * in/out), in-1) as F.interpolate(mode='nearest', size=...) computes it
 * (dirtorch/nets/rmac_resnet_fpn.py:55-60).  C % 8 == 0. */
int dir_upsample_add(const void* x, const void* low, void* y, int B, int H, int W, int h, int w, int C,
                     int dtype, void* stream);
/* L2-normalise each row in place: x / max(||x||, eps) (F.normalize, rmac_resnet.py:7-9). */
int dir_l2norm_rows(float* x, int rows, int cols, float eps, void* stream);
/* K9/K11/K12: out[j][i] = alpha_i * (sum_k P[i][k] * (Q[j][k] - qsub[k])) + bias[i]
 *   P: [NP,K] fp32 (ldp), Q: [NQ,K] fp32 (ldq), out: [NQ,NP] fp32 (ldo); qsub/bias/alpha may be
 *   NULL.  Exact fp32 (v_mfma_f32_32x32x2_f32).  Any K >= 1 and any pitches ldp, ldq >= K (16-byte
 *   loads when K, ldp, ldq are multiples of 4 and the bases 16-byte aligned, an element-wise gather
 *   otherwise - e.g. --whitenv 50).  Used as
 *     FC          : P = fc.weight, Q = pooled features, bias = fc.bias   (rmac_resnet.py:66)
 *     PCA whiten  : P = components_[:v], Q = X, qsub = mean_, alpha = 1/(m*var^p) (common.py:221-232)
 *     similarity  : P = database descriptors, Q = queries -> scores[Q][N]       (common.py:30-38)
 *   Shapes with fewer than 128 output tiles (128 x 32..128) and K >= 512 - the FC of a batch, PCA whitening of a few
 *   hundred descriptors - run as up to 16 K slices whose fp32 partial sums (stream-ordered scratch, <= 64 MB) are
 *   added in slice order by a second kernel: same sums, another association, run-to-run identical.
 *   dir_gemm_splitk_factor (host-only) tells how many slices a shape gets. */
int dir_gemm_splitk_factor(int NP, int NQ, int K);
int dir_gemm_nt_f32(const float* P, int ldp, const float* Q, int ldq, float* out, int ldo,
                    int NP, int NQ, int K, const float* qsub, const float* bias,
                    const float* alpha, void* stream);
/* The three named uses of the GEMM above, as the reference's callers see them (all fp32, row-major,
 * contiguous; every output buffer is the caller's):
 *   dir_fc_l2          x[B,K] -> normalize(x W^T + b): the tail of ResNet_RMAC.forward
 *                      (dirtorch/nets/rmac_resnet.py:66-68); W is [D,K] (nn.Linear layout)
 *   dir_pca_whiten_l2  common.whiten_features (dirtorch/utils/common.py:221-239):
 *                      out[n][i] = scale[i] * sum_k components[i][k] * (X[n][k] - mean[k]), i < v, then
 *                      row L2 if l2norm != 0; scale[i] = 1 / (whitenm * explained_variance[i]^whitenp)
 *                      is computed by the caller (v floats, device), NULL = no rescaling
 *   dir_similarity     common.matmul(queries, database) (dirtorch/utils/common.py:30-38):
 *                      scores[q][n] = <queries[q], database[n]>, scores is [Q,N] with row stride N.
 *                      N >= 32768 with D % 32 == 0 (the 10^6-distractor protocol): every fp32 operand is split
 *                      into three bf16 planes and the six leading plane products run on the bf16 matrix cores
 *                      with fp32 accumulation (csrc/sim_split.hip) - products to 2^-23, measured error against
 *                      fp64 below that of the k-ordered fp32 chain, 1.8x its speed; takes ceil(Q/96) * D * 576
 *                      bytes of stream-ordered scratch (hipMallocAsync).  Smaller databases, other widths and
 *                      DIRTORCH_AMD_SIM_EXACT=1 in the environment: the exact k-ordered chain of dir_gemm_nt_f32.
 *   dir_similarity_unit  the same product for operands the caller KNOWS to lie in (-64, 64) - L2-normalised
 *                      descriptors, what common.matmul is called on in dirtorch/test_dir.py:150 - on the large-database
 *                      path: every operand as two fp16 planes of 2^10 x (~22 bits), three plane products instead of
 *                      six, scores rescaled by 2^-20: as accurate on unit vectors, 20+ % faster (the six-product form
 *                      is matrix-pipe-bound).  A value of magnitude >= 64 overflows its plane to inf and the scores
 *                      of its row come out NON-FINITE - never silently wrong.  Other sizes: identical to dir_similarity. */
int dir_fc_l2(const float* x, int B, int K, const float* W, const float* b, int D, float* out,
              void* stream);
int dir_pca_whiten_l2(const float* X, int N, int D, const float* mean, const float* components,
                      int v, const float* scale, int l2norm, float* out, void* stream);
/* dir_pca_whiten_l2 for operands the caller KNOWS to be bounded: |X - mean| < 64 and |components| < 64 - L2-normalised descriptors
 * and the orthonormal rows of a PCA, what common.whiten_features is called on in dirtorch/test_dir.py:136-138.  N >= 32768 with
 * D % 32 == 0 and D <= 6144 (the 10^6-distractor database of BASELINE configs[3]: 8.4 TFLOP): X minus the mean (subtracted in fp32,
 * before anything is rounded) and the components as two fp16 planes of 2^10 x each (~22 bits), three plane products on the fp16
 * matrix cores, fp32 accumulation, result x 2^-20 scale[j] (csrc/sim_split.hip whiten_split_kernel): within ~1e-6 (relative to the
 * row's largest entry) of the fp64 product, ~4x the fp32 MFMA chain.  A value outside the range overflows its plane and its row
 * comes out NON-FINITE, never silently wrong.  Other sizes, and DIRTORCH_AMD_SIM_EXACT=1: identical to dir_pca_whiten_l2.
 * Takes ceil(v/96) * D * 384 bytes of stream-ordered scratch (hipMallocAsync). */
int dir_pca_whiten_l2_unit(const float* X, int N, int D, const float* mean, const float* components,
                      int v, const float* scale, int l2norm, float* out, void* stream);
int dir_similarity(const float* queries, int Q, const float* database, int N, int D, float* scores,
                   void* stream);
int dir_similarity_unit(const float* queries, int Q, const float* database, int N, int D, float* scores,
                        void* stream);
/* Fitting a PCA whitening: the N-dependent half, on the device.  The reference has no call to cite - it ships the
 * Landmarks18_pca image list and no code for the fit; what this feeds is the PCA that dirtorch/utils/common.py:221-232
 * reads (mean_, components_, explained_variance_), which dirtorch_amd/whitening.py derives on the host from gram and sums.
 *   a[n][i]     = X[n][i] - shift[i]            (fp32, subtracted at load, before any product: the shifted-data form -
 *                                                with shift near the column mean the sums sums^T / n correction is tiny)
 *   gram[i][j] += sum_n a[n][i] * a[n][j]       fp64 [D][D] contiguous, both triangles written, bit-symmetric
 *   sums[i]    += sum_n a[n][i]                 fp64 [D]
 *   X: [N,D] fp32 with row pitch ldx >= D; shift: [D] fp32; all device pointers.  Any D >= 1, N >= 0 (N = 0 leaves the
 *   accumulators untouched, and X may then be NULL); 16-byte loads when D and ldx are multiples of 4 and X, shift 16-byte aligned, an
 *   element-wise gather otherwise.  The caller zeroes gram and sums before the first call; calls add, so a set of any
 *   size is fed in chunks.  Products on v_mfma_f32_32x32x2_f32 (exact products, fp32 fma chain); a chain runs over at
 *   most dir_cov_chain_rows() rows (host-only query) and is then folded into an fp64 accumulator, so every entry is within
 *   (R + 3) 2^-24 sum_n |a_ni| |a_nj| of the exact sum whatever N is.  Upper-triangle tiles of 128 x 128 x up to 64 row
 *   slices; the slices' fp64 partials (stream-ordered scratch, hipMallocAsync: slices x tiles x 128 KiB, <= 1024 tiles x
 *   slices) are added in slice order by a second kernel - no atomics, run-to-run identical. */
int dir_cov_chain_rows(void);
int dir_cov_accumulate(const float* X, int ldx, int N, int D, const float* shift, double* gram, double* sums,
                       void* stream);
/* K10: multi-scale pooling of S descriptor sets [S][N][D] -> [N][D] (common.py:41-55):
 * mode 0 = mean, 1 = signed-power ("gem") mean with exponent gemp; no final L2 (caller does it). */
int dir_multiscale_pool(const float* x, float* out, int S, int N, int D, int mode, float gemp,
                        void* stream);

/* N1: ranking without sorting, for ImageListRelevants.eval_query_AP
 * (dirtorch/datasets/generic.py:196-224).  For every query q and every probe p (a database index,
 * -1 = unused slot) counts[q][p] = number of database items that rank before it under
 * np.argsort(scores[q])[::-1]: score greater, or equal with a larger index.  probe_scores[q][p]
 * receives scores[q][probe].  scores: [Q][N] fp32 with row stride lds; probe_idx / counts /
 * probe_scores are [Q][P] (any P: 4096 probes per query per pass).  Sorted probes + one binary search per score + a
 * histogram (ranking.hip): each score is read once per pass, NaN scores rank before nothing, -0 == +0; probe_scores
 * doubles as the kernels' scratch until the call's last kernel (no workspace argument). */
int dir_rank_counts(const float* scores, int lds, int Q, int N, const int* probe_idx, int P,
                    int* counts, float* probe_scores, void* stream);
/* N1, second half: the APs themselves on the device - ImageListRelevants.eval_query_AP
 * (dirtorch/datasets/generic.py:196-224) + compute_average_precision (dirtorch/utils/evaluation.py:46-82)
 * from the outputs of dir_rank_counts.  For every (query q, mode m < modes) the caller lists, as
 * positions INTO row q of probe_idx, the positives pos_list[pos_off[q*modes+m] .. pos_off[q*modes+m+1])
 * and the junk junk_list[junk_off[..] ..) of that mode (duplicates removed; an image that is both is
 * junk - generic.py:192).  ap_out[q*modes+m] = the trapezoidal AP, summed in fp64 in the reference's
 * order, or -1 when the mode has no positive.  terms: fp64 scratch, one slot per pos_list entry. */
int dir_revisitop_ap(const int* probe_idx, int Q, int P, const int* counts, const float* probe_scores,
                     const int* pos_off, const int* pos_list, const int* junk_off, const int* junk_list,
                     int modes, double* terms, double* ap_out, void* stream);
/* N1 for class-labelled datasets (ImageListLabels / ImageListLabelsQ): replaces, per query, get_query_groundtruth +
 * sklearn's average_precision_score (dirtorch/datasets/dataset.py:70-101, dirtorch/utils/evaluation.py:41-43) and the
 * argsort of eval_query_top (dirtorch/test_dir.py:153-178), without a sort of the score row.
 *   scores [Q][lds] fp32, lds >= N; labels [N] = class id of every database image; class_off [C+1] / class_members [N] =
 *   CSR of the database indices of every class (shared by all queries); qclass [Q] = the query's class, -1 when no
 *   database image carries it; qself [Q] = the query's own database index when the queries ARE the database, else -1.
 *   ap[q]        = (1/n_pos) sum over positives p of pos_ge(s_p) / all_ge(s_p), counted over the kept items (all but
 *                  qself): sklearn's value - tied scores share one threshold, -0 == +0 - summed in fp64 in a fixed order;
 *                  -1 when no kept item is positive; NaN when a kept score of the row is NaN or +-inf (sklearn raises)
 *   best_rank[q] = position of the best-placed image of the class under np.argsort(-scores, kind='stable') (score
 *                  descending, index ascending on ties, NaN last; qself is NOT left out): correct[:k].any() is
 *                  best_rank < k; N when the class has no image
 * The tables are checked on the device before anything indexes with them and the call waits for the verdict (one
 * stream synchronisation per call): lds < N, a class_off that is no CSR from 0 to N, a class_members entry outside [0, N),
 * filed under another class than labels gives it or listed twice (class_members is a permutation of the database
 * indices), qclass outside [-1, C) or qself outside [-1, N) fail with DIR_ERR_INVALID and launch nothing else.  One workgroup per query; each score is read once per 4096 class members. */
int dir_label_rank(const float* scores, int lds, int Q, int N, const int* labels, const int* class_off,
                   const int* class_members, int C, const int* qclass, const int* qself, double* ap, int* best_rank,
                   void* stream);
/* Ranked neighbour lists: the k best database items of every query, in order, without a sort of the score row - what
 * np.argsort(scores[q])[::-1][:k] (dirtorch/datasets/generic.py:207-208) and the np.argpartition of expand_descriptors
 * (dirtorch/test_dir.py:24-44) give on the host after downloading the Q x N matrix.
 *   scores [Q][lds] fp32, lds >= N.  ids NULL: an item's id is its column; else ids [Q][lds] int32 gives the id of every
 *   column (distinct within a row - the caller's duty), -1 = an empty column that is skipped: the form that merges
 *   per-shard or per-database-block lists, or a running list with a new block's candidates.  exclude NULL or [Q]: the item
 *   with id exclude[q] is left out of row q (-1: nothing) - a query is not its own neighbour.
 *   Order (dir_rank_counts' order): item j before item p when s_j > s_p, or s_j == s_p and id_j > id_p - on a NaN-free row
 *   np.argsort(row, kind='stable')[::-1]; -0 == +0, +-inf are ordinary values; a NaN ranks after every number, -inf
 *   included, and among NaNs the larger id comes first.
 *   out_idx [Q][k] = the ids, best first; out_score [Q][k] = the stored bits of their scores (-0, a NaN's payload).  A row
 *   with fewer than k kept items ends in (idx -1, score NaN) slots.
 * 1 <= k <= min(N, dir_topk_max_k()) (host-only query; 2048).  workspace: at least dir_topk_workspace_bytes(Q, N, k)
 * (host-only; monotone in each argument; 0 for rows of one slice, where workspace may be NULL).  k outside that range,
 * lds < N, a null scores / out_idx / out_score or a short workspace fail with DIR_ERR_INVALID before anything is launched;
 * Q == 0 is DIR_OK and launches nothing.
 * topk.hip: one workgroup per (slice of 16384 columns, query) reads its scores once (N * 4 B per query, like
 * rank_hist_kernel), radix-selects the slice's k best from keys held in registers and writes them to the workspace as a shorter row with an id
 * table; the same kernel reduces that row until one slice is left, whose k survivors are sorted in LDS.  The 64-bit keys
 * (score key : id) are distinct, so the output is bitwise reproducible: it does not depend on the slice size, the grid,
 * workgroup scheduling or the arrival order of the (LDS, integer) atomics. */
int dir_topk_max_k(void);
int dir_topk_workspace_bytes(int Q, int N, int k, size_t* bytes);
int dir_topk(const float* scores, int lds, int Q, int N, int k, const int* ids, const int* exclude, int* out_idx,
             float* out_score, void* workspace, size_t workspace_bytes, void* stream);
/* The int8 descriptor index (index_i8.hip): a compact database, the scan that scores it and the re-score of a shortlist.
 * The quantisation of a row x of D fp32 values, every step a single IEEE fp32 operation rounded to nearest:
 *     amax  = max_k |x_k|                                  (exact)
 *     scale = amax / 127          inv = 127 / amax         (two divisions)
 *     code_k = clamp(rint(x_k * inv), -127, 127) as int8   (one multiply, then round-half-even; -128 never occurs)
 *   a row whose inv is not finite (amax zero, or so small that 127 / amax overflows) has all-zero codes and scale 0;
 *   a row that holds a NaN or an infinity has all-zero codes and scale NaN (all its scores are NaN: dir_topk ranks them last).
 *   Codes are stored as [rows][ldc] int8, ldc >= D rounded up to a multiple of 64; bytes D .. that multiple of every row are
 *   written as zero, so a scan has no K tail.
 * dir_index_i8_max_dim (host-only; 131072): the widest row.  |code| <= 127, so a dot product of that width is at most
 *   2 114 060 288 < 2^31: the int32 accumulator of the scan cannot wrap.
 * dir_quantize_rows_i8: X [N][ldx] fp32 (ldx >= D, any pitch) -> codes [N][ldc] (4-byte aligned, ldc % 4 == 0) and scales [N].
 *   One wave per row; a row of up to 2048 values is read once (32 floats per lane), a wider one twice.
 * dir_similarity_i8: scores[q][n] = ((float)dot_i32 * qscales[q]) * bscales[n], dot_i32 = sum_k qcodes[q][k] * bcodes[n][k]
 *   in int32 (exact), the conversion rounded to nearest, the two fp32 multiplies in that order - ONE defined fp32 number,
 *   independent of tiling, K order, chunking and sharding.  qcodes [Q][ldq] (ldq >= D), bcodes [N][ldb] (16-byte aligned,
 *   ldb % 16 == 0, ldb >= D rounded up to 64: that many bytes of every row are read; what they hold past D does not
 *   matter), scores [Q][lds] fp32, lds >= N.  v_mfma_i32_32x32x32_i8 on sim_split.hip's work split: 256 database rows per
 *   workgroup brought in once by LDS-DMA, the query block (96 rows) as a prepared image of the LDS stage, K slabs of 128.
 *   The query image lives in stream-ordered scratch (no workspace argument).
 * dir_gather_scores: scores[q][r] = <queries[q], database[cand[q][r]]> in fp32 - the re-score of a shortlist.  queries
 *   [Q][ldq], database [N][ldb] fp32, cand [Q][ldcand] int32, scores [Q][ldsc]; an entry -1 gives a NaN score, an entry
 *   outside [-1, N) is undefined (the caller's duty, as ids in dir_topk).  fp32 products and fp32 sums in an unspecified
 *   order: each score is within (D + 2) * 2^-24 * sum_k |q_k b_k| of the exact sum.  One wave per (query, candidate).
 * All three: a negative count, D < 1 (or above the max dim), a pitch below its minimum, lds < N or a null pointer fail with
 * DIR_ERR_INVALID before anything is launched; Q == 0 or N == 0 (or R == 0) is DIR_OK and launches nothing. */
int dir_index_i8_max_dim(void);
int dir_quantize_rows_i8(const float* X, int ldx, int N, int D, int8_t* codes, int ldc, float* scales, void* stream);
int dir_similarity_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                      const float* bscales, int N, int D, float* scores, int lds, void* stream);
int dir_gather_scores(const float* queries, int ldq, int Q, const float* database, int ldb, int N, int D, const int* cand,
                      int ldcand, int R, float* scores, int ldsc, void* stream);
/* The fp4 descriptor index (index_fp4.hip; dirtorch_amd/index.py Fp4Index; numpy restatement: tests/fp4_ref.py): half of the
 * int8 index's bytes, scanned on the scaled matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4).  It stands beside
 * dir_quantize_rows_i8 / dir_similarity_i8 and replaces nothing in the reference, which keeps fp32 descriptors.
 * A row x of D fp32 values, 1 <= D <= dir_index_fp4_max_dim() = 7281, is cut into blocks of 32 consecutive k (the last one
 * padded with zeros) and stored as
 *     codes  [ldc] bytes: two e2m1 values per byte, even k in the low nibble of byte k / 2; ldc >= D rounded up to 64,
 *            divided by 2 - that many bytes are written, the padding as 0x0;
 *     exps   [lde] bytes: one e8m0 byte per block, lde >= 8 * ceil(D / 256) (whole K slabs of the scan) - that many bytes
 *            are written, 127 for every block past D;
 *     scale  one fp32 power of two.
 * The quantisation, in integer operations on the exponent field and exact fp32 multiplications by powers of two:
 *     amax_b = max |x_k| over block b;  f_b = its biased exponent field (0 for zero and subnormal blocks)
 *     F = max_b f_b;  E = F - 129  (= floor(log2 amax) - 2, the OCP MX rule);  m_b = max(f_b, F - 2)
 *     e_b = m_b - 129: the block exponent, floor(log2 amax_b) - 2 clamped to [E - 2, E] - a clamped block is coded on the
 *       grid of the row's top blocks, its absolute error never above theirs;  exps[b] = 127 + (e_b - E), one of 125, 126, 127
 *     y_k = |x_k| * 2^-e_b  (exact, < 8);  code_k = the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} to y_k, a midpoint going to
 *       the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating: y in (5, 8) -> 6
 *     nibble = sign bit : 3-bit e2m1 code; a value that rounds to zero is stored as +0 (nibble 0x0, like the padding)
 *     scale = 2^E
 *   a row that holds a NaN or an infinity has zero codes, block bytes 127 and scale NaN (all its scores are NaN);
 *   a row with amax < 2^-60 (zero included) has zero codes, block bytes 127 and scale +0.
 * dir_quantize_rows_fp4: X [N][ldx] fp32 (ldx >= D, any pitch) -> codes [N][ldc] (2-byte aligned, ldc % 2 == 0), exps
 *   [N][lde] row-major at their own pitch, scales [N].  One wave per row; a row of up to 2048 values is read once.
 * dir_similarity_fp4: scores[q][n] = (acc * qscales[q]) * bscales[n], two fp32 multiplies in that order, acc = the fp32
 *   accumulator of the scaled MFMAs fed the stored block bytes = sum_k a_k b_k of the values code * 2^(exps - 127).  Every
 *   product is a multiple of 1/64 of at most 36, so every partial sum in any order is a multiple of 1/64 below
 *   36 * 7281 < 2^24 / 64: acc is exact whatever the K order, the tiling or the chunking, the scales are powers of two,
 *   and the score is the exact inner product of the two dequantised rows (rounded once if it leaves fp32's range) - ONE
 *   defined fp32 number.  That fixes the widest row.
 *   qcodes [Q][ldq] (ldq >= ceil(D / 2)), qexps [Q][ldqe] (ldqe >= ceil(D / 32)): read up to D only.  bcodes [N][ldb]
 *   (16-byte aligned, ldb % 16 == 0, ldb >= D rounded up to 64, divided by 2: that many bytes of every row are read; what
 *   they hold past D does not matter), bexps [N][ldbe] (8-byte aligned, ldbe % 8 == 0, ldbe >= 8 * ceil(D / 256): that many
 *   bytes of every row are read, one 8-byte load per slab; the bytes of blocks past D rounded up to 64 do not matter, the
 *   others are e8m0 bytes other than 255).  The codes pitch need not cover a whole slab: the loader cuts the last slab by
 *   16-byte chunk.  scores [Q][lds] fp32, lds >= N.  The query image lives in stream-ordered scratch.
 * Both: a negative count, D < 1 or above the max dim, a pitch below its minimum, lds < N or a null pointer fail with
 * DIR_ERR_INVALID before anything is launched; Q == 0 or N == 0 is DIR_OK and launches nothing. */
int dir_index_fp4_max_dim(void);
int dir_quantize_rows_fp4(const float* X, int ldx, int N, int D, uint8_t* codes, int ldc, uint8_t* exps, int lde,
                          float* scales, void* stream);
int dir_similarity_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                       const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, int N, int D,
                       float* scores, int lds, void* stream);
/* The binary descriptor index (index_bin.hip; dirtorch_amd/index.py BinaryIndex; numpy restatement: tests/bin_ref.py): one
 * sign bit per value and one fp32 scale per row - at D = 2048 a row is 260 bytes, a quarter of the fp4 row - scanned on the
 * int8 matrix cores (v_mfma_i32_32x32x32_i8) against int8 query codes.  It stands beside the int8 and fp4 indexes and
 * replaces nothing in the reference, which keeps fp32 descriptors.
 * A row x of D fp32 values, 1 <= D <= dir_index_bin_max_dim() = 131072 (= dir_index_i8_max_dim(): 127 * D < 2^24, so the
 * int32 sum of a score converts to fp32 exactly), is stored as
 *     bits   [ldb] bytes, ldb >= D rounded up to 128, divided by 8 (a multiple of 16) - that many bytes are written: bit
 *            k & 7 of byte k >> 3 is 1 when the sign bit of x_k is clear, for k < D, and 0 for k >= D (numpy:
 *            packbits(~signbit(x), bitorder='little')); -0.0 codes as 0;
 *     scale  = sumsq / sumabs, one fp32 division, of sumabs = sum |x_k| and sumsq = sum (x_k * x_k) - each product rounded,
 *            then added, no fma - both as chains of single fp32 additions in THIS order: 64 chains, chain l over
 *            k = 256 j + 4 l + e for j = 0, 1, .. and e = 0 .. 3 ascending (k >= D adds +0), each from +0; then six
 *            butterfly steps d = 32, 16, 8, 4, 2, 1, every chain l replaced by chain l + chain (l ^ d).  The order does not
 *            depend on N, the pitch, the alignment or the launch.
 *   a row that holds a NaN or an infinity has all-zero bits and scale NaN (all its scores are NaN: dir_topk ranks them last);
 *   a row whose sumabs is zero, or whose sumabs or sumsq overflows to infinity, has all-zero bits and scale +0.
 * The query side is dir_quantize_rows_i8's, unchanged (qcodes, qscales).
 * dir_quantize_rows_bin: X [N][ldx] fp32 (ldx >= D, any pitch) -> bits [N][ldb] (4-byte aligned, ldb % 4 == 0) and scales
 *   [N].  One wave per row; a row of up to 2048 values is read once, a wider one twice; whole dwords of bits are stored.
 * dir_similarity_bin: scores[q][n] = ((float)t * qscales[q]) * bscales[n], t = sum_{k < D} qcodes[q][k] * s_k with s_k = +1
 *   where bit k of row n is set and -1 where it is clear: an exact int32 of at most 127 * D < 2^24, the conversion exact,
 *   the two fp32 multiplies in that order (dir_similarity_i8's form) - ONE defined fp32 number, independent of tiling, K
 *   order, chunking and sharding.  The kernel computes t = 2 * sum_k qc_k b_k - sum_{k < D} qc_k with b_k the bit.
 *   qcodes [Q][ldq] int8 (ldq >= D: read up to D only), bits [N][ldb] (16-byte aligned, ldb % 16 == 0, ldb >= D rounded up
 *   to 128, divided by 8: that many bytes of every row are read; the bits past D meet zero query codes and do not
 *   matter), scores [Q][lds] fp32, lds >= N.  256 database rows per workgroup, brought in once per query block by LDS-DMA
 *   in 128-byte pieces of a row (1024 k); the query block (96 rows) streams beside them as dir_similarity_i8's image, in
 *   sub-slabs of 128 k.  The query image and the query sums live in stream-ordered scratch.
 * Both: a negative count, D < 1 or above the max dim, a pitch below its minimum, lds < N or a null pointer fail with
 * DIR_ERR_INVALID before anything is launched; Q == 0 or N == 0 is DIR_OK and launches nothing. */
int dir_index_bin_max_dim(void);
int dir_quantize_rows_bin(const float* X, int ldx, int N, int D, uint8_t* bits, int ldb, float* scales, void* stream);
int dir_similarity_bin(const int8_t* qcodes, int ldq, const float* qscales, int Q, const uint8_t* bits, int ldb,
                       const float* bscales, int N, int D, float* scores, int lds, void* stream);
/* The inverted-file int8 index (ivf.hip; dirtorch_amd/index.py IVFInt8Index; numpy restatement: tests/ivf_ref.py).
 * An index of width D with nlist lists holds
 *     centroids [nlist][D] fp32 with their codes and scales (dir_quantize_rows_i8),
 *     the database in LIST-MAJOR storage: codes [N][ldc] int8, scales [N] fp32, ids [N] int32 - the id of a row is its number
 *       in the order the rows were added (the number the flat int8 index reports),
 *     list_off [nlist + 1] int32, a CSR from 0 to N: list l is rows list_off[l] .. list_off[l + 1), in ascending id.
 * Assignment: a row belongs to the list whose centroid has the best QUANTISED score under dir_topk's order, i.e.
 *   dir_topk(dir_similarity_i8(row codes, row scale, centroid codes, centroid scales), k = 1): score descending, the
 *   larger list index among equal scores, NaN last.  A zero row (every score 0) and a non-finite row (every score NaN)
 *   therefore belong to list nlist - 1; that is the rule, not a special case.  The contents of an index do not depend on
 *   how the rows were cut into calls or chunks.
 * Probing: the lists of query q are dir_topk(dir_similarity_i8(q codes, q scale, centroid codes, centroid scales), nprobe),
 *   in that order.
 * Search: the candidates of q are the rows of its probed lists, their scores dir_similarity_i8's numbers
 *   ((float)dot_i32 * qscales[q]) * bscales[n], the result dir_topk of those with the rows' ids as ids (exclude for a query
 *   set that is the database); a query with fewer than k candidates ends in (-1, NaN) slots.  With a re-rank of R: the R
 *   best are kept, re-scored with dir_gather_scores against the fp32 rows addressed by id, and ranked again.
 * Training: spherical Lloyd iterations.  The initial centroids are nlist rows of the training sample; an iteration assigns
 *   every row by the rule above, sums the members of each list in fp32 (dir_segment_sums) and L2-normalises the sums
 *   (dir_l2norm_rows); an empty list keeps its centroid.  Bitwise reproducible from call to call.
 *
 * dir_segment_sums: sums[s][k] = sum of X[order[i]][k] over i in [seg_off[s], seg_off[s + 1]), fp32 accumulation in a fixed
 *   order (a function of the segment's length alone; no float atomics), so results are bitwise reproducible; each sum is
 *   within n_s * 2^-24 * sum |x| of the exact one (n_s rows; n_s / 16 + 4 additions on the longest path).  X [N][ldx] fp32
 *   (ldx >= D, any pitch), order [seg_off[S]] int32 with entries in [0, N) (an entry outside adds nothing), seg_off
 *   [S + 1] int32 ascending, sums [S][lds] fp32 (lds >= D); an empty segment gives zeros.  S <= 65535.
 * dir_ivf_scan_i8: the scores of every query against the rows of the lists it probes.  The probe table arrives INVERTED -
 *   by list, which is how the scan is cut (a workgroup multiplies up to 256 rows of one list with up to 32 of the queries
 *   that probe it: queries that share a list read it once) - and is the caller's duty, as ids are in dir_topk
 *   (dirtorch_amd/ops.py ivf_probe_tables builds it on the device from probe [Q][nprobe] and col_off [Q][nprobe]):
 *     a pair is one (query q, slot p) with probe[q][p] = l >= 0; the pairs are grouped by list,
 *     pair_off [nlist + 1]  CSR of the pairs by list,
 *     pair_q [pairs], pair_col [pairs]  the query of a pair and col_off[q][p], the first output column of the slot,
 *     item_off [nlist + 1]  CSR of the workgroups by list: list l takes ceil(len_l / 256) * ceil(pairs_l / 32) of them
 *                           (0 when either is 0), items = item_off[nlist] - the grid.
 *   For every pair and r < len_l: scores[q][col + r] = the quantised score of q against row list_off[l] + r, and
 *   out_ids[q][col + r] = ids[list_off[l] + r].  out_ids[q][0 .. width) is pre-filled with -1 BY THIS CALL (a fill kernel
 *   ahead of the scan), so a column no slot covers carries id -1 (its score is unspecified); columns at or past `width`
 *   of the [Q][lds] rows are not touched, and a pair whose columns would pass `width`, or whose query is outside [0, Q),
 *   stores nothing there.  qcodes [Q][ldq] and bcodes [N][ldb]: 16-byte aligned, pitches % 16 == 0 and >= D rounded up
 *   to 64, Q * ldq < 2^31; the query codes must be ZERO in bytes D .. D rounded up to 64 (dir_quantize_rows_i8 writes them
 *   so; both operands are read in 16-byte pieces and what the database holds there does not matter).  The slots of one
 *   query must not overlap.  Otherwise sim_i8_kernel's pipeline: LDS-DMA loaders (the query rows of a group gathered by
 *   a per-lane offset), v_mfma_i32_32x32x32_i8, K slabs of 128, four stages.
 *   `items` may be ANY upper bound of item_off[nlist] (dir_ivf_scan_fp4 too): a workgroup at or past item_off[nlist] finds
 *   no rows of the last list left for it and returns before it loads or stores anything, so a caller that knows a bound
 *   on the host (dir_ivf_plan's callers) need not read the count back.
 * Both: a negative count, D < 1, a pitch below its minimum or a null pointer fail with DIR_ERR_INVALID before anything is
 *   launched; S == 0, Q == 0 or width == 0 is DIR_OK and launches nothing.
 * dir_ivf_plan: the tables of both scans by list from probe [Q][nprobe] int32 and list_off [nlist + 1] int32, in ONE kernel
 *   launch on `stream` (ivf_plan.hip; one workgroup, the sort in LDS) and without a word coming back to the host; numpy
 *   restatement: tests/ivf_plan_ref.py.  len_l = list_off[l + 1] - list_off[l]; a slot whose list is outside [0, nlist) is
 *   EMPTY: length 0.  With P = Q * nprobe and the flat index f = q * nprobe + p of slot (q, p):
 *     col_off [Q][nprobe]   col_off[q][p] = the sum of the lengths of the slots (q, p') with p' < p: the lists of a query
 *                           side by side in probe order;
 *     pair_q, pair_col [P]  the slots in the order: by list ascending, inside a list by f ascending, the empty slots last
 *                           (by f ascending) - the order of a stable sort by list, whatever the launch; place i holds
 *                           q and col_off[q][p] of its slot;
 *     pair_off [nlist + 1]  the CSR of that order by list; pair_off[nlist] = the slots that are not empty;
 *     item_off [nlist + 1]  the CSR of ceil(len_l / 256) * ceil(pairs_l / 32), pairs_l = pair_off[l + 1] - pair_off[l];
 *     counts [2]            (item_off[nlist], reach), reach = the largest col_off[q][p] + the length of slot (q, p), 0
 *                           without a slot: for tests and measurements; a search does not read it.
 *   All int32; list_off ascending and item_off[nlist] and reach within int32 are the caller's duty.  These are, entry for
 *   entry, the tables dirtorch_amd/ops.py ivf_probe_tables makes.  nlist <= 65535 and P <= dir_ivf_plan_max_pairs()
 *   (host-only; 16384), else DIR_ERR_INVALID before anything is launched, as for a negative count, Q > 0 without a list
 *   or a null pointer; Q == 0 is DIR_OK and launches nothing. */
int dir_segment_sums(const float* X, int ldx, int N, int D, const int* order, const int* seg_off, int S, float* sums,
                     int lds, void* stream);
int dir_ivf_scan_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                    const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                    const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                    int lds, int width, void* stream);
int dir_ivf_plan_max_pairs(void);
int dir_ivf_plan(const int* probe, int Q, int nprobe, const int* list_off, int nlist, int* col_off, int* pair_off, int* pair_q,
                 int* pair_col, int* item_off, int* counts, void* stream);
/* The inverted file over fp4 codes (ivf_fp4.hip; dirtorch_amd/index.py IVFFp4Index; numpy restatement: tests/ivffp4_ref.py):
 * the inverted file's lists with the fp4 index's rows in them, 1 <= D <= dir_index_fp4_max_dim() = 7281.
 * Coarse side: the inverted-file int8 index's, unchanged - centroids [nlist][D] fp32 with their int8 codes and scales;
 *   assignment and probing by the quantised int8 score under dir_topk's order, exactly as above.  A row therefore lands in
 *   the same list in all three inverted files, and training is the int8 inverted file's.
 * Lists: a row is stored as dir_quantize_rows_fp4 gives it - codes [N][ldc] uint8, block bytes [N][lde] uint8, scales [N]
 *   fp32 - LIST-MAJOR with ids [N] int32 and list_off [nlist + 1] int32 as above, ids ascending inside a list.
 * Score: that of query q against row n of a probed list is dir_similarity_fp4's number, (acc * qscales[q]) * bscales[n], two
 *   fp32 multiplies in that order, with acc the exact sum: it does not depend on the tiling, the K order, the rotation,
 *   the grouping of the queries or the chunking.  CONSEQUENCE: with nprobe = nlist a search returns the fp4 index's lists
 *   bit for bit (dir_topk ranks the same set of (score, id) pairs); with fewer lists those of the numpy restatement.
 * dir_ivf_scan_fp4: dir_ivf_scan_i8's contract - the same inverted probe table (pair_off, pair_q, pair_col, item_off, items:
 *   256 rows a tile, 32 pairs a group), the same outputs: for every pair and r < len_l, scores[q][col + r] = the score
 *   above against row list_off[l] + r and out_ids[q][col + r] = ids[list_off[l] + r]; out_ids[q][0 .. width) pre-filled with
 *   -1 BY THIS CALL; columns at or past `width` untouched; a pair that would pass `width` or whose query is outside [0, Q)
 *   stores nothing.  qcodes [Q][ldq] and bcodes [N][ldb]: 16-byte aligned, pitches % 16 == 0 and >= D rounded up to 64,
 *   divided by 2 (need not cover a whole slab of 256 k: both sides are cut by 16-byte chunk in the last slab), Q * ldq <
 *   2^31; the query codes must be ZERO in the nibbles D .. D rounded up to 64 (dir_quantize_rows_fp4 writes them so; what
 *   the database holds there does not matter).  qexps [Q][ldqe] and bexps [N][ldbe]: 8-byte aligned, pitches % 8 == 0 and
 *   >= 8 * ceil(D / 256) - one 8-byte load per slab and row on BOTH sides; the bytes of blocks past D rounded up to 64 do
 *   not matter (they are replaced by 127), the others are e8m0 bytes other than 255.  The slots of one query must not
 *   overlap.  LDS-DMA loaders (the query rows of a group gathered by a per-lane offset),
 *   v_mfma_scale_f32_32x32x64_f8f6f4, K slabs of 256, four stages.
 *   A negative count, D < 1 or above the max dim, a pitch below its minimum or a null pointer fail with DIR_ERR_INVALID
 *   before anything is launched; Q == 0 or width == 0 is DIR_OK and launches nothing. */
int dir_ivf_scan_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                     const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, const int* ids, int N,
                     int D, const int* list_off, int nlist, const int* pair_off, const int* pair_q, const int* pair_col,
                     const int* item_off, int items, float* scores, int* out_ids, int lds, int width, void* stream);
/* The inverted file over sign-bit rows (ivf_bin.hip; dirtorch_amd/index.py IVFBinaryIndex; numpy restatement:
 * tests/ivfbin_ref.py): the inverted file's lists with the binary index's rows in them, 1 <= D <= dir_index_bin_max_dim() =
 * 131072.
 * Coarse side: the inverted-file int8 index's, unchanged, as for the fp4 inverted file: a row lands in the same list in all
 *   inverted files, and training is the int8 inverted file's.
 * Lists: a row is stored as dir_quantize_rows_bin gives it - bits [N][ldb] uint8, scales [N] fp32 - LIST-MAJOR with ids [N]
 *   int32 and list_off [nlist + 1] int32 as above, ids ascending inside a list.  The query side is dir_quantize_rows_i8's.
 * Score: that of query q against row n of a probed list is dir_similarity_bin's number, ((float)t * qscales[q]) * bscales[n],
 *   t = 2 * sum_k qcodes[q][k] * b_k - qsums[q] an exact int32: it does not depend on the tiling, the grouping of the
 *   queries or the chunking.  CONSEQUENCE: with nprobe = nlist a search returns the binary index's lists bit for bit; with
 *   fewer lists those of the numpy restatement.
 * dir_code_sums: qsums[q] = sum_{k < D} qcodes[q][k] for q < Q, int32 (index_bin.hip's code_sums_kernel, one wave per row);
 *   qcodes [Q][ldq] int8, ldq >= D, read up to D only.  The caller of the scan makes them once per query chunk.
 * dir_ivf_scan_bin: dir_ivf_scan_i8's contract with bits on the database side - the same inverted probe table (pair_off,
 *   pair_q, pair_col, item_off, items: 256 rows a tile, 32 pairs a group; `items` any upper bound), the same outputs: for
 *   every pair and r < len_l, scores[q][col + r] = the score above against row list_off[l] + r and out_ids[q][col + r] =
 *   ids[list_off[l] + r]; out_ids[q][0 .. width) pre-filled with -1 BY THIS CALL; columns at or past `width` untouched; a
 *   pair that would pass `width` or whose query is outside [0, Q) stores nothing.  qcodes [Q][ldq]: 16-byte aligned, ldq %
 *   16 == 0 and >= D rounded up to 64, Q * ldq < 2^31, ZERO in bytes D .. D rounded up to 64 (dir_quantize_rows_i8 writes
 *   them so) and read no further than that, whatever ldq is.  bits [N][ldb]: 16-byte aligned, ldb % 16 == 0 and >= D rounded
 *   up to 128, divided by 8, ldb * 256 < 2^31; what the bits past D hold does not matter: they meet zero query codes.
 *   qsums [Q] from dir_code_sums; the scan allocates nothing.  The slots of one query must not overlap.  LDS-DMA loaders
 *   (the query rows of a group gathered by a per-lane offset, cut by 16-byte chunk at D rounded up to 64),
 *   v_mfma_i32_32x32x32_i8 on bits widened to 0 / 1 code bytes in registers, K slabs of 1024 holding both operands, two
 *   stages of 64 KB, no K rotation.
 * Both: a negative count, D < 1 or above the max dim, a pitch below its minimum or a null pointer fail with DIR_ERR_INVALID
 *   before anything is launched; Q == 0 (or width == 0) is DIR_OK and launches nothing. */
int dir_code_sums(const int8_t* qcodes, int ldq, int Q, int D, int* qsums, void* stream);
int dir_ivf_scan_bin(const int8_t* qcodes, int ldq, const float* qscales, const int* qsums, int Q, const uint8_t* bits, int ldb,
                     const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                     const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                     int lds, int width, void* stream);
/* The product-quantised index (pq.hip; dirtorch_amd/index.py PQIndex; numpy restatement: tests/pq_ref.py).
 * A row of D fp32 values is cut into M sub-vectors of dsub = D / M values (M divides D, 1 <= M <= dir_pq_max_m(), D <=
 * dir_index_i8_max_dim()); sub-vector m is replaced by the number of one of the 256 centroids of sub-space m, so a row is
 * M bytes.  codebooks [M][256][dsub] fp32, contiguous.  Every number below is a chain of single IEEE fp32 operations
 * rounded to nearest (no fused multiply-add), in the stated order: it does not depend on tiling, chunking or the number
 * of calls, and a numpy float32 restatement reproduces it bit for bit.
 *   Encoding of row x, sub-space m:  dist_j = (((+0 + t_0 * t_0) + t_1 * t_1) + ...), t_d = x[m * dsub + d] - c[m][j][d],
 *     d = 0 .. dsub - 1.  code_m = the result of  best = 0; for j = 1 .. 255: if dist_j < dist_best, or dist_best is a NaN
 *     and dist_j is not: best = j  - the smallest distance, the smaller j among equal distances, a NaN distance never
 *     chosen over a number; a row that holds a NaN has code 0 in the sub-spaces the NaN falls into.
 *   Table of query q:  lut[q][m][j] = (((+0 + q_0 * c_0) + q_1 * c_1) + ...) over the dsub values of sub-space m.
 *   Score:  score[q][n] = (((+0 + lut[q][0][code[n][0]]) + lut[q][1][code[n][1]]) + ...), m = 0 .. M - 1: the inner
 *     product of the query with the row's centroids (asymmetric distance computation), one defined fp32 number per pair.
 * dir_pq_max_m (host-only; 128): the largest M - one query's table, M KiB, has to fit the 160 KiB of LDS.
 * dir_pq_encode: X [N][ldx] fp32 (ldx >= D, any pitch) -> codes [N][ldc] uint8, ldc >= M and ldc % 4 == 0.  Bytes M .. M
 *   rounded up to a multiple of 4 of every row are written as zero; bytes past that are not touched.  One workgroup per
 *   (sub-space, 256 rows): thread j holds centroid j's distances to 32 rows at a time, the arg-min is a minimum of
 *   (distance bits, j) keys.  At most 2^31 - 1 workgroups: N * M / 256 rows of them.
 * dir_pq_lut: queries [Q][ldq] fp32 (ldq >= D) -> lut [Q][M][256] fp32, contiguous.
 * dir_pq_scan: lut [Q][M][256] (16-byte aligned), codes [N][ldc] uint8 (4-byte aligned, ldc >= M, ldc % 4 == 0; what the
 *   bytes past M hold does not matter) -> scores [Q][lds] fp32, lds >= N; columns at or past N are not touched.  A
 *   workgroup of 1024 threads keeps the codes of a tile of 2048 rows (1024 for M > 64) in registers and walks the
 *   queries two at a time, their tables interleaved in LDS (64 sub-spaces at a time for M > 64).
 * All three: a negative count, D < 1 or above the max dim, M outside 1 .. dir_pq_max_m(), M not dividing D, a pitch below
 *   its minimum, ldc % 4 != 0, a misaligned lut / codes or a null pointer fail with DIR_ERR_INVALID before anything is
 *   launched; Q == 0 or N == 0 is DIR_OK and launches nothing.
 * Training (PQIndex.train): Lloyd iterations per sub-space.  The initial centroids are 256 rows of the training sample,
 *   sub-space m taking columns m * dsub .. of them; an iteration encodes the sample (dir_pq_encode is the assignment), sums
 *   the members of every centroid in fp32 (dir_segment_sums on the sub-space's columns, members in ascending row order)
 *   and divides each sum by the member count (one fp32 division); a centroid without members keeps its value.
 * Search: dir_topk of the scores, exactly as the flat int8 index ranks its own; with a re-rank of R the R best are
 *   re-scored with dir_gather_scores against the fp32 rows and ranked again. */
int dir_pq_max_m(void);
int dir_pq_encode(const float* X, int ldx, int N, int D, int M, const float* codebooks, uint8_t* codes, int ldc, void* stream);
int dir_pq_lut(const float* queries, int ldq, int Q, int D, int M, const float* codebooks, float* lut, void* stream);
int dir_pq_scan(const float* lut, int Q, int M, const uint8_t* codes, int ldc, int N, float* scores, int lds, void* stream);
/* The IVF-PQ index (ivfpq.hip; dirtorch_amd/index.py IVFPQIndex; numpy restatement: tests/ivfpq_ref.py): the inverted file
 * above with M-byte product-quantiser codes of RESIDUALS in its lists.  The house rule holds: every number is a chain of
 * single IEEE fp32 operations in the stated order (no fused multiply-add).  An index of width D, nlist lists and M
 * sub-spaces (M divides D, 1 <= M <= dir_pq_max_m(), dsub = D / M) holds
 *     the coarse quantiser of the inverted int8 index, unchanged: centroids [nlist][D] fp32 with their int8 codes and
 *       scales.  ASSIGNMENT and PROBING are the rules written there (dir_topk of dir_similarity_i8 against the quantised
 *       centroids): a row lands in the same list in both indexes,
 *     codebooks [M][256][dsub] fp32,
 *     the database LIST-MAJOR: codes [N][ldc] uint8 (ldc = M rounded up to 4, the padding zero), ids [N] int32, list_off
 *       [nlist + 1] int32; rows ascend in id inside a list, and the store does not depend on how the rows were cut into
 *       add calls.
 *   Residual of row x in list l:  r_d = x_d - centroids[l][d], one fp32 subtraction per element against the fp32 centroid
 *     (not its dequantised code).  The codes of the row are dir_pq_encode of r.
 *   Coarse term of query q and list l:  s_m = (((+0 + q_{m,0} c_{m,0}) + q_{m,1} c_{m,1}) + ...) over the dsub columns of
 *     sub-space m of centroids[l], in column order;  base[q][l] = (((+0 + s_0) + s_1) + ... + s_{M-1}).
 *   Score of q against row n of a probed list l:  (((base[q][l] + lut[q][0][code[n][0]]) + lut[q][1][code[n][1]]) + ...),
 *     m ascending, lut = dir_pq_lut(q, codebooks): for inner products the table does not depend on the list, and the
 *     chain starts at the coarse term instead of +0.
 *   Search: the candidates of q are the rows of its nprobe probed lists, the result dir_topk of their scores with the rows'
 *     ids as ids (exclude for a query set that is the database); a row that runs short ends in (-1, NaN).  With a re-rank of
 *     R the R best are re-scored with dir_gather_scores against the fp32 rows addressed by id and ranked again.
 *   Training: 1. the coarse centroids exactly as the inverted int8 index trains them (same sample, same start rows, same
 *     iterations); 2. the codebooks exactly as the product-quantised index trains them, on the residuals of that same
 *     sample to the final centroids of the lists its rows are assigned to.  Bitwise reproducible from call to call.
 *
 * dir_ivfpq_scan_cols (host-only; 1024): the output columns a workgroup of the scan owns.
 * dir_ivfpq_base: queries [Q][ldq] fp32 (ldq >= D), centroids [nlist][ldc] fp32 (ldc >= D), probe [Q][nprobe] int32 ->
 *   base [Q][nprobe] fp32, contiguous: the coarse term of every slot; a slot outside [0, nlist) (-1 = empty) stores a NaN.
 *   One workgroup per slot, one thread per sub-space chain, then the M partial sums added in order.
 * dir_ivfpq_scan: lut [Q][M][256] (16-byte aligned), base, probe, col_off [Q][nprobe] (contiguous), codes [N][ldc] uint8
 *   (4-byte aligned, ldc >= M, ldc % 4 == 0; what the bytes past M hold does not matter), ids [N], list_off [nlist + 1] ->
 *   scores [Q][lds] fp32 and out_ids [Q][lds] int32 over `width` columns, with dir_ivf_scan_i8's output contract: for every
 *   slot p of query q with l = probe[q][p] >= 0 and r < len_l, column col_off[q][p] + r carries the score of row list_off[l]
 *   + r and ids[list_off[l] + r]; a column of [0, width) that no slot covers carries id -1 (its score is unspecified);
 *   columns at or past `width` are not touched, and a slot stores nothing there.  The slots of one query must not overlap;
 *   a list outside [0, nlist) is an empty slot, and rows at or past N are not read.  Cut QUERY-major - the expensive operand
 *   is the query's table, M KiB of LDS, not the M-byte rows: a workgroup of 1024 threads owns one query and 1024 consecutive
 *   output columns, stages the table once, finds the slot of each column from the col_off row and adds the entries of the
 *   row's codes (held in registers) in the order m = 0 .. M - 1 starting from base.  No inverted probe table, no sort, no
 *   fill kernel and no host synchronisation: the grid is Q * ceil(width / 1024).
 * Both: a negative count, a bad D or M (as dir_pq_lut), a pitch below its minimum, ldc % 4 != 0, lds < width, a misaligned
 *   lut / codes or a null pointer fail with DIR_ERR_INVALID before anything is launched; Q == 0, nprobe == 0 (base) or
 *   width == 0 (scan) is DIR_OK and launches nothing. */
int dir_ivfpq_scan_cols(void);
int dir_ivfpq_base(const float* queries, int ldq, int Q, const float* centroids, int ldc, int nlist, int D, int M,
                   const int* probe, int nprobe, float* base, void* stream);
int dir_ivfpq_scan(const float* lut, const float* base, int Q, int M, const uint8_t* codes, int ldc, const int* ids, int N,
                   const int* list_off, int nlist, const int* probe, const int* col_off, int nprobe, float* scores,
                   int* out_ids, int lds, int width, void* stream);
/* N3: alpha query expansion / database augmentation, expand_descriptors of
 * dirtorch/test_dir.py:24-44.  out[i] = normalize(mean(descs[i], sim[i][j]^alpha * db[j] for the k
 * rows j of db most similar to descs[i])), sim = descs . db^T in fp32; self_set != 0 (db == descs,
 * m == n): a row is not its own neighbour (its self-similarity counts as 0, test_dir.py:33-34).
 * descs [n][D], db [m][D], out [n][D] fp32 contiguous; sim: caller's scratch of sim_bytes >= 4*m
 * (rows are processed in chunks of sim_bytes / (4*m)); 0 <= k <= m, alpha >= 0.  A row whose similarities are
 * not finite yields a NaN row (the reference propagates NaN the same way). */
int dir_expand_descriptors(const float* descs, int n, const float* db, int m, int D, int k, float alpha,
                           int self_set, float* out, float* sim, size_t sim_bytes, void* stream);
/* The same expansion from neighbour LISTS (expand_lists.hip; dirtorch_amd/ranking.py expand_device; numpy restatement:
 * tests/expand_ref.py): the k neighbours of every row arrive as dir_topk writes them - exact, or from any of the index
 * classes - so neither the n x m score matrix nor a selection pass over it exists.  descs [n][ldd], db [m][ldb] and out
 * [n][ldo] fp32 with any pitch >= D; idx / vals [n][ldl] int32 / fp32, ldl >= k, best first.  The house rule of the index
 * blocks holds: every number is a chain of single IEEE fp32 operations rounded to nearest, in the stated order (no fused
 * multiply-add), and a numpy float32 restatement reproduces it bit for bit - except powf, below.
 *   Weight:  w_t = vals[i][t]^alpha.  alpha an integer in 0 .. 64: w = 1, then alpha times w = w * v (what
 *     expand_rows_kernel does); otherwise powf(v, alpha), the one step that is not bit-defined.
 *   Sum:  acc_d = descs[i][d]; for t = 0 .. k - 1 ascending with idx[i][t] >= 0:  acc_d = acc_d + (db[idx[i][t]][d] * w_t),
 *     the product rounded, then the sum.  A slot with idx < 0 (a list that ran short) contributes nothing and its vals
 *     entry is not read; an id outside [-1, m) is undefined (the caller's duty, as ids in dir_topk).
 *   Mean:  acc_d = acc_d * inv, inv = 1.f / (float)(k + 1): the reference's mean over k + 1 rows, however many slots are
 *     empty.
 *   Norm:  column d belongs to lane tau = (d mod 1024) / 4 of 256.  p[tau] = the chain p = p + acc_d * acc_d over the lane's
 *     columns in ascending d, from +0; then for s = 128, 64, .., 1: p[tau] = p[tau] + p[tau + s] for tau < s;
 *     out[i][d] = acc_d / sqrtf(p[0]), one division.  A NaN weight or row gives a NaN row, as the reference's arithmetic
 *     does, and touches no other row.
 * k == 0 is allowed and normalises descs (idx and vals may then be NULL).  out must not overlap descs or db: with db ==
 * descs (DBA) other rows still read what a row would overwrite.
 * One workgroup of 256 threads per output row, no scratch and no atomics; a lane reads its four columns of a span as one
 * 16-byte load when D % 4 == 0 and descs, db and out are 16-byte aligned with pitches % 4 == 0, as four scalars otherwise;
 * the rows of four picks are requested before the first is added.  It reads (k + 1) * 4 D bytes per output row.
 * A negative count, D < 1, a pitch below its minimum, ldl < k, alpha < 0 (or NaN) or a null pointer fail with
 * DIR_ERR_INVALID before anything is launched; n == 0 is DIR_OK and launches nothing. */
int dir_expand_lists(const float* descs, int ldd, int n, const float* db, int ldb, int m, int D, const int* idx,
                     const float* vals, int ldl, int k, float alpha, float* out, int ldo, void* stream);
/* Diffusion re-ranking on the kNN graph of the database (diffusion.hip; dirtorch_amd/ranking.py knn_graph_device /
 * diffuse_device; numpy restatement: tests/diffusion_ref.py): Iscen et al., "Efficient Diffusion on Region Manifolds", in
 * its global-descriptor form.  The house rule holds: every number is a chain of single IEEE fp32 operations rounded to
 * nearest, in the stated order (no fused multiply-add), and a numpy float32 restatement reproduces it bit for bit - except
 * powf, below.
 * GRAPH (dir_knn_graph).  idx / vals [N][ldl] int32 / fp32 are the self-set lists of the database, k slots a row, as
 *   dir_topk or an index's search(same_set) writes them; S [N][lds] fp32 is the graph in the same layout (ldl, lds >= k).
 *   Slot (i, t) is LIVE when j = idx[i][t] has 0 <= j < N and j != i, no earlier slot of row i holds j, and vals[i][t] > 0
 *     (a NaN fails).  Every other slot - a -1 hole, an id out of range, the row itself, a later duplicate, a score that is
 *     zero, negative or NaN - has S = +0 and its id is never dereferenced.
 *   w(i,t) = vals[i][t]^gamma: gamma an integer in 0 .. 64: w = 1, then gamma times w = w * v; otherwise powf(v, gamma), the
 *     one step that is not bit-defined (dir_expand_lists' rule).
 *   a(i,t) = min(w(i,t), w(j,t')), t' the first live slot of row j that holds i; +0 when there is none.  Mutual edges only:
 *     the graph is a subset of every row's own list and symmetric bit for bit.
 *   deg[i] = the chain deg = deg + a(i,t) over t ascending from +0;  dinv[i] = 1 / sqrtf(deg[i]) when deg[i] > 0 (two
 *     correctly rounded operations), else 0;  S[i][t] = a(i,t) * (dinv[i] * dinv[j]), the product of the two dinv first, so
 *     S is symmetric bit for bit as well; a slot with a(i,t) == 0 keeps +0.  A row of degree 0 is isolated: all zero.
 *   Three kernels (one thread per slot, per row, per slot); dinv lives in stream-ordered scratch.
 * SEEDS (dir_diffusion_seed).  qidx / qvals [Q][ldq], the kq best database rows of every query; Y [N][ldy] fp32, ldy >= Q.
 *   Columns 0 .. Q of every row of Y are set to +0 by this call, then for every query q and t = 0 .. kq - 1 ascending with
 *   0 <= j = qidx[q][t] < N and qvals[q][t] > 0:  Y[j][q] = qvals[q][t]^gamma (the power above).  A later slot of a list that
 *   names the same row overwrites an earlier one; any other slot writes nothing.  The queries are a set of their own: there
 *   is no self test.  Columns at or past Q are not touched.
 * SOLVE (dir_diffusion_solve).  (I - alpha S) f = y for each of the Q columns of Y by conjugate gradients, `iters`
 *   iterations, no early exit and no host synchronisation; the columns are independent.  Per column, x r p ap over the N rows:
 *       x = 0; r = y; p = y; rr = dot(r, r)
 *       repeat iters times:
 *           g[i]  = the chain g = g + S[i][t] * p[idx[i][t]] over t ascending from +0 (product, then sum) - over the slots
 *                   with 0 <= idx[i][t] < N and S[i][t] != 0; any other slot is skipped and its id is not dereferenced
 *           ap[i] = p[i] - alpha * g[i]                                   (product, then difference)
 *           pap = dot(p, ap);    a = pap > 0 ? rr / pap : 0
 *           x[i] = x[i] + a * p[i];    r[i] = r[i] - a * ap[i];    rn = dot(r, r)
 *           b = rr > 0 ? rn / rr : 0;    p[i] = r[i] + b * p[i];    rr = rn
 *       f = x
 *   dot(u, v): the rows are cut into slabs of dir_diffusion_slab_rows() = 256 consecutive rows (host-only query).  Row r
 *     of a slab belongs to chain r mod 64; chain c = the sum c = c + u[i] * v[i] over its rows in ascending order from +0
 *     (a row at or past N ends the chain); then for s = 32, 16, 8, 4, 2, 1: chain[c] = chain[c] + chain[c + s] for c < s; the
 *     slab's partial is chain[0].  dot = the chain d = d + partial over the slabs in ascending order from +0.  Nothing in
 *     this order depends on the CU count, on Q, on a pitch or alignment, or on how the columns are blocked: solving the same
 *     columns in one call or in several gives the same bits.
 *   Consequences: alpha = 0 gives F = Y bit for bit after one iteration; a zero column stays zero; iters = 0 gives F = 0.
 *   idx [N][ldl], S [N][lds], Y [N][ldy], F [N][ldf] (ldy, ldf >= Q; F must not overlap the other operands).  workspace: at
 *   least dir_diffusion_workspace_bytes(N, Q) bytes (host-only), 16-byte aligned; it holds x r p ap as [N][Qp] fp32, Qp = Q
 *   rounded up to 4 with zero padding columns, the slab partials and rr, a, b.  Per iteration: the apply kernel (ap and the
 *   slab partials of pap; a lane owns four columns - one 16-byte load per gathered row - of one chain of a slab and takes
 *   two of its rows at a time, the rows of four slots of each are requested before the first is added and the next four
 *   ids and weights before those adds; a skipped slot reads the lane's own row instead and its add is dropped by a
 *   select), one thread per column that finishes pap and writes a, the x / r update with the slab partials
 *   of rn, one thread per column that writes b and rr, and the p update.  No atomics.
 * All three: a negative count, a pitch below its width, k or kq above dir_topk_max_k(), gamma < 0 (or NaN), alpha outside
 * [0, 1), N * k (graph) or N * Q (seeds, solve) at or above 2^32 - 256 (the pointwise kernels take one thread per slot or
 * element), a null pointer, a short or misaligned workspace fail with DIR_ERR_INVALID before anything is launched; N == 0 or
 * Q == 0 (k == 0 for the graph) is DIR_OK and launches nothing. */
int dir_diffusion_slab_rows(void);
int dir_knn_graph(const int* idx, const float* vals, int ldl, int N, int k, float gamma, float* S, int lds, void* stream);
int dir_diffusion_seed(const int* qidx, const float* qvals, int ldq, int Q, int kq, int N, float gamma, float* Y, int ldy,
                       void* stream);
int dir_diffusion_workspace_bytes(int N, int Q, size_t* bytes);
int dir_diffusion_solve(const int* idx, int ldl, const float* S, int lds, int N, int k, const float* Y, int ldy, int Q,
                        float alpha, int iters, float* F, int ldf, void* workspace, size_t workspace_bytes, void* stream);
/* Truncated diffusion (diffusion_local.hip; dirtorch_amd/ranking.py diffuse_truncated_device; numpy restatement:
 * tests/diffusion_trunc_ref.py): the system of a query restricted to its T best database rows, as Iscen et al. do at query
 * time.  The same house rule: every number a chain of single fp32 operations in the stated order, no fused multiply-add,
 * powf of a non-integer gamma the one exception.  1 <= T <= dir_diffusion_local_max_rows() (host-only; = dir_topk_max_k(),
 * 2048), k <= dir_topk_max_k().
 * INPUTS.  The graph idx / S [N][ldl / lds] as dir_knn_graph writes it; per query a candidate list cidx / cvals [Q][ldc]
 *   with T slots, best first, as dir_topk or an index's search writes it.
 * LIVENESS.  Candidate slot a of query q is live when 0 <= cidx[q][a] < N and no earlier slot of the list holds the same
 *   id; cid[q][a] is the id when live, else -1.  A dead candidate is a row without edges or seed; its id is never
 *   dereferenced.
 * SUBGRAPH (dir_diffusion_subgraph).  lidx / lw [Q][k][ldt] int32 / fp32, slot-major (ldt >= T), and the seeds y [Q][ldt];
 *   cid [Q][ldt].  For a live a with i = cid[q][a] and slot t, j = idx[i][t]: when S[i][t] != 0, 0 <= j < N and j is the id
 *   of live candidate b of the same query, lidx[q][t][a] = b and lw[q][t][a] = S[i][t]; otherwise -1 and +0.  Every slot of
 *   a dead row is -1 / +0.  The local matrix is a principal sub-matrix of the symmetric S: symmetric bit for bit.
 *   one_hot == 0: y[q][a] = cvals[q][a]^gamma (dir_knn_graph's power rule) for a < kq, live, cvals[q][a] > 0; else +0.
 *   one_hot != 0: y[q][0] = 1 when slot 0 is live; everything else +0 (the query is candidate 0, a database row; cvals is
 *   not read).  Columns at or past T of cid, lidx, lw and y are not touched.
 *   One workgroup per query: the T ids go into an LDS hash table whose entry keeps the MINIMUM slot that holds an id (an
 *   LDS atomic min, so the result does not depend on the order of the insertions), then T x k look-ups.  No global atomics.
 * SOLVE (dir_diffusion_solve_local).  Per query, the recurrence of dir_diffusion_solve verbatim on the T local rows, one
 *   column, dot() being that entry's with N := T (slabs of 256 rows, 64 chains, the tree, the partials in slab order): the
 *   result is what dir_diffusion_solve gives on (lidx[q]^T, lw[q]^T, y[q]) as a one-column problem, bit for bit.  A slot with
 *   lidx outside [0, T) or lw == 0 is skipped.  f[q][a] = x[a], NaN where cid[q][a] < 0 (cid may be null: all live);
 *   f [Q][ldf], ldf >= T.  alpha = 0 returns y after one iteration, iters = 0 returns 0, a zero seed stays zero.
 *   One workgroup per query and ONE launch for all iterations: p and the products of a dot live in LDS (16 KiB), x r ap of
 *   a row in the registers of the lane that owns it; a lane walks the k slots of its rows in slot order from the slot-major
 *   arrays, the next four ids and weights requested before the current four adds; a skipped slot is a select.  a, b and rr
 *   are computed by one thread and broadcast through LDS.  No workspace, no scratch, no atomics.
 * SPREAD (dir_diffusion_spread).  scores [Q][lds] fp32 (the plain similarities, lds >= N) in place, two kernels in stream
 *   order: scores[q][j] = scores[q][j] - 4 for every j < N; then for every live candidate scores[q][cid[q][a]] =
 *   f[q][a] > -2 ? f[q][a] : -2 (a NaN becomes -2); cid and f [Q][ldt].  Cosines lie in [-1, 1], hence in [-5, -3] after
 *   the shift: every candidate outranks every non-candidate and the non-candidates keep their cosine order.
 * All three: a negative count, a pitch below its width, T or k above the limits (T < 1 for the first two), gamma < 0 or
 * alpha outside [0, 1) (or NaN), Q * 1024 (subgraph, solve) or Q * N, Q * T (spread) at or above 2^32 - 256, a null pointer
 * fail with DIR_ERR_INVALID before anything is launched; Q == 0 (N == 0 for the spread) is DIR_OK and launches nothing. */
int dir_diffusion_local_max_rows(void);
int dir_diffusion_subgraph(const int* idx, int ldl, const float* S, int lds, int N, int k, const int* cidx, const float* cvals,
                           int ldc, int Q, int T, int kq, float gamma, int one_hot, int* cid, int* lidx, float* lw, float* y,
                           int ldt, void* stream);
int dir_diffusion_solve_local(const int* lidx, const float* lw, int k, const float* y, const int* cid, int ldt, int Q, int T,
                              float alpha, int iters, float* f, int ldf, void* stream);
int dir_diffusion_spread(float* scores, int lds, int Q, int N, const int* cid, const float* f, int ldt, int T, void* stream);

/* ---- the exchange step ------------------------------------------------------------
 * All-gather of per-GPU descriptor blocks over RCCL / xGMI for ONE process driving several GPUs - the
 * shape of the reference's nn.DataParallel use (dirtorch/utils/common.py:150-175).  One process per
 * GPU reaches the same collective through torch.distributed (dirtorch_amd/distributed.py).  librccl is
 * bound at first use (dlopen): without it these calls fail with DIR_ERR_STATE, nothing else changes.
 *   dir_comm_init_all   ncclCommInitAll over devices[0..ndev) (NULL = 0..ndev-1)
 *   dir_allgather_desc  rank i contributes send[i] = [rows][D] fp32 on device i and receives
 *                       recv[i] = [ndev*rows][D] (rank order = shard order; equal `rows` per rank - the
 *                       caller pads the last shard and trims after, as distributed.py does);
 *                       streams[i] = the stream of device i to enqueue on (NULL array = default streams) */
typedef struct dir_comm dir_comm;
int dir_comm_init_all(int ndev, const int* devices, dir_comm** out);
int dir_comm_size(const dir_comm* c, int* ndev);
int dir_comm_destroy(dir_comm* c);
int dir_allgather_desc(dir_comm* c, const float* const* send, float* const* recv, size_t rows, int D,
                       void* const* streams);

#ifdef __cplusplus
}
#endif
#endif /* DIR_ENGINE_H */
