"""Tensor-level wrappers of the per-op C-ABI entry points (include/dir_engine.h).

torch is used for device memory and the current stream only; every computation below is a HIP
kernel of libdir_engine.so.  16-bit activations travel as torch.bfloat16 / torch.float16 tensors in
NHWC layout.
"""
import ctypes
import functools

import torch

from . import _lib
from ._lib import DIR_BF16, DIR_FP16, POOLING, call, ptr, stream_ptr


def _dtype_code(t):
    if t.dtype == torch.bfloat16:
        return DIR_BF16
    if t.dtype == torch.float16:
        return DIR_FP16
    raise TypeError('16-bit activation tensor expected (bfloat16 or float16), got %s' % t.dtype)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError('device tensor expected')
        if t is not None and not t.is_contiguous():
            raise ValueError('contiguous tensor expected')


def conv_variant_names():
    lib = _lib.load()
    out = []
    for v in range(lib.dir_conv_variant_count()):
        buf = ctypes.create_string_buffer(64)
        call('dir_conv_variant_name', v, buf, 64)
        out.append(buf.value.decode())
    return out


class overflow_watch:
    """with ops.overflow_watch() as watch: ... - every 16-bit per-op launch inside the block reports into one zeroed device
    word, as an engine's launches report into the engine's (include/dir_engine.h, dir_engine_overflow): bit 0 = an fp16 store
    overflowed, bit 1 = a bounded LDS-counter wait ran out.  watch.read() synchronises the device, returns the word as an int
    and zeroes it (sticky until then).  The hook behind it is process-wide, not thread-scoped, and blocks do not nest: a
    diagnostic tool for tests.  Leaving the block clears the hook."""

    def __init__(self, device=None):
        self._device = device
        self._word = None

    def __enter__(self):
        self._word = torch.zeros(1, dtype=torch.int32, device=self._device or 'cuda')
        torch.cuda.synchronize()      # the word is zero before any launch on any stream can report
        _lib.set_op_overflow_word(self._word.data_ptr())
        return self

    def read(self):
        torch.cuda.synchronize()
        value = int(self._word.item())
        self._word.zero_()
        torch.cuda.synchronize()
        return value

    def __exit__(self, *exc):
        _lib.set_op_overflow_word(None)
        torch.cuda.synchronize()      # no kernel that still holds the word outlives it
        self._word = None
        return False


def pack_conv_weight(w_oihw, dtype=torch.bfloat16):
    """OIHW fp32 -> [Cout][R][S][Cin] 16-bit (what dir_conv_bn_act expects)."""
    return w_oihw.permute(0, 2, 3, 1).contiguous().to(dtype)


def pack_stem_weight(w_oihw, dtype=torch.bfloat16):
    """7x7 s2 stem weight [64,3,7,7] -> 4x4 s1 space-to-depth form [64][4][4][16]
    (tap r = 2R + dy - 1, s = 2S + dx - 1, channel (dy*2+dx)*3 + c); mirrors engine.hip."""
    O = w_oihw.shape[0]
    out = torch.zeros(O, 4, 4, 16, dtype=torch.float32, device=w_oihw.device)
    for R in range(4):
        for S in range(4):
            for dy in range(2):
                for dx in range(2):
                    r, s = 2 * R + dy - 1, 2 * S + dx - 1
                    if 0 <= r < 7 and 0 <= s < 7:
                        c0 = (dy * 2 + dx) * 3
                        out[:, R, S, c0:c0 + 3] = w_oihw[:, :, r, s]
    return out.to(dtype)


def conv_bn_act_f32(x, w, bias, res=None, stride=1, pad=0, relu=True):
    """The strict path's convolution (dir_conv_bn_act_f32, conv_f32.hip): x NHWC [B,H,W,Cin] fp32,
    w [Cout,R,S,Cin] fp32, bias fp32 [Cout], res NHWC fp32 or None -> NHWC [B,OH,OW,Cout] fp32."""
    _need_cuda(x, w, bias, res)
    for t in (x, w, bias, res):
        if t is not None and t.dtype != torch.float32:
            raise TypeError('fp32 tensors expected')
    B, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w.shape
    if Cin2 != Cin:
        raise ValueError('Cin mismatch')
    OH = (H + 2 * pad - R) // stride + 1
    OW = (W + 2 * pad - S) // stride + 1
    y = torch.empty(B, OH, OW, Cout, dtype=torch.float32, device=x.device)
    call('dir_conv_bn_act_f32', ptr(x), ptr(w), ptr(bias), ptr(res), ptr(y), B, H, W, Cin, Cout, R, S, stride, pad,
         OH, OW, int(bool(relu)), stream_ptr())
    return y


def conv_bn_act(x, w, bias, res=None, stride=1, pad=0, relu=True, out_hw=None, variant=-1,
                naive=False, ksplit=None):
    """x NHWC [B,H,W,Cin] 16-bit, w [Cout,R,S,Cin] 16-bit, bias fp32 [Cout] -> NHWC [B,OH,OW,Cout].
    ksplit: None = plain launch; n > 1 = split-K into n slices; -1 = the engine's own choice
    (conv_bn_act.last_ksplit holds what was used; the fp32 scratch is sized for that factor, none when nothing splits)."""
    _need_cuda(x, w, bias, res)
    B, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w.shape
    if Cin2 != Cin:
        raise ValueError('Cin mismatch')
    if out_hw is None:
        OH = (H + 2 * pad - R) // stride + 1
        OW = (W + 2 * pad - S) // stride + 1
    else:
        OH, OW = out_hw
    y = torch.empty(B, OH, OW, Cout, dtype=x.dtype, device=x.device)
    args = [ptr(x), ptr(w), ptr(bias), ptr(res), ptr(y), B, H, W, Cin, Cout, R, S, stride, pad, OH,
            OW, int(bool(relu)), _dtype_code(x)]
    if ksplit is not None:
        n = max(int(ksplit), 1)
        if ksplit < 0:      # the engine's own factor for this launch: a host-only query, so that only its slices are reserved
            q = ctypes.c_int()
            shape = (B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, int(res is not None))
            if variant < 0:
                call('dir_conv_heuristic', *shape, ctypes.create_string_buffer(64), 64, ctypes.byref(q))
            else:
                call('dir_conv_variant_splitk', int(variant), *shape, ctypes.byref(q))
            n = q.value
        scratch = torch.empty(n * B * OH * OW * Cout if n > 1 else 0, dtype=torch.float32, device=x.device)
        used = ctypes.c_int()
        call('dir_conv_bn_act_splitk', *args, int(variant), int(ksplit), ptr(scratch), scratch.numel() * 4,
             ctypes.byref(used), stream_ptr())
        conv_bn_act.last_ksplit = used.value
    elif naive:
        call('dir_conv_bn_act_naive', *args, stream_ptr())
    else:
        call('dir_conv_bn_act', *args, int(variant), stream_ptr())
    return y


def conv_c3c1(t2, w3, bias3, res, w1, bias1, relu3=True, relu1=True):
    """Fused bottleneck seam (dir_conv_c3c1): returns (y [B,H,W,4P], t1 [B,H,W,P2]).
    t2 [B,H,W,P], w3 [4P,1,1,P] or [4P,P], res [B,H,W,4P], w1 [P2,1,1,4P] or [P2,4P]; 16-bit NHWC, fp32 biases."""
    _need_cuda(t2, w3, bias3, res, w1, bias1)
    B, H, W, P = t2.shape
    P2 = w1.shape[0]
    y = torch.empty(B, H, W, 4 * P, dtype=t2.dtype, device=t2.device)
    t1 = torch.empty(B, H, W, P2, dtype=t2.dtype, device=t2.device)
    call('dir_conv_c3c1', ptr(t2), ptr(w3), ptr(bias3), ptr(res), ptr(y), ptr(w1), ptr(bias1), ptr(t1), B, H, W, P, P2,
         int(bool(relu3)), int(bool(relu1)), _dtype_code(t2), stream_ptr())
    return y, t1


def conv_c3c1_ds(t2, x, wcat, bias, w1, bias1, relu3=True, relu1=True):
    """Fused seam with the downsample branch folded in as extra K (dir_conv_c3c1_ds): t2, x [B,H,W,64],
    wcat [256, 128] = [w3 | wds], bias = bias3 + bias_ds -> (y [B,H,W,256], t1 [B,H,W,64])."""
    _need_cuda(t2, x, wcat, bias, w1, bias1)
    B, H, W, P = t2.shape
    y = torch.empty(B, H, W, 256, dtype=t2.dtype, device=t2.device)
    t1 = torch.empty(B, H, W, 64, dtype=t2.dtype, device=t2.device)
    call('dir_conv_c3c1_ds', ptr(t2), ptr(x), ptr(wcat), ptr(bias), ptr(y), ptr(w1), ptr(bias1), ptr(t1), B, H, W,
         int(bool(relu3)), int(bool(relu1)), _dtype_code(t2), stream_ptr())
    return y, t1


def conv_c3c1_wpair(t2, w3, bias3, res, w1, bias1, relu3=True, relu1=True):
    """The fused seam with paired weights (dir_conv_c3c1_wpair, fp16, planes 64): w3 = (hi, lo) [256, 64], w1 = (hi, lo)
    or (hi, None) [P2, 256]; t2 [B,H,W,64], res [B,H,W,256] single fp16 planes -> (y [B,H,W,256], t1 [B,H,W,P2])."""
    (w3h, w3l), (w1h, w1l) = w3, w1
    _need_cuda(t2, w3h, w3l, bias3, res, w1h, bias1)
    B, H, W, P = t2.shape
    P2 = w1h.shape[0]
    y = torch.empty(B, H, W, 4 * P, dtype=t2.dtype, device=t2.device)
    t1 = torch.empty(B, H, W, P2, dtype=t2.dtype, device=t2.device)
    call('dir_conv_c3c1_wpair', ptr(t2), ptr(w3h), ptr(w3l), ptr(bias3), ptr(res), ptr(y), ptr(w1h),
         ptr(w1l) if w1l is not None else None, ptr(bias1), ptr(t1), B, H, W, P2, int(bool(relu3)), int(bool(relu1)), stream_ptr())
    return y, t1


def _seam_y(y, res):
    """The caller's block-output tensor (res itself = in place), or a fresh one."""
    if y is None:
        return torch.empty_like(res)
    _need_cuda(y)
    if y.shape != res.shape or y.dtype != res.dtype:
        raise ValueError('y must have the shape and dtype of res')
    return y


def conv_c3c1_keep(t2, w3, bias3, res, w1, bias1, keep_stride=0, y=None, relu3=True, relu1=True):
    """conv_c3c1 as the engine launches it at a stage exit / in place (dir_conv_c3c1_keep): keep_stride = s > 1 stores only the
    pixels of y on rows and columns that are multiples of s (the rest of y is left untouched: pass a pre-filled y to see it);
    y = res writes the block output over the residual.  Returns (y, t1); t1 is always complete."""
    _need_cuda(t2, w3, bias3, res, w1, bias1)
    B, H, W, P = t2.shape
    P2 = w1.shape[0]
    y = _seam_y(y, res)
    t1 = torch.empty(B, H, W, P2, dtype=t2.dtype, device=t2.device)
    call('dir_conv_c3c1_keep', ptr(t2), ptr(w3), ptr(bias3), ptr(res), ptr(y), ptr(w1), ptr(bias1), ptr(t1), B, H, W, P, P2,
         int(bool(relu3)), int(bool(relu1)), int(keep_stride), _dtype_code(t2), stream_ptr())
    return y, t1


def conv_c3c1_wpair_keep(t2, w3, bias3, res, w1, bias1, keep_stride=0, y=None, relu3=True, relu1=True):
    """... and with paired weights (dir_conv_c3c1_wpair_keep; operands as conv_c3c1_wpair)."""
    (w3h, w3l), (w1h, w1l) = w3, w1
    _need_cuda(t2, w3h, w3l, bias3, res, w1h, bias1)
    B, H, W, P = t2.shape
    P2 = w1h.shape[0]
    y = _seam_y(y, res)
    t1 = torch.empty(B, H, W, P2, dtype=t2.dtype, device=t2.device)
    call('dir_conv_c3c1_wpair_keep', ptr(t2), ptr(w3h), ptr(w3l), ptr(bias3), ptr(res), ptr(y), ptr(w1h),
         ptr(w1l) if w1l is not None else None, ptr(bias1), ptr(t1), B, H, W, P2, int(bool(relu3)), int(bool(relu1)),
         int(keep_stride), stream_ptr())
    return y, t1


def conv_c3c1_ds_wpair(t2, x, wcat, bias, w1, bias1, relu3=True, relu1=True):
    """... and its downsample form (dir_conv_c3c1_ds_wpair): x = (hi, lo) [B,H,W,64] the paired block input,
    wcat = (hi, lo) [256, 128] = [w3 | wds], w1 = (hi, lo) [64, 256] -> (y [B,H,W,256], t1 [B,H,W,64])."""
    (xh, xl), (wh, wl), (w1h, w1l) = x, wcat, w1
    _need_cuda(t2, xh, xl, wh, wl, bias, w1h, w1l, bias1)
    B, H, W, P = t2.shape
    y = torch.empty(B, H, W, 256, dtype=t2.dtype, device=t2.device)
    t1 = torch.empty(B, H, W, 64, dtype=t2.dtype, device=t2.device)
    call('dir_conv_c3c1_ds_wpair', ptr(t2), ptr(xh), ptr(xl), ptr(wh), ptr(wl), ptr(bias), ptr(y), ptr(w1h), ptr(w1l),
         ptr(bias1), ptr(t1), B, H, W, int(bool(relu3)), int(bool(relu1)), stream_ptr())
    return y, t1


def conv_dual(t2, x, wcat, bias, stride2=2, relu=True):
    """conv3 + downsample as one two-source GEMM (dir_conv_dual): t2 [B,OH,OW,Cin], x [B,H2,W2,Cin2],
    wcat [Cout, Cin + Cin2], bias fp32 [Cout] -> y [B,OH,OW,Cout]."""
    _need_cuda(t2, x, wcat, bias)
    B, OH, OW, Cin = t2.shape
    _, H2, W2, Cin2 = x.shape
    Cout = wcat.shape[0]
    y = torch.empty(B, OH, OW, Cout, dtype=t2.dtype, device=t2.device)
    call('dir_conv_dual', ptr(t2), ptr(x), ptr(wcat), ptr(bias), ptr(y), B, OH, OW, Cin, Cout, Cin2, H2, W2,
         int(stride2), int(bool(relu)), _dtype_code(t2), stream_ptr())
    return y


def prep_input(img, dtype=torch.bfloat16, mean=None, std=None):
    """fp32 NCHW (normalised) or uint8 NHWC image batch -> space-to-depth NHWC16 stem input."""
    _need_cuda(img)
    if img.dtype == torch.float32:
        B, C, H, W = img.shape
        fmt = _lib.DIR_IMG_F32_NCHW
    elif img.dtype == torch.uint8:
        B, H, W, C = img.shape
        fmt = _lib.DIR_IMG_U8_NHWC
    else:
        raise TypeError('image must be float32 NCHW or uint8 NHWC')
    if C != 3:
        raise ValueError('3-channel image expected')
    out = torch.empty(B, (H + 1) // 2, (W + 1) // 2, 16, dtype=dtype, device=img.device)
    m = (ctypes.c_float * 3)(*(mean or (0, 0, 0)))
    s = (ctypes.c_float * 3)(*(std or (1, 1, 1)))
    call('dir_prep_input', ptr(img), fmt, m, s, ptr(out), B, H, W,
         DIR_BF16 if dtype == torch.bfloat16 else DIR_FP16, stream_ptr())
    return out


def maxpool_3x3s2(x):
    _need_cuda(x)
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=x.dtype, device=x.device)
    call('dir_maxpool_3x3s2', ptr(x), ptr(y), B, H, W, C, _dtype_code(x), stream_ptr())
    return y


def global_pool(x, pooling='gem', p=3.0, eps=1e-6, center_bias=0.0):
    _need_cuda(x)
    B, H, W, C = x.shape
    out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    call('dir_global_pool', ptr(x), ptr(out), B, H, W, C, POOLING[pooling], float(p), float(eps),
         float(center_bias), _dtype_code(x), stream_ptr())
    return out


def resize_bilinear_u8(img, size):
    """PIL `img.resize((ow, oh), Image.BILINEAR)` of uint8 images on the GPU, bit-identical to Pillow.
    img: [H,W,3] or [B,H,W,3] uint8; size = (ow, oh) like PIL.  The `Scale` transform of
    dirtorch/utils/transforms.py:133-185 without the CPU."""
    _need_cuda(img)
    if img.dtype != torch.uint8 or img.shape[-1] != 3 or img.dim() not in (3, 4):
        raise TypeError('uint8 [H,W,3] or [B,H,W,3] image expected')
    x = img.contiguous().view((-1,) + tuple(img.shape[-3:]))
    B, H, W, _ = x.shape
    ow, oh = int(size[0]), int(size[1])
    need = ctypes.c_size_t()
    call('dir_resize_workspace_bytes', B, H, W, oh, ow, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
    out = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=x.device)
    call('dir_resize_bilinear_u8', ptr(x), ptr(out), B, H, W, oh, ow, ptr(ws), ws.numel(), stream_ptr())
    return out if img.dim() == 4 else out[0]


def upsample_add(x, low):
    """x + nearest-upsampled low: NHWC 16-bit [B,H,W,C] and [B,h,w,C] (rmac_resnet_fpn.py:55-60)."""
    _need_cuda(x, low)
    if x.dtype != low.dtype or x.shape[0] != low.shape[0] or x.shape[3] != low.shape[3]:
        raise ValueError('upsample_add: x and low must share dtype, batch and channels')
    x, low = x.contiguous(), low.contiguous()
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    call('dir_upsample_add', ptr(x), ptr(low), ptr(y), B, H, W, low.shape[1], low.shape[2], C,
         _dtype_code(x), stream_ptr())
    return y


def _need_f32(*ts):
    _need_cuda(*ts)
    for t in ts:
        if t.dtype != torch.float32:
            raise TypeError('fp32 tensors expected')


def prep_input_f32(img, mean=None, std=None):
    """prep_input of the strict path (dir_prep_input_f32, conv_f32.hip): the same feeds -> fp32 [B,ceil(H/2),ceil(W/2),16]."""
    _need_cuda(img)
    if img.dtype == torch.float32:
        B, C, H, W = img.shape
        fmt = _lib.DIR_IMG_F32_NCHW
    elif img.dtype == torch.uint8:
        B, H, W, C = img.shape
        fmt = _lib.DIR_IMG_U8_NHWC
    else:
        raise TypeError('image must be float32 NCHW or uint8 NHWC')
    if C != 3:
        raise ValueError('3-channel image expected')
    out = torch.empty(B, (H + 1) // 2, (W + 1) // 2, 16, dtype=torch.float32, device=img.device)
    m = (ctypes.c_float * 3)(*(mean or (0, 0, 0)))
    s = (ctypes.c_float * 3)(*(std or (1, 1, 1)))
    call('dir_prep_input_f32', ptr(img), fmt, m, s, ptr(out), B, H, W, stream_ptr())
    return out


def maxpool_3x3s2_f32(x):
    """maxpool_3x3s2 on fp32 NHWC, C % 4 == 0 (dir_maxpool_3x3s2_f32)."""
    _need_f32(x)
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
    call('dir_maxpool_3x3s2_f32', ptr(x), ptr(y), B, H, W, C, stream_ptr())
    return y


def global_pool_f32(x, pooling='gem', p=3.0, eps=1e-6, center_bias=0.0):
    """global_pool on fp32 NHWC, C % 64 == 0 (dir_global_pool_f32)."""
    _need_f32(x)
    B, H, W, C = x.shape
    out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    call('dir_global_pool_f32', ptr(x), ptr(out), B, H, W, C, POOLING[pooling], float(p), float(eps),
         float(center_bias), stream_ptr())
    return out


def upsample_add_f32(x, low):
    """upsample_add on fp32 NHWC, C % 4 == 0 (dir_upsample_add_f32)."""
    if x.shape[0] != low.shape[0] or x.shape[3] != low.shape[3]:
        raise ValueError('upsample_add: x and low must share batch and channels')
    x, low = x.contiguous(), low.contiguous()
    _need_f32(x, low)
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    call('dir_upsample_add_f32', ptr(x), ptr(low), ptr(y), B, H, W, low.shape[1], low.shape[2], C, stream_ptr())
    return y


def l2norm_rows_(x, eps=1e-12):
    """In place: x[i] /= max(||x[i]||, eps)."""
    _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError('2-D float32 tensor expected')
    call('dir_l2norm_rows', ptr(x), x.shape[0], x.shape[1], float(eps), stream_ptr())
    return x


def gemm_nt(P, Q, qsub=None, bias=None, alpha=None):
    """out[j][i] = alpha[i] * sum_k P[i][k] * (Q[j][k] - qsub[k]) + bias[i]; fp32, exact MFMA."""
    _need_cuda(P, Q, qsub, bias, alpha)
    for t in (P, Q, qsub, bias, alpha):
        if t is not None and t.dtype != torch.float32:
            raise TypeError('float32 tensors expected')
    NP, K = P.shape
    NQ, K2 = Q.shape
    if K != K2:
        raise ValueError('inner dimensions differ')
    out = torch.empty(NQ, NP, dtype=torch.float32, device=P.device)
    if NP == 0 or NQ == 0:
        return out
    call('dir_gemm_nt_f32', ptr(P), K, ptr(Q), K, ptr(out), NP, NP, NQ, K, ptr(qsub), ptr(bias),
         ptr(alpha), stream_ptr())
    return out


def cov_chain_rows():
    """R of dir_cov_accumulate: the rows one fp32 chain runs over before it is folded into fp64 (host-only query)."""
    return int(_lib.load().dir_cov_chain_rows())


def cov_accumulate(X, shift, gram, sums):
    """gram += (X - shift)^T (X - shift), sums += column sums of X - shift (dir_cov_accumulate, csrc/cov_f32.hip): the
    N-dependent half of a PCA fit.  X [N,D] fp32 CUDA with unit column stride and any row pitch >= D (a column slice of
    a wider tensor is taken as it is), shift [D] fp32, gram [D,D] and sums [D] fp64 contiguous accumulators, updated
    in place and returned."""
    for t in (X, shift, gram, sums):
        if not t.is_cuda:
            raise ValueError('device tensor expected')
    if X.dtype != torch.float32 or shift.dtype != torch.float32 or X.dim() != 2:
        raise TypeError('X [N,D] and shift [D] must be float32')
    if gram.dtype != torch.float64 or sums.dtype != torch.float64:
        raise TypeError('gram and sums must be float64')
    N, D = X.shape
    if X.is_contiguous() or X.stride(1) != 1 or X.stride(0) < D:
        X, ldx = X.contiguous(), D
    else:
        ldx = X.stride(0)
    if tuple(shift.shape) != (D,) or tuple(gram.shape) != (D, D) or tuple(sums.shape) != (D,):
        raise ValueError('shift [D], gram [D,D], sums [D] expected for X [N,D]')
    if not (shift.is_contiguous() and gram.is_contiguous() and sums.is_contiguous()):
        raise ValueError('contiguous shift, gram and sums expected')
    call('dir_cov_accumulate', ptr(X), int(ldx), N, D, ptr(shift), ptr(gram), ptr(sums), stream_ptr())
    return gram, sums


def similarity(queries, database, unit_range=False):
    """scores [Q, N] = queries . database^T, fp32 (dir_similarity).  Databases of >= 32768 rows with a width that
    is a multiple of 32 run as a three-plane bf16 split on the matrix cores (products to 2^-23, fp32
    accumulation; csrc/sim_split.hip), everything else - and everything under DIRTORCH_AMD_SIM_EXACT=1 - as
    the k-ordered fp32 MFMA chain of gemm_nt.
    unit_range=True (dir_similarity_unit): the caller guarantees |values| < 64 (L2-normalised descriptors) - two fp16
    planes and half the matrix work on the large-database path; a larger value gives NON-FINITE scores, not wrong ones."""
    _need_cuda(queries, database)
    for t in (queries, database):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise TypeError('contiguous 2-D float32 tensors expected')
    Q, D = queries.shape
    N, D2 = database.shape
    if D != D2:
        raise ValueError('inner dimensions differ')
    out = torch.empty(Q, N, dtype=torch.float32, device=database.device)
    if Q == 0 or N == 0:
        return out
    call('dir_similarity_unit' if unit_range else 'dir_similarity', ptr(queries), Q, ptr(database), N, D, ptr(out), stream_ptr())
    return out


def multiscale_pool(xs, pooling='mean', gemp=3.0):
    """xs: [S,N,D] fp32 -> [N,D] (mean or signed-power mean); no final L2."""
    _need_cuda(xs)
    S, N, D = xs.shape
    mode = {'mean': 0, 'gem': 1}[pooling]
    out = torch.empty(N, D, dtype=torch.float32, device=xs.device)
    call('dir_multiscale_pool', ptr(xs), ptr(out), S, N, D, mode, float(gemp), stream_ptr())
    return out


def rank_counts(scores, probe_idx):
    """scores [Q,N] fp32 (CUDA), probe_idx [Q,P] int32 (-1 = unused) -> (counts [Q,P] int32,
    probe_scores [Q,P] fp32): how many items rank before each probe (np.argsort(...)[::-1] order)."""
    _need_cuda(scores, probe_idx)
    if scores.dtype != torch.float32 or probe_idx.dtype != torch.int32:
        raise TypeError('float32 scores and int32 probe indices expected')
    Q, N = scores.shape
    P = probe_idx.shape[1]
    counts = torch.empty(Q, P, dtype=torch.int32, device=scores.device)    # zeroed by the call
    pscores = torch.zeros(Q, P, dtype=torch.float32, device=scores.device)
    call('dir_rank_counts', ptr(scores), N, Q, N, ptr(probe_idx), P, ptr(counts), ptr(pscores), stream_ptr())
    return counts, pscores


def revisitop_ap(probe_idx, counts, pscores, pos_off, pos_list, junk_off, junk_list, modes):
    """APs of every (query, mode) from the outputs of rank_counts (dir_revisitop_ap): returns a CUDA
    float64 tensor [Q, modes], -1 where a mode has no positive.  pos_* / junk_* are CSR lists of
    positions into the rows of probe_idx (int32 CUDA tensors)."""
    _need_cuda(probe_idx, counts, pscores, pos_off, pos_list, junk_off, junk_list)
    Q, P = probe_idx.shape
    ap = torch.empty(Q, modes, dtype=torch.float64, device=probe_idx.device)
    terms = torch.empty(max(int(pos_list.numel()), 1), dtype=torch.float64, device=probe_idx.device)
    call('dir_revisitop_ap', ptr(probe_idx), Q, P, ptr(counts), ptr(pscores), ptr(pos_off), ptr(pos_list),
         ptr(junk_off), ptr(junk_list), int(modes), ptr(terms), ptr(ap), stream_ptr())
    return ap


def label_rank(scores, labels, class_off, class_members, qclass, qself):
    """Class-labelled ranking of a block of score rows (dir_label_rank, csrc/label_rank.hip) -> (ap [Q] float64,
    best_rank [Q] int32), both CUDA.  scores [Q,N] fp32 with unit column stride and any row pitch >= N; labels [N],
    class_off [C+1], class_members [N], qclass [Q], qself [Q] int32 CUDA (ranking.build_label_tables).  ap = sklearn's
    average_precision_score over every image but qself (-1 without a positive, NaN for a row with a non-finite kept
    score), best_rank = position of the best same-class image under np.argsort(-scores, kind='stable') (N when the
    class has no image).  Tables that do not fit together raise DirError; the call synchronises the stream once."""
    tables = (labels, class_off, class_members, qclass, qself)
    for t in (scores,) + tables:
        if not t.is_cuda:
            raise ValueError('device tensor expected')
    if scores.dtype != torch.float32 or scores.dim() != 2 or any(t.dtype != torch.int32 for t in tables):
        raise TypeError('float32 scores [Q,N] and int32 tables expected')
    if any(t.dim() != 1 or not t.is_contiguous() for t in tables):
        raise ValueError('contiguous 1-D tables expected')
    Q, N = scores.shape
    if Q > 1 and (scores.stride(1) != 1 or scores.stride(0) < N) or (Q <= 1 and not scores.is_contiguous()):
        scores = scores.contiguous()
    lds = int(scores.stride(0)) if Q > 1 else N
    C = int(class_off.numel()) - 1
    if C < 0 or labels.numel() != N or class_members.numel() != N or qclass.numel() != Q or qself.numel() != Q:
        raise ValueError('labels [N], class_off [C+1], class_members [N], qclass [Q], qself [Q] expected for scores [Q,N]')
    ap = torch.empty(Q, dtype=torch.float64, device=scores.device)
    best = torch.empty(Q, dtype=torch.int32, device=scores.device)
    if Q:
        call('dir_label_rank', ptr(scores), lds, Q, N, ptr(labels), ptr(class_off), ptr(class_members), C, ptr(qclass),
             ptr(qself), ptr(ap), ptr(best), stream_ptr())
    return ap, best


@functools.lru_cache(maxsize=None)     # a constant of the library: asked once, not in every call of a search
def topk_max_k():
    """The largest k ops.topk takes (dir_topk_max_k; host-only)."""
    return int(_lib.load().dir_topk_max_k())


def topk(scores, k, exclude=None, ids=None):
    """Ranked neighbour lists of a block of score rows (dir_topk, csrc/topk.hip) -> (idx [Q,k] int32, vals [Q,k] float32),
    both CUDA: the k best items of every row, best first - score descending, larger id first among equal scores (-0 == +0),
    NaN after every number; on a NaN-free row np.argsort(row, kind='stable')[::-1][:k].  scores [Q,N] fp32 with unit column
    stride and any row pitch >= N; 1 <= k <= min(N, topk_max_k()).  ids [Q,N] int32 (same layout rules; None = the column
    is the id): the id of every column, distinct within a row, -1 = an empty column - the form that merges lists.
    exclude [Q] int32: the id left out of each row (-1 = none).  A row with fewer than k kept items ends in (-1, NaN)
    slots; vals carries the stored bits of the picked scores.  The workspace is allocated here."""
    tables = tuple(t for t in (exclude, ids) if t is not None)
    for t in (scores,) + tables:
        if not t.is_cuda:
            raise ValueError('device tensor expected')
    if scores.dtype != torch.float32 or scores.dim() != 2 or any(t.dtype != torch.int32 for t in tables):
        raise TypeError('float32 scores [Q,N] and int32 tables expected')
    Q, N = scores.shape
    k = int(k)
    if k < 1 or k > min(N, topk_max_k()):
        raise ValueError('1 <= k <= min(N, %d) expected, got k = %d for N = %d' % (topk_max_k(), k, N))
    if ids is not None and tuple(ids.shape) != (Q, N):
        raise ValueError('ids [Q,N] expected for scores [Q,N]')
    if exclude is not None and (exclude.dim() != 1 or exclude.numel() != Q or not exclude.is_contiguous()):
        raise ValueError('contiguous exclude [Q] expected for scores [Q,N]')
    if Q > 1 and (scores.stride(1) != 1 or scores.stride(0) < N) or (Q <= 1 and not scores.is_contiguous()):
        scores = scores.contiguous()
    lds = int(scores.stride(0)) if Q > 1 else N
    if ids is not None:
        # the library reads ids at the pitch of scores
        if Q > 1 and (ids.stride(1) != 1 or ids.stride(0) != lds) or (Q <= 1 and not ids.is_contiguous()):
            if lds != N:
                scores, lds = scores.contiguous(), N
            ids = ids.contiguous()
    idx = torch.empty(Q, k, dtype=torch.int32, device=scores.device)
    vals = torch.empty(Q, k, dtype=torch.float32, device=scores.device)
    if Q:
        need = ctypes.c_size_t(0)
        call('dir_topk_workspace_bytes', Q, N, k, ctypes.byref(need))
        ws = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=scores.device)
        call('dir_topk', ptr(scores), lds, Q, N, k, ptr(ids), ptr(exclude), ptr(idx), ptr(vals), ptr(ws),
             int(need.value), stream_ptr())
    return idx, vals


# ---- the int8 descriptor index (csrc/index_i8.hip) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)     # a constant of the library: asked once, not in every call of a search
def index_i8_max_dim():
    """The widest row the int8 index takes (dir_index_i8_max_dim; host-only)."""
    return int(_lib.load().dir_index_i8_max_dim())


def _rows_pitch(t, width):
    """t [n, >= width] with unit column stride -> (t, row pitch in elements); copies what the library cannot address."""
    n = t.shape[0]
    if n > 1 and (t.stride(1) != 1 or t.stride(0) < width) or (n <= 1 and not t.is_contiguous()):
        t = t.contiguous()
    return t, (int(t.stride(0)) if n > 1 else int(t.shape[1]))


def _on_device(*ts):
    """every tensor given (None: an optional one left out) is a device tensor; unlike _need_cuda, of any strides"""
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError('device tensor expected')


def _i8_codes(codes, ldc, align=16):
    """one-byte codes [n, >= ldc] -> (codes, row pitch) at a pitch and address that are multiples of `align`; copies what is not"""
    codes, ld = _rows_pitch(codes, ldc)
    if ld % align or codes.data_ptr() % align:
        codes, ld = codes[:, :ldc].contiguous(), ldc
    return codes, ld


def _u8_codes(codes, M):
    """uint8 codes [N, >= M] -> (codes, row pitch) at a 4-byte pitch and address; copies (padding zero) what is not"""
    codes, ldc = _rows_pitch(codes, M)
    if ldc % 4 or codes.data_ptr() % 4:
        padded = torch.zeros(codes.shape[0], (M + 3) // 4 * 4, dtype=torch.uint8, device=codes.device)
        padded[:, :M] = codes[:, :M]
        codes, ldc = padded, int(padded.shape[1])
    return codes, ldc


def _score_out(out, Q, N, device):
    """out= of a score block: float32 [Q, >= N] with unit column stride, or None: a new [Q, N] -> (out, its row pitch)"""
    if out is None:
        return torch.empty(Q, N, dtype=torch.float32, device=device), N
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != Q or out.shape[1] < N or (
            Q > 1 and (out.stride(1) != 1 or out.stride(0) < N)) or (Q <= 1 and not out.is_contiguous()):
        raise ValueError('out: float32 [Q, >= N] with unit column stride expected')
    return out, (int(out.stride(0)) if Q > 1 else int(out.shape[1]))


def _scan_out(out, Q, width, device):
    """out= of a scan by list: (float32 scores, int32 ids), [Q, >= width] with unit column stride and ONE row pitch, or
    None: a new pair [Q, width] -> (scores, ids, their row pitch)"""
    if out is None:
        return (torch.empty(Q, width, dtype=torch.float32, device=device),
                torch.empty(Q, width, dtype=torch.int32, device=device), width)
    scores, out_ids = out
    if scores.dtype != torch.float32 or out_ids.dtype != torch.int32:
        raise TypeError('out: float32 scores and int32 ids expected')
    for t in (scores, out_ids):
        if t.dim() != 2 or t.shape[0] != Q or t.shape[1] < width or (Q > 1 and (t.stride(1) != 1 or t.stride(0) < width)) or (
                Q <= 1 and not t.is_contiguous()):
            raise ValueError('out: [Q, >= width] tensors with unit column stride expected')
    if Q > 1 and scores.stride(0) != out_ids.stride(0) or (Q <= 1 and scores.shape[1] != out_ids.shape[1]):
        raise ValueError('out: scores and ids of one row pitch expected')
    return scores, out_ids, (int(scores.stride(0)) if Q > 1 else int(scores.shape[1]))


def _list_tables(Q, N, ids, list_off, probe, col_off, base=None):
    """The tables of a scan by list: ids [N] and list_off [nlist+1] of a list-major database of N rows; probe, col_off and,
    where there is one, base [Q,nprobe] of Q queries -> nlist"""
    if base is not None and base.dtype != torch.float32:
        raise TypeError('float32 base expected')
    if not ids.dtype == list_off.dtype == probe.dtype == col_off.dtype == torch.int32:
        raise TypeError('int32 ids, list_off, probe and col_off expected')
    if ids.dim() != 1 or ids.numel() != N:
        raise ValueError('ids [N] expected for codes of N rows')
    if list_off.dim() != 1 or list_off.numel() < 2:
        raise ValueError('list_off [nlist+1] expected')
    if probe.dim() != 2 or probe.shape[0] != Q or col_off.shape != probe.shape or (base is not None and base.shape != probe.shape):
        raise ValueError('probe, col_off and base [Q,nprobe] expected')
    return int(list_off.numel()) - 1


def _slot_ends(lens, probe, col_off):
    """[Q,nprobe] int64: col_off + the length of the slot's list (lens [nlist] int64; 0 for an empty slot); its largest
    entry is the reach of the slots, the width a scan by list needs"""
    return col_off.long() + torch.where(probe >= 0, lens[probe.long().clamp(min=0)], lens.new_zeros(()))


def _rows_in(X, max_dim):
    """the head of the row quantisers: fp32 CUDA rows [N, D] of 1 <= D <= max_dim -> (X as the library can address it, its row
    pitch, N, D)"""
    _on_device(X)
    if X.dtype != torch.float32 or X.dim() != 2:
        raise TypeError('float32 rows [N,D] expected')
    N, D = X.shape
    if D < 1 or D > max_dim:
        raise ValueError('1 <= D <= %d expected, got %d' % (max_dim, D))
    X, ldx = _rows_pitch(X, D)
    return X, ldx, N, D


def _scales_out(rows, qscales, Q, bscales, N, out, device):
    """The tail of the flat similarity wrappers ahead of their library call: the shape check of the scales (rows: how its
    message names the two sides), their contiguous form and out= -> (qscales, bscales, out, its row pitch)"""
    if qscales.dim() != 1 or bscales.dim() != 1 or qscales.numel() != Q or bscales.numel() != N:
        raise ValueError('scales [Q] and [N] expected for ' + rows)
    out, lds = _score_out(out, Q, N, device)
    return qscales.contiguous(), bscales.contiguous(), out, lds


def quantize_rows(X):
    """fp32 rows -> (codes int8 [N, ldc], scales fp32 [N]), both CUDA (dir_quantize_rows_i8; include/dir_engine.h gives
    the definition): ldc = D rounded up to a multiple of 64, the padding bytes zero.  X [N,D] fp32 CUDA with unit column
    stride and any row pitch."""
    X, ldx, N, D = _rows_in(X, index_i8_max_dim())
    ldc = (D + 63) // 64 * 64
    codes = torch.empty(N, ldc, dtype=torch.int8, device=X.device)
    scales = torch.empty(N, dtype=torch.float32, device=X.device)
    if N:
        call('dir_quantize_rows_i8', ptr(X), ldx, N, D, ptr(codes), ldc, ptr(scales), stream_ptr())
    return codes, scales


def similarity_i8(qcodes, qscales, bcodes, bscales, D, out=None):
    """scores [Q,N] fp32 CUDA of two coded sets (dir_similarity_i8): ((float)int32 dot * qscales[q]) * bscales[n], one
    defined fp32 number per pair.  qcodes [Q,ldc] / bcodes [N,ldc] int8 and qscales [Q] / bscales [N] fp32 as
    quantize_rows gives them (row slices included), D the width the codes were made from.  out: a [Q, >= N] fp32 CUDA
    tensor with unit column stride to write into (its first N columns are returned)."""
    _on_device(qcodes, qscales, bcodes, bscales, out)
    if qcodes.dtype != torch.int8 or bcodes.dtype != torch.int8 or qcodes.dim() != 2 or bcodes.dim() != 2:
        raise TypeError('int8 codes [rows, ldc] expected')
    if qscales.dtype != torch.float32 or bscales.dtype != torch.float32:
        raise TypeError('float32 scales expected')
    D = int(D)
    Q, N = qcodes.shape[0], bcodes.shape[0]
    ldc = (D + 63) // 64 * 64
    if D < 1 or D > index_i8_max_dim() or qcodes.shape[1] < ldc or bcodes.shape[1] < ldc:
        raise ValueError('codes of a width of at least D rounded up to 64 expected, 1 <= D <= %d' % index_i8_max_dim())
    qcodes, ldq = _rows_pitch(qcodes, ldc)
    bcodes, ldb = _i8_codes(bcodes, ldc)
    qscales, bscales, out, lds = _scales_out('codes of Q and N rows', qscales, Q, bscales, N, out, bcodes.device)
    if Q and N:
        call('dir_similarity_i8', ptr(qcodes), ldq, ptr(qscales), Q, ptr(bcodes), ldb, ptr(bscales), N, D, ptr(out), lds,
             stream_ptr())
    return out[:, :N]


# ---- the fp4 descriptor index (csrc/index_fp4.hip) ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_fp4_max_dim():
    """The widest row the fp4 index takes (dir_index_fp4_max_dim; host-only)."""
    return int(_lib.load().dir_index_fp4_max_dim())


def fp4_widths(D):
    """(bytes of codes, block bytes) of a row as quantize_rows_fp4 stores it: D rounded up to 64, halved; 8 * ceil(D / 256)"""
    return (D + 63) // 64 * 32, (D + 255) // 256 * 8


def quantize_rows_fp4(X):
    """fp32 rows -> (codes uint8 [N, ldc], exps uint8 [N, lde], scales fp32 [N]), all CUDA (dir_quantize_rows_fp4;
    include/dir_engine.h gives the definition): e2m1 codes two to a byte, one e8m0 byte per block of 32, one power of two
    per row; (ldc, lde) = fp4_widths(D), the padding written.  X [N,D] fp32 CUDA with unit column stride and any row pitch."""
    X, ldx, N, D = _rows_in(X, index_fp4_max_dim())
    ldc, lde = fp4_widths(D)
    codes = torch.empty(N, ldc, dtype=torch.uint8, device=X.device)
    exps = torch.empty(N, lde, dtype=torch.uint8, device=X.device)
    scales = torch.empty(N, dtype=torch.float32, device=X.device)
    if N:
        call('dir_quantize_rows_fp4', ptr(X), ldx, N, D, ptr(codes), ldc, ptr(exps), lde, ptr(scales), stream_ptr())
    return codes, exps, scales


def similarity_fp4(qcodes, qexps, qscales, bcodes, bexps, bscales, D, out=None):
    """scores [Q,N] fp32 CUDA of two fp4-coded sets (dir_similarity_fp4): (acc * qscales[q]) * bscales[n] with acc the exact
    sum of the products of the dequantised values - one defined fp32 number per pair.  codes / exps uint8 and scales fp32
    as quantize_rows_fp4 gives them (row slices included), D the width they were made from.  out: a [Q, >= N] fp32 CUDA
    tensor with unit column stride to write into (its first N columns are returned)."""
    _on_device(qcodes, qexps, qscales, bcodes, bexps, bscales, out)
    for t in (qcodes, qexps, bcodes, bexps):
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise TypeError('uint8 codes [rows, ldc] and block bytes [rows, lde] expected')
    if qscales.dtype != torch.float32 or bscales.dtype != torch.float32:
        raise TypeError('float32 scales expected')
    D = int(D)
    Q, N = qcodes.shape[0], bcodes.shape[0]
    if D < 1 or D > index_fp4_max_dim():
        raise ValueError('1 <= D <= %d expected, got %d' % (index_fp4_max_dim(), D))
    ldc, lde = fp4_widths(D)
    if qcodes.shape[1] < ldc or bcodes.shape[1] < ldc or qexps.shape[1] < lde or bexps.shape[1] < lde:
        raise ValueError('codes of %d and block bytes of %d columns at least expected for D = %d' % (ldc, lde, D))
    if qexps.shape[0] != Q or bexps.shape[0] != N:
        raise ValueError('block bytes of Q and N rows expected for codes of Q and N rows')
    qcodes, ldq = _rows_pitch(qcodes, ldc)
    qexps, ldqe = _rows_pitch(qexps, lde)
    bcodes, ldb = _i8_codes(bcodes, ldc)
    bexps, ldbe = _i8_codes(bexps, lde, align=8)
    qscales, bscales, out, lds = _scales_out('codes of Q and N rows', qscales, Q, bscales, N, out, bcodes.device)
    if Q and N:
        call('dir_similarity_fp4', ptr(qcodes), ldq, ptr(qexps), ldqe, ptr(qscales), Q, ptr(bcodes), ldb, ptr(bexps), ldbe,
             ptr(bscales), N, D, ptr(out), lds, stream_ptr())
    return out[:, :N]


# ---- the binary descriptor index (csrc/index_bin.hip) -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_bin_max_dim():
    """The widest row the binary index takes (dir_index_bin_max_dim; host-only)."""
    return int(_lib.load().dir_index_bin_max_dim())


def bin_width(D):
    """bytes of a row of bits as quantize_rows_bin stores it: D rounded up to 128, divided by 8 (a multiple of 16)"""
    return (D + 127) // 128 * 16


def quantize_rows_bin(X):
    """fp32 rows -> (bits uint8 [N, ldb], scales fp32 [N]), both CUDA (dir_quantize_rows_bin; include/dir_engine.h gives
    the definition): bit k & 7 of byte k >> 3 is set where x_k has a clear sign bit, scale = sumsq / sumabs; ldb =
    bin_width(D), the padding bits zero.  X [N,D] fp32 CUDA with unit column stride and any row pitch."""
    X, ldx, N, D = _rows_in(X, index_bin_max_dim())
    ldb = bin_width(D)
    bits = torch.empty(N, ldb, dtype=torch.uint8, device=X.device)
    scales = torch.empty(N, dtype=torch.float32, device=X.device)
    if N:
        call('dir_quantize_rows_bin', ptr(X), ldx, N, D, ptr(bits), ldb, ptr(scales), stream_ptr())
    return bits, scales


def similarity_bin(qcodes, qscales, bits, bscales, D, out=None):
    """scores [Q,N] fp32 CUDA of int8-coded queries against sign-bit rows (dir_similarity_bin): ((float)t * qscales[q]) *
    bscales[n] with t the exact int32 sum of +-qcodes[q][k] - one defined fp32 number per pair.  qcodes [Q,ldc] int8 and
    qscales [Q] fp32 as quantize_rows gives them, bits [N,ldb] uint8 and bscales [N] fp32 as quantize_rows_bin gives them
    (row slices included), D the width they were made from.  out: a [Q, >= N] fp32 CUDA tensor with unit column stride to
    write into (its first N columns are returned)."""
    _on_device(qcodes, qscales, bits, bscales, out)
    if qcodes.dtype != torch.int8 or qcodes.dim() != 2:
        raise TypeError('int8 query codes [Q, ldc] expected')
    if bits.dtype != torch.uint8 or bits.dim() != 2:
        raise TypeError('uint8 bits [N, ldb] expected')
    if qscales.dtype != torch.float32 or bscales.dtype != torch.float32:
        raise TypeError('float32 scales expected')
    D = int(D)
    Q, N = qcodes.shape[0], bits.shape[0]
    if D < 1 or D > index_bin_max_dim():
        raise ValueError('1 <= D <= %d expected, got %d' % (index_bin_max_dim(), D))
    ldb = bin_width(D)
    if qcodes.shape[1] < D or bits.shape[1] < ldb:
        raise ValueError('query codes of %d and bits of %d columns at least expected for D = %d' % (D, ldb, D))
    qcodes, ldq = _rows_pitch(qcodes, D)
    bits, ldb = _i8_codes(bits, ldb)
    qscales, bscales, out, lds = _scales_out('codes of Q and bits of N rows', qscales, Q, bscales, N, out, bits.device)
    if Q and N:
        call('dir_similarity_bin', ptr(qcodes), ldq, ptr(qscales), Q, ptr(bits), ldb, ptr(bscales), N, D, ptr(out), lds,
             stream_ptr())
    return out[:, :N]


def gather_scores(queries, database, cand):
    """scores [Q,R] fp32 CUDA, scores[q][r] = <queries[q], database[cand[q][r]]> (dir_gather_scores): the re-score of a
    shortlist.  queries [Q,D], database [N,D] fp32 CUDA, cand [Q,R] int32 CUDA with entries in [-1, N) - the caller's
    duty, as ids in ops.topk; -1 gives NaN.  Unit column strides, any row pitch."""
    _on_device(queries, database, cand)
    if queries.dtype != torch.float32 or database.dtype != torch.float32 or cand.dtype != torch.int32:
        raise TypeError('float32 queries / database and int32 cand expected')
    if queries.dim() != 2 or database.dim() != 2 or cand.dim() != 2:
        raise ValueError('queries [Q,D], database [N,D], cand [Q,R] expected')
    Q, D = queries.shape
    N, D2 = database.shape
    R = cand.shape[1]
    if D != D2 or D < 1 or cand.shape[0] != Q:
        raise ValueError('queries [Q,D], database [N,D], cand [Q,R] expected')
    queries, ldq = _rows_pitch(queries, D)
    database, ldb = _rows_pitch(database, D)
    cand, ldcand = _rows_pitch(cand, R) if R else (cand, 0)
    scores = torch.empty(Q, R, dtype=torch.float32, device=queries.device)
    if Q and R:
        if N == 0:
            scores.fill_(float('nan'))
        else:
            call('dir_gather_scores', ptr(queries), ldq, Q, ptr(database), ldb, N, D, ptr(cand), ldcand, R, ptr(scores), R,
                 stream_ptr())
    return scores


# ---- the inverted-file int8 index (csrc/ivf.hip) -----------------------------------------------------------------------
def segment_sums(X, order, seg_off):
    """sums [S,D] fp32 CUDA, sums[s] = the rows X[order[seg_off[s] : seg_off[s+1]]] added up in fp32 in a fixed order
    (dir_segment_sums): bitwise reproducible, an empty segment gives zeros.  X [N,D] fp32 CUDA with unit column stride
    and any row pitch; order int32 CUDA with entries in [0, N); seg_off [S+1] int32 CUDA, ascending from 0 to at most
    len(order) - the caller's duty, as ids in ops.topk."""
    _on_device(X, order, seg_off)
    if X.dtype != torch.float32 or X.dim() != 2 or order.dtype != torch.int32 or seg_off.dtype != torch.int32:
        raise TypeError('float32 rows [N,D] and int32 order / seg_off expected')
    if order.dim() != 1 or seg_off.dim() != 1 or seg_off.numel() < 1:
        raise ValueError('order [n] and seg_off [S+1] expected')
    N, D = X.shape
    S = int(seg_off.numel()) - 1
    if D < 1:
        raise ValueError('D >= 1 expected')
    X, ldx = _rows_pitch(X, D)
    order, seg_off = order.contiguous(), seg_off.contiguous()
    sums = torch.empty(S, D, dtype=torch.float32, device=X.device)
    if S:
        call('dir_segment_sums', ptr(X), ldx, N, D, ptr(order), ptr(seg_off), S, ptr(sums), D, stream_ptr())
    return sums


def ivf_probe_tables(list_off, probe, col_off):
    """The probe table of a scan by list - what dir_ivf_scan_i8 walks (include/dir_engine.h) - built with integer torch
    operations on the device: (pair_off [nlist+1], pair_q [pairs], pair_col [pairs], item_off [nlist+1], items, reach),
    int32 CUDA tensors and two host integers: the workgroups of the scan and the largest col_off + list length.  Reading
    those two back is the ONE host synchronisation of a scan."""
    nlist, nprobe = int(list_off.numel()) - 1, int(probe.shape[1])
    # pairs (query, slot) in a stable order of their lists, empty slots last (key nlist)
    flat = probe.reshape(-1).long()
    key, order = torch.sort(torch.where(flat < 0, torch.full_like(flat, nlist), flat), stable=True)
    pair_off = torch.searchsorted(key, torch.arange(nlist + 1, device=probe.device)).to(torch.int32)
    pair_q = (order // max(nprobe, 1)).to(torch.int32)
    pair_col = col_off.reshape(-1)[order].contiguous()
    lens = (list_off[1:] - list_off[:-1]).long()
    pairs = (pair_off[1:] - pair_off[:-1]).long()
    per_list = ((lens + 255) // 256) * ((pairs + 31) // 32)
    item_off = torch.cat([per_list.new_zeros(1), torch.cumsum(per_list, 0)])
    ends = _slot_ends(lens, probe, col_off)
    reach = ends.max().reshape(1) if ends.numel() else item_off[:1]
    items, reach = torch.cat([item_off[-1:], reach]).tolist()             # the one synchronisation
    if items > 0x7fffffff:
        raise ValueError('more than 2^31 - 1 workgroups in one scan: cut the queries')
    return pair_off, pair_q, pair_col, item_off.to(torch.int32), int(items), int(reach)


@functools.lru_cache(maxsize=None)     # a constant of the library: asked once, not in every chunk of a search
def ivf_plan_max_pairs():
    """The most (query, slot) pairs one ivf_plan call takes (dir_ivf_plan_max_pairs; host-only)."""
    return int(_lib.load().dir_ivf_plan_max_pairs())


@functools.lru_cache(maxsize=None)
def ivf_scan_max_items():
    """The largest grid a scan by list takes: items * 768 threads within dir_launch_max_threads() (host-only)."""
    return int(_lib.load().dir_launch_max_threads()) // 768


def ivf_plan(list_off, probe, items_bound):
    """ivf_probe_tables' tables from ONE kernel launch and without a synchronisation (dir_ivf_plan, csrc/ivf_plan.hip;
    include/dir_engine.h gives the definition) -> (col_off [Q,nprobe] int32, tables, counts [2] int32), all CUDA.
    list_off [nlist+1] int32 CUDA, nlist <= 65535; probe [Q,nprobe] int32 CUDA, a list outside [0, nlist) = an empty slot,
    Q * nprobe <= ivf_plan_max_pairs().  col_off: the lists of a query side by side in probe order.  tables = (pair_off,
    pair_q, pair_col, item_off, items_bound, None): what ivf_scan, ivf_scan_fp4 and ivf_scan_bin take as tables= TOGETHER
    WITH an explicit width= (the reach is not known on the host) - the four tensors equal ivf_probe_tables' bit for bit.
    items_bound: the grid of the scan, any host integer that is at least item_off[nlist] (the scans' surplus workgroups
    return at once) and at most ivf_scan_max_items() - the caller's duty, as the tables of ivf_scan are.  counts =
    (item_off[nlist], reach) stays on the device: for tests and measurements."""
    _on_device(list_off, probe)
    if list_off.dtype != torch.int32 or probe.dtype != torch.int32:
        raise TypeError('int32 list_off and probe expected')
    if list_off.dim() != 1 or list_off.numel() < 2:
        raise ValueError('list_off [nlist+1] expected')
    if probe.dim() != 2:
        raise ValueError('probe [Q,nprobe] expected')
    nlist, (Q, nprobe) = int(list_off.numel()) - 1, probe.shape
    P = Q * nprobe
    items_bound = int(items_bound)
    if nlist > 65535:
        raise ValueError('nlist <= 65535 expected, got %d' % nlist)
    if P > ivf_plan_max_pairs():
        raise ValueError('Q * nprobe <= %d expected, got %d: cut the queries' % (ivf_plan_max_pairs(), P))
    if items_bound < 0 or items_bound > ivf_scan_max_items():
        raise ValueError('0 <= items_bound <= %d expected, got %d: cut the queries' % (ivf_scan_max_items(), items_bound))
    list_off, probe = list_off.contiguous(), probe.contiguous()
    # one allocation: col_off, pair_q, pair_col [P], pair_off, item_off [nlist + 1], counts [2]
    col_off, pair_q, pair_col, pair_off, item_off, counts = torch.empty(
        3 * P + 2 * (nlist + 1) + 2, dtype=torch.int32, device=probe.device).split([P, P, P, nlist + 1, nlist + 1, 2])
    if Q:
        call('dir_ivf_plan', ptr(probe), Q, nprobe, ptr(list_off), nlist, ptr(col_off), ptr(pair_off), ptr(pair_q),
             ptr(pair_col), ptr(item_off), ptr(counts), stream_ptr())
    else:
        pair_off.zero_(), item_off.zero_(), counts.zero_()
    return col_off.view(Q, nprobe), (pair_off, pair_q, pair_col, item_off, items_bound, None), counts


def _ivf_scan(entry, front, Q, N, D, nlist, ids, list_off, probe, col_off, width, out, tables):
    """What the three scans by list do after their own dtype and shape checks.  front: the entry's arguments up to the
    database scales, as the library takes them (pointers of tensors the caller holds); the rest is the same for every entry:
    ids, N, D, list_off, nlist, the inverted probe table (tables, or ivf_probe_tables' for this list_off, probe and col_off),
    the outputs and the width."""
    ids, list_off = ids.contiguous(), list_off.contiguous()
    pair_off, pair_q, pair_col, item_off, items, reach = tables if tables is not None else ivf_probe_tables(list_off, probe, col_off)
    if width is None and reach is None:
        raise ValueError('tables of ivf_plan need an explicit width: their reach stays on the device')
    width = reach if width is None else int(width)
    scores, out_ids, lds = _scan_out(out, Q, width, ids.device)
    if Q and width:
        call(entry, *front, ptr(ids), N, D, ptr(list_off), nlist, ptr(pair_off), ptr(pair_q), ptr(pair_col), ptr(item_off), items,
             ptr(scores), ptr(out_ids), lds, width, stream_ptr())
    return scores[:, :width], out_ids[:, :width]


def ivf_scan(qcodes, qscales, codes, scales, ids, list_off, probe, col_off, D, width=None, out=None, tables=None):
    """The quantised scores of every query against the rows of the lists it probes (dir_ivf_scan_i8) -> (scores [Q,width]
    fp32, out_ids [Q,width] int32), both CUDA.  qcodes [Q,ldc] / qscales [Q] as quantize_rows gives them (zero padding
    included); codes [N,ldc] int8, scales [N] fp32, ids [N] int32, list_off [nlist+1] int32: a list-major database
    (index.IVFInt8Index); probe [Q,nprobe] int32: the lists of every query, -1 = an empty slot; col_off [Q,nprobe] int32:
    the first output column of every slot.  For r < len(list probe[q][p]), column col_off[q][p] + r carries the score
    ((float)int32 dot * qscales[q]) * scales[n] and the id of row n = list_off[probe[q][p]] + r; a column no slot covers
    carries id -1.  The tables are the caller's duty, as ids in ops.topk: lists in [-1, nlist), slots of a query that do
    not overlap and end at or below width.  width None: the largest col_off + list length of the call.
    out: (scores, out_ids) [Q, >= width] with unit column stride and ONE row pitch to write into; columns at or past
    width keep what they hold.
    The inverted probe table the kernel walks (pairs grouped by list, workgroups per list) comes from ivf_probe_tables,
    which synchronises with the host ONCE, to learn the grid and the width; tables: its result for these list_off, probe
    and col_off, when the caller has it already (the call then does not synchronise), or ivf_plan's tables for this
    list_off and probe with its col_off and an explicit width (no synchronisation anywhere)."""
    _on_device(qcodes, qscales, codes, scales, ids, list_off, probe, col_off, *(out or ()))
    if qcodes.dtype != torch.int8 or codes.dtype != torch.int8 or qcodes.dim() != 2 or codes.dim() != 2:
        raise TypeError('int8 codes [rows, ldc] expected')
    if qscales.dtype != torch.float32 or scales.dtype != torch.float32:
        raise TypeError('float32 scales expected')
    Q, N = qcodes.shape[0], codes.shape[0]
    nlist = _list_tables(Q, N, ids, list_off, probe, col_off)
    D = int(D)
    ldc = (D + 63) // 64 * 64
    if D < 1 or D > index_i8_max_dim() or qcodes.shape[1] < ldc or codes.shape[1] < ldc:
        raise ValueError('codes of a width of at least D rounded up to 64 expected, 1 <= D <= %d' % index_i8_max_dim())
    if qscales.dim() != 1 or scales.dim() != 1 or qscales.numel() != Q or scales.numel() != N:
        raise ValueError('qscales [Q] and scales [N] expected for codes of Q and N rows')
    qcodes, ldq = _i8_codes(qcodes, ldc)
    codes, ldb = _i8_codes(codes, ldc)
    qscales, scales = qscales.contiguous(), scales.contiguous()
    return _ivf_scan('dir_ivf_scan_i8', (ptr(qcodes), ldq, ptr(qscales), Q, ptr(codes), ldb, ptr(scales)), Q, N, D, nlist, ids,
                     list_off, probe, col_off, width, out, tables)


# ---- the inverted file over fp4 codes (csrc/ivf_fp4.hip) ----------------------------------------------------------------
def ivf_scan_fp4(qcodes, qexps, qscales, codes, exps, scales, ids, list_off, probe, col_off, D, width=None, out=None,
                 tables=None):
    """ivf_scan over fp4 rows (dir_ivf_scan_fp4) -> (scores [Q,width] fp32, out_ids [Q,width] int32), both CUDA.  qcodes
    [Q,ldc] / qexps [Q,lde] / qscales [Q] as quantize_rows_fp4 gives them (zero padding included; row slices too); codes
    [N,ldc] uint8, exps [N,lde] uint8, scales [N] fp32, ids [N] int32, list_off [nlist+1] int32: a list-major database
    (index.IVFFp4Index); (ldc, lde) = fp4_widths(D).  probe, col_off, width, out and tables under ivf_scan's contract: for
    r < len(list probe[q][p]), column col_off[q][p] + r carries similarity_fp4's score (acc * qscales[q]) * scales[n] and
    the id of row n = list_off[probe[q][p]] + r; a column no slot covers carries id -1; columns at or past width keep
    what they hold.  tables: ivf_probe_tables' result for these list_off, probe and col_off (the call then does not
    synchronise with the host), or ivf_plan's tables for this list_off and probe with its col_off and an explicit width."""
    _on_device(qcodes, qexps, qscales, codes, exps, scales, ids, list_off, probe, col_off, *(out or ()))
    for t in (qcodes, qexps, codes, exps):
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise TypeError('uint8 codes [rows, ldc] and block bytes [rows, lde] expected')
    if qscales.dtype != torch.float32 or scales.dtype != torch.float32:
        raise TypeError('float32 scales expected')
    Q, N = qcodes.shape[0], codes.shape[0]
    nlist = _list_tables(Q, N, ids, list_off, probe, col_off)
    D = int(D)
    if D < 1 or D > index_fp4_max_dim():
        raise ValueError('1 <= D <= %d expected, got %d' % (index_fp4_max_dim(), D))
    ldc, lde = fp4_widths(D)
    if qcodes.shape[1] < ldc or codes.shape[1] < ldc or qexps.shape[1] < lde or exps.shape[1] < lde:
        raise ValueError('codes of %d and block bytes of %d columns at least expected for D = %d' % (ldc, lde, D))
    if qexps.shape[0] != Q or exps.shape[0] != N:
        raise ValueError('block bytes of Q and N rows expected for codes of Q and N rows')
    if qscales.dim() != 1 or scales.dim() != 1 or qscales.numel() != Q or scales.numel() != N:
        raise ValueError('qscales [Q] and scales [N] expected for codes of Q and N rows')
    qcodes, ldq = _i8_codes(qcodes, ldc)
    qexps, ldqe = _i8_codes(qexps, lde, align=8)
    codes, ldb = _i8_codes(codes, ldc)
    exps, ldbe = _i8_codes(exps, lde, align=8)
    qscales, scales = qscales.contiguous(), scales.contiguous()
    return _ivf_scan('dir_ivf_scan_fp4', (ptr(qcodes), ldq, ptr(qexps), ldqe, ptr(qscales), Q, ptr(codes), ldb, ptr(exps), ldbe,
                                          ptr(scales)), Q, N, D, nlist, ids, list_off, probe, col_off, width, out, tables)


# ---- the inverted file over sign-bit rows (csrc/ivf_bin.hip) ------------------------------------------------------------
def code_sums(qcodes, D):
    """qsums [Q] int32 CUDA, qsums[q] = the sum of qcodes[q][:D] (dir_code_sums): what ivf_scan_bin subtracts from twice its
    sum over the set bits.  qcodes [Q, >= D] int8 CUDA with unit column stride and any row pitch."""
    _on_device(qcodes)
    if qcodes.dtype != torch.int8 or qcodes.dim() != 2:
        raise TypeError('int8 query codes [Q, ldc] expected')
    D = int(D)
    if D < 1 or D > index_bin_max_dim() or qcodes.shape[1] < D:
        raise ValueError('codes of at least D columns expected, 1 <= D <= %d' % index_bin_max_dim())
    Q = qcodes.shape[0]
    qcodes, ldq = _rows_pitch(qcodes, D)
    qsums = torch.empty(Q, dtype=torch.int32, device=qcodes.device)
    if Q:
        call('dir_code_sums', ptr(qcodes), ldq, Q, D, ptr(qsums), stream_ptr())
    return qsums


def ivf_scan_bin(qcodes, qscales, bits, bscales, ids, list_off, probe, col_off, D, width=None, out=None, tables=None,
                 qsums=None):
    """ivf_scan over sign-bit rows (dir_ivf_scan_bin) -> (scores [Q,width] fp32, out_ids [Q,width] int32), both CUDA.  qcodes
    [Q,ldc] int8 / qscales [Q] as quantize_rows gives them (ldc >= D rounded up to 64, zero in D .. that; row slices too);
    bits [N,ldb] uint8, ldb >= bin_width(D), and bscales [N] fp32 as quantize_rows_bin gives them, ids [N] int32, list_off
    [nlist+1] int32: a list-major database (index.IVFBinaryIndex).  probe, col_off, width, out and tables under ivf_scan's
    contract: for r < len(list probe[q][p]), column col_off[q][p] + r carries similarity_bin's score ((float)t * qscales[q])
    * bscales[n] and the id of row n = list_off[probe[q][p]] + r; a column no slot covers carries id -1; columns at or past
    width keep what they hold.  qsums: code_sums(qcodes, D) when the caller has it already."""
    _on_device(qcodes, qscales, bits, bscales, ids, list_off, probe, col_off, qsums, *(out or ()))
    if qcodes.dtype != torch.int8 or qcodes.dim() != 2:
        raise TypeError('int8 query codes [Q, ldc] expected')
    if bits.dtype != torch.uint8 or bits.dim() != 2:
        raise TypeError('uint8 bits [N, ldb] expected')
    if qscales.dtype != torch.float32 or bscales.dtype != torch.float32:
        raise TypeError('float32 scales expected')
    if qsums is not None and qsums.dtype != torch.int32:
        raise TypeError('int32 qsums expected')
    Q, N = qcodes.shape[0], bits.shape[0]
    nlist = _list_tables(Q, N, ids, list_off, probe, col_off)
    D = int(D)
    if D < 1 or D > index_bin_max_dim():
        raise ValueError('1 <= D <= %d expected, got %d' % (index_bin_max_dim(), D))
    ldc, ldb = (D + 63) // 64 * 64, bin_width(D)
    if qcodes.shape[1] < ldc or bits.shape[1] < ldb:
        raise ValueError('query codes of %d and bits of %d columns at least expected for D = %d' % (ldc, ldb, D))
    if qscales.dim() != 1 or bscales.dim() != 1 or qscales.numel() != Q or bscales.numel() != N:
        raise ValueError('qscales [Q] and bscales [N] expected for codes of Q and bits of N rows')
    if qsums is not None and (qsums.dim() != 1 or qsums.numel() != Q):
        raise ValueError('qsums [Q] expected for codes of Q rows')
    qcodes, ldq = _i8_codes(qcodes, ldc)
    bits, ldb = _i8_codes(bits, ldb)
    qsums = code_sums(qcodes, D) if qsums is None else qsums.contiguous()
    qscales, bscales = qscales.contiguous(), bscales.contiguous()
    return _ivf_scan('dir_ivf_scan_bin', (ptr(qcodes), ldq, ptr(qscales), ptr(qsums), Q, ptr(bits), ldb, ptr(bscales)), Q, N, D,
                     nlist, ids, list_off, probe, col_off, width, out, tables)


# ---- the product-quantised index (csrc/pq.hip) -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)     # a constant of the library: asked once, not in every call of a search
def pq_max_m():
    """The largest number of sub-spaces a product quantiser takes (dir_pq_max_m; host-only)."""
    return int(_lib.load().dir_pq_max_m())


def _pq_codebooks(codebooks, D):
    """codebooks [M, 256, dsub] fp32 CUDA for rows of D = M * dsub values, D within the index's bound -> (codebooks,
    contiguous, M)"""
    _on_device(codebooks)
    if codebooks.dtype != torch.float32 or codebooks.dim() != 3 or codebooks.shape[1] != 256 or codebooks.shape[2] < 1:
        raise TypeError('float32 codebooks [M, 256, dsub] expected')
    M = int(codebooks.shape[0])
    if M < 1 or M > pq_max_m():
        raise ValueError('1 <= M <= %d expected, got %d' % (pq_max_m(), M))
    if int(D) != M * int(codebooks.shape[2]):
        raise ValueError('rows of M * dsub = %d values expected, got %d' % (M * int(codebooks.shape[2]), D))
    if D > index_i8_max_dim():
        raise ValueError('D <= %d expected, got %d' % (index_i8_max_dim(), D))
    return codebooks.contiguous(), M


def pq_encode(X, codebooks):
    """fp32 rows -> codes uint8 [N, ldc] CUDA (dir_pq_encode; include/dir_engine.h gives the definition): byte m of a row
    is its nearest of the 256 centroids of sub-space m, ldc = M rounded up to a multiple of 4, the padding bytes zero.
    X [N,D] fp32 CUDA with unit column stride and any row pitch; codebooks [M, 256, D / M] fp32 CUDA."""
    _on_device(X)
    if X.dtype != torch.float32 or X.dim() != 2:
        raise TypeError('float32 rows [N,D] expected')
    N, D = X.shape
    codebooks, M = _pq_codebooks(codebooks, D)
    X, ldx = _rows_pitch(X, D)
    ldc = (M + 3) // 4 * 4
    codes = torch.empty(N, ldc, dtype=torch.uint8, device=X.device)
    if N:
        call('dir_pq_encode', ptr(X), ldx, N, D, M, ptr(codebooks), ptr(codes), ldc, stream_ptr())
    return codes


def pq_lut(queries, codebooks):
    """The tables of every query, lut [Q, M, 256] fp32 CUDA (dir_pq_lut): lut[q][m][j] = <sub-vector m of query q,
    centroid j of sub-space m>, accumulated in fp32 in column order.  queries [Q,D] fp32 CUDA with unit column stride."""
    _on_device(queries)
    if queries.dtype != torch.float32 or queries.dim() != 2:
        raise TypeError('float32 queries [Q,D] expected')
    Q, D = queries.shape
    codebooks, M = _pq_codebooks(codebooks, D)
    queries, ldq = _rows_pitch(queries, D)
    lut = torch.empty(Q, M, 256, dtype=torch.float32, device=queries.device)
    if Q:
        call('dir_pq_lut', ptr(queries), ldq, Q, D, M, ptr(codebooks), ptr(lut), stream_ptr())
    return lut


def pq_scan(lut, codes, out=None):
    """scores [Q,N] fp32 CUDA (dir_pq_scan): scores[q][n] = the entries lut[q][m][codes[n][m]] added up in fp32 in the
    order m = 0 .. M - 1, one defined number per pair.  lut [Q, M, 256] fp32 CUDA as pq_lut gives it; codes [N, >= M]
    uint8 CUDA as pq_encode gives them (row slices included).  out: a [Q, >= N] fp32 CUDA tensor with unit column stride
    to write into (its first N columns are returned; the others keep what they hold)."""
    _on_device(lut, codes, out)
    if lut.dtype != torch.float32 or lut.dim() != 3 or lut.shape[2] != 256:
        raise TypeError('float32 lut [Q, M, 256] expected')
    if codes.dtype != torch.uint8 or codes.dim() != 2:
        raise TypeError('uint8 codes [N, ldc] expected')
    Q, M = int(lut.shape[0]), int(lut.shape[1])
    N = int(codes.shape[0])
    if M < 1 or M > pq_max_m() or codes.shape[1] < M:
        raise ValueError('codes of at least M bytes a row expected, 1 <= M <= %d' % pq_max_m())
    lut = lut.contiguous()
    codes, ldc = _u8_codes(codes, M)
    out, lds = _score_out(out, Q, N, codes.device)
    if Q and N:
        call('dir_pq_scan', ptr(lut), Q, M, ptr(codes), ldc, N, ptr(out), lds, stream_ptr())
    return out[:, :N]


# ---- the IVF-PQ index (csrc/ivfpq.hip) ----------------------------------------------------------------------------------
def ivfpq_scan_cols():
    """The output columns a workgroup of the IVF-PQ scan owns (dir_ivfpq_scan_cols; host-only)."""
    return int(_lib.load().dir_ivfpq_scan_cols())


def ivfpq_base(queries, centroids, probe, M):
    """The coarse term of every probed list, base [Q,nprobe] fp32 CUDA (dir_ivfpq_base): base[q][p] = <q, centroids[probe
    [q][p]]> as M partial sums - the chain over the D / M columns of sub-space m, in column order - added in the order
    m = 0 .. M - 1 (include/dir_engine.h); NaN for a slot of -1.  queries [Q,D] and centroids [nlist,D] fp32 CUDA with unit
    column stride and any row pitch; probe [Q,nprobe] int32 CUDA with entries in [-1, nlist)."""
    _on_device(queries, centroids, probe)
    if queries.dtype != torch.float32 or centroids.dtype != torch.float32 or queries.dim() != 2 or centroids.dim() != 2:
        raise TypeError('float32 queries [Q,D] and centroids [nlist,D] expected')
    if probe.dtype != torch.int32:
        raise TypeError('int32 probe expected')
    Q, D = queries.shape
    M = int(M)
    if centroids.shape[1] != D or D < 1 or D > index_i8_max_dim():
        raise ValueError('queries and centroids of one width D expected, 1 <= D <= %d' % index_i8_max_dim())
    if M < 1 or M > pq_max_m() or D % M:
        raise ValueError('1 <= M <= %d dividing D = %d expected, got %d' % (pq_max_m(), D, M))
    if probe.dim() != 2 or probe.shape[0] != Q:
        raise ValueError('probe [Q,nprobe] expected')
    nlist, nprobe = int(centroids.shape[0]), int(probe.shape[1])
    queries, ldq = _rows_pitch(queries, D)
    centroids, ldc = _rows_pitch(centroids, D)
    probe = probe.contiguous()
    base = torch.empty(Q, nprobe, dtype=torch.float32, device=queries.device)
    if Q and nprobe:
        call('dir_ivfpq_base', ptr(queries), ldq, Q, ptr(centroids), ldc, nlist, D, M, ptr(probe), nprobe, ptr(base),
             stream_ptr())
    return base


def ivfpq_scan(lut, base, codes, ids, list_off, probe, col_off, width=None, out=None):
    """The scores of every query against the rows of the lists it probes (dir_ivfpq_scan) -> (scores [Q,width] fp32,
    out_ids [Q,width] int32), both CUDA.  lut [Q, M, 256] fp32 as pq_lut gives it; base [Q,nprobe] fp32 as ivfpq_base gives
    it; codes [N, >= M] uint8, ids [N] int32, list_off [nlist+1] int32: a list-major database (index.IVFPQIndex); probe
    [Q,nprobe] int32: the lists of every query, -1 = an empty slot; col_off [Q,nprobe] int32: the first output column of
    every slot.  For r < len(list probe[q][p]), column col_off[q][p] + r carries (((base[q][p] + lut[q][0][code[n][0]]) +
    lut[q][1][code[n][1]]) + ...) and the id of row n = list_off[probe[q][p]] + r; a column no slot covers carries id -1.
    The tables are the caller's duty, as ids in ops.topk: lists in [-1, nlist), slots of a query that do not overlap; a
    slot stores nothing at or past width.  width None: the largest col_off + list length of the call, which is read back
    from the device (the one host synchronisation; a caller that knows its width passes it and has none).
    out: (scores, out_ids) [Q, >= width] with unit column stride and ONE row pitch to write into; columns at or past
    width keep what they hold."""
    _on_device(lut, base, codes, ids, list_off, probe, col_off, *(out or ()))
    if lut.dtype != torch.float32 or lut.dim() != 3 or lut.shape[2] != 256:
        raise TypeError('float32 lut [Q, M, 256] expected')
    if codes.dtype != torch.uint8 or codes.dim() != 2:
        raise TypeError('uint8 codes [N, ldc] expected')
    Q, M = int(lut.shape[0]), int(lut.shape[1])
    N = int(codes.shape[0])
    nlist = _list_tables(Q, N, ids, list_off, probe, col_off, base)
    if M < 1 or M > pq_max_m() or codes.shape[1] < M:
        raise ValueError('codes of at least M bytes a row expected, 1 <= M <= %d' % pq_max_m())
    nprobe = int(probe.shape[1])
    lut = lut.contiguous()
    codes, ldc = _u8_codes(codes, M)
    base, ids, list_off, probe, col_off = (t.contiguous() for t in (base, ids, list_off, probe, col_off))
    if width is None:
        ends = _slot_ends((list_off[1:] - list_off[:-1]).long(), probe, col_off)
        width = int(ends.max()) if ends.numel() else 0
    width = max(int(width), 0)
    scores, out_ids, lds = _scan_out(out, Q, width, codes.device)
    if Q and width:
        call('dir_ivfpq_scan', ptr(lut), ptr(base), Q, M, ptr(codes), ldc, ptr(ids), N, ptr(list_off), nlist, ptr(probe),
             ptr(col_off), nprobe, ptr(scores), ptr(out_ids), lds, width, stream_ptr())
    return scores[:, :width], out_ids[:, :width]


def expand_descriptors(descs, db=None, alpha=0.0, k=0, scratch_bytes=256 << 20):
    """alpha-QE / DBA on the device (dir_expand_descriptors): descs [n,D], db [m,D] fp32 CUDA (db None =
    expand the set against itself, a row never being its own neighbour) -> [n,D] fp32 CUDA."""
    _need_cuda(descs, db)
    self_set = db is None
    pool_ = descs if self_set else db
    n, D = descs.shape
    m = pool_.shape[0]
    out = torch.empty_like(descs)
    if n == 0:
        return out
    rows = max(1, min(n, scratch_bytes // max(4 * m, 1)))
    sim = torch.empty(rows * m, dtype=torch.float32, device=descs.device)
    call('dir_expand_descriptors', ptr(descs), n, ptr(pool_), m, D, int(k), float(alpha), int(self_set),
         ptr(out), ptr(sim), sim.numel() * 4, stream_ptr())
    return out


def expand_lists(descs, db, idx, vals, alpha):
    """alpha-QE / DBA from neighbour lists (dir_expand_lists, csrc/expand_lists.hip; include/dir_engine.h gives the
    definition, tests/expand_ref.py restates it) -> [n,D] fp32 CUDA:
    out[i] = normalize((descs[i] + sum_t vals[i][t]^alpha * db[idx[i][t]]) / (k + 1)), the picks added in list order.
    descs [n,D], db [m,D] fp32 CUDA (db may BE descs: the self-set); idx / vals [n,k] int32 / fp32 CUDA as ops.topk or an
    index's search gives them - entries in [-1, m) are the caller's duty, a -1 slot adds nothing and its vals entry is
    not read.  Unit column strides, any row pitch; k = 0 normalises descs.  alpha >= 0."""
    _on_device(descs, db, idx, vals)
    if descs.dtype != torch.float32 or db.dtype != torch.float32 or idx.dtype != torch.int32 or vals.dtype != torch.float32:
        raise TypeError('float32 descs / db / vals and int32 idx expected')
    if descs.dim() != 2 or db.dim() != 2 or idx.dim() != 2 or vals.dim() != 2:
        raise ValueError('descs [n,D], db [m,D], idx and vals [n,k] expected')
    n, D = descs.shape
    m, D2 = db.shape
    k = idx.shape[1]
    if D != D2 or idx.shape[0] != n or tuple(vals.shape) != (n, k):
        raise ValueError('descs [n,D], db [m,D], idx and vals [n,k] expected')
    descs, ldd = _rows_pitch(descs, D)
    db, ldb = _rows_pitch(db, D)
    idx, ldi = _rows_pitch(idx, k) if k else (idx, 0)
    vals, ldv = _rows_pitch(vals, k) if k else (vals, 0)
    if ldi != ldv:      # (one pitch for both tables in the C ABI)
        idx, vals, ldi = idx.contiguous(), vals.contiguous(), k
    out = torch.empty(n, D, dtype=torch.float32, device=descs.device)
    call('dir_expand_lists', ptr(descs), ldd, n, ptr(db), ldb, m, D, ptr(idx), ptr(vals), ldi, k, float(alpha), ptr(out), D,
         stream_ptr())
    return out


# ---- diffusion on the kNN graph (csrc/diffusion.hip) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def diffusion_slab_rows():
    """The rows of a slab of the solve's dot products (dir_diffusion_slab_rows; host-only)."""
    return int(_lib.load().dir_diffusion_slab_rows())


def _list_pair(idx, vals, what):
    """(idx, vals, pitch) of a pair of [n,k] int32 / fp32 list tables at one row pitch"""
    _on_device(idx, vals)
    if idx.dtype != torch.int32 or vals.dtype != torch.float32:
        raise TypeError('int32 %s ids and float32 values expected' % what)
    if idx.dim() != 2 or tuple(vals.shape) != tuple(idx.shape):
        raise ValueError('%s ids and values [n,k] expected' % what)
    k = idx.shape[1]
    if k == 0:
        return idx, vals, 0
    idx, ldi = _rows_pitch(idx, k)
    vals, ldv = _rows_pitch(vals, k)
    if ldi != ldv:      # (one pitch for both tables in the C ABI)
        idx, vals, ldi = idx.contiguous(), vals.contiguous(), k
    return idx, vals, ldi


def knn_graph(idx, vals, gamma=3):
    """The mutual kNN graph of a database from its self-set neighbour lists (dir_knn_graph, csrc/diffusion.hip;
    include/dir_engine.h gives the definition, tests/diffusion_ref.py restates it) -> S [N,k] fp32 CUDA in the layout of
    the lists: S[i][t] = min(vals[i][t]^gamma, vals[j][t']^gamma) / sqrt(deg[i] deg[j]) for the mutual neighbours
    j = idx[i][t], +0 for every other slot (a hole, an id out of range, the row itself, a later duplicate, a score <= 0 or
    NaN, a neighbour that does not list the row back).  idx / vals [N,k] int32 / fp32 CUDA as ops.topk or an index's
    search(same_set=True) gives them."""
    idx, vals, ldl = _list_pair(idx, vals, 'list')
    N, k = idx.shape
    S = torch.empty(N, k, dtype=torch.float32, device=idx.device)
    if N and k:
        call('dir_knn_graph', ptr(idx), ptr(vals), ldl, N, k, float(gamma), ptr(S), k, stream_ptr())
    return S


def diffusion_seed(qidx, qvals, N, gamma=3):
    """The seed columns of a query set (dir_diffusion_seed) -> Y [N,Q] fp32 CUDA: zero except Y[qidx[q][t]][q] =
    qvals[q][t]^gamma for the slots with an id in [0, N) and a score > 0; a later slot of a list that names the same row
    overwrites an earlier one.  qidx / qvals [Q,kq]: the kq best database rows of every query."""
    qidx, qvals, ldq = _list_pair(qidx, qvals, 'query list')
    Q, kq = qidx.shape
    N = int(N)
    Y = torch.empty(N, Q, dtype=torch.float32, device=qidx.device)
    if N and Q:
        call('dir_diffusion_seed', ptr(qidx), ptr(qvals), ldq, Q, kq, N, float(gamma), ptr(Y), Q, stream_ptr())
    return Y


def diffusion_solve(idx, S, Y, alpha=0.99, iters=20):
    """(I - alpha S) F = Y by `iters` conjugate-gradient iterations, all Q columns at once (dir_diffusion_solve) ->
    F [N,Q] fp32 CUDA.  idx / S [N,k]: the graph as knn_graph gives it (a slot with S == 0 or an id outside [0, N) is
    skipped); Y [N,Q] fp32 CUDA.  0 <= alpha < 1.  No host synchronisation; the workspace is allocated here.  The result
    of a column does not depend on the other columns of the call."""
    idx, S, ldl = _list_pair(idx, S, 'graph')
    _on_device(Y)
    if Y.dtype != torch.float32 or Y.dim() != 2 or Y.shape[0] != idx.shape[0]:
        raise ValueError('float32 Y [N,Q] expected for a graph of N rows')
    if not 0 <= alpha < 1:
        raise ValueError('0 <= alpha < 1 expected, got %g' % alpha)
    if iters < 0:
        raise ValueError('iters must be non-negative')
    N, k = idx.shape
    Q = Y.shape[1]
    F = torch.empty(N, Q, dtype=torch.float32, device=Y.device)
    if N == 0 or Q == 0:
        return F
    Y, ldy = _rows_pitch(Y, Q)
    need = ctypes.c_size_t(0)
    call('dir_diffusion_workspace_bytes', N, Q, ctypes.byref(need))
    ws = torch.empty(max(int(need.value), 16), dtype=torch.uint8, device=Y.device)
    call('dir_diffusion_solve', ptr(idx), ldl, ptr(S), ldl, N, k, ptr(Y), ldy, Q, float(alpha), int(iters), ptr(F), Q,
         ptr(ws), int(need.value), stream_ptr())
    return F


# ---- truncated diffusion: a query's top-T subgraph solved in one workgroup (csrc/diffusion_local.hip) -------------------
@functools.lru_cache(maxsize=None)
def diffusion_local_max_rows():
    """The largest T of the truncated diffusion (dir_diffusion_local_max_rows; host-only): topk_max_k()."""
    return int(_lib.load().dir_diffusion_local_max_rows())


def _local_pitch(t, T, what):
    """a [Q, .., T] table of the local graph with unit stride along T and its rows packed at one pitch -> (t, pitch)"""
    if t.shape[-1] != T:
        raise ValueError('%s: %d local rows expected, got %d' % (what, T, t.shape[-1]))
    if t.numel() == 0:
        return t, T
    rows = t.shape[-2]                                    # (k for lidx / lw, Q for y / cid / f)
    outer = t.shape[0] if t.dim() == 3 else 1
    if rows > 1:
        ld = int(t.stride(-2))
    elif outer > 1:
        ld = int(t.stride(0))                             # one slot a query: the queries are a pitch apart
    else:
        ld = T
    packed = (T == 1 or t.stride(-1) == 1) and ld >= T and (outer <= 1 or t.stride(0) == ld * rows)
    if not packed:
        t, ld = t.contiguous(), T
    return t, ld


def diffusion_subgraph(idx, S, cidx, cvals, kq=10, gamma=3, one_hot=False, ldt=None):
    """The subgraph of every query's candidate list (dir_diffusion_subgraph; include/dir_engine.h gives the definition,
    tests/diffusion_trunc_ref.py restates it) -> (cid [Q,T] int32, lidx [Q,k,T] int32, lw [Q,k,T] fp32, y [Q,T] fp32), all
    CUDA.  idx / S [N,k]: the graph as knn_graph gives it; cidx / cvals [Q,T] int32 / fp32: T candidates a query, best
    first, as ops.topk or an index's search gives them, 1 <= T <= diffusion_local_max_rows().  cid is the id of a live
    candidate (in [0, N), first of its id in the list), -1 of a dead one; lidx / lw are the edges among the live candidates
    in local numbering, slot-major, -1 / +0 elsewhere; y the seeds: cvals^gamma of the live ones among the first kq with a
    score > 0, or with one_hot 1 at candidate 0.  ldt: the pitch of the T axis of the results (>= T; None = T) - they come
    back as views [.., :T] of it, which diffusion_solve_local and diffusion_spread take as they are."""
    idx, S, ldl = _list_pair(idx, S, 'graph')
    cidx, cvals, ldc = _list_pair(cidx, cvals, 'candidate list')
    N, k = idx.shape
    Q, T = cidx.shape
    if not 1 <= T <= diffusion_local_max_rows():
        raise ValueError('1 <= T <= %d candidates expected, got %d' % (diffusion_local_max_rows(), T))
    ldt = T if ldt is None else int(ldt)
    if ldt < T or kq < 0:
        raise ValueError('ldt >= T and kq >= 0 expected')
    dev = cidx.device
    cid = torch.empty(Q, ldt, dtype=torch.int32, device=dev)
    lidx = torch.empty(Q, k, ldt, dtype=torch.int32, device=dev)
    lw = torch.empty(Q, k, ldt, dtype=torch.float32, device=dev)
    y = torch.empty(Q, ldt, dtype=torch.float32, device=dev)
    if Q:
        call('dir_diffusion_subgraph', ptr(idx), ldl, ptr(S), ldl, N, k, ptr(cidx), ptr(cvals), ldc, Q, T, int(kq), float(gamma),
             int(bool(one_hot)), ptr(cid), ptr(lidx), ptr(lw), ptr(y), ldt, stream_ptr())
    return cid[:, :T], lidx[:, :, :T], lw[:, :, :T], y[:, :T]


def diffusion_solve_local(lidx, lw, y, cid=None, alpha=0.99, iters=20):
    """(I - alpha S_q) f = y_q on every query's own subgraph by `iters` conjugate-gradient iterations, one workgroup per
    query and one launch in all (dir_diffusion_solve_local) -> f [Q,T] fp32 CUDA, at the pitch of y.  lidx / lw [Q,k,T],
    y [Q,T] and cid [Q,T] (optional) as diffusion_subgraph gives them; a slot with lidx outside [0, T) or lw == 0 is
    skipped.  f is NaN where cid < 0.  The result of a query is diffusion_solve's on that query's graph with the one
    column y, bit for bit, and does not depend on the other queries of the call."""
    _on_device(lidx, lw, y, cid)
    if lidx.dtype != torch.int32 or lw.dtype != torch.float32 or y.dtype != torch.float32 or (
            cid is not None and cid.dtype != torch.int32):
        raise TypeError('int32 lidx / cid and float32 lw / y expected')
    if lidx.dim() != 3 or tuple(lw.shape) != tuple(lidx.shape) or y.dim() != 2 or y.shape[0] != lidx.shape[0] or (
            cid is not None and tuple(cid.shape) != tuple(y.shape)):
        raise ValueError('lidx / lw [Q,k,T], y [Q,T] and cid [Q,T] expected')
    if not 0 <= alpha < 1:
        raise ValueError('0 <= alpha < 1 expected, got %g' % alpha)
    if iters < 0:
        raise ValueError('iters must be non-negative')
    Q, k, T = lidx.shape
    if not 1 <= T <= diffusion_local_max_rows():
        raise ValueError('1 <= T <= %d local rows expected, got %d' % (diffusion_local_max_rows(), T))
    tabs = [_local_pitch(t, T, 'local table') for t in (lidx, lw, y) + ((cid,) if cid is not None else ())]
    if len({ld for _, ld in tabs}) != 1:      # (one pitch for all tables in the C ABI)
        tabs = [(t.contiguous(), T) for t, _ in tabs]
    ldt = tabs[0][1]
    lidx, lw, y = tabs[0][0], tabs[1][0], tabs[2][0]
    cid = tabs[3][0] if cid is not None else None
    f = torch.empty(Q, ldt, dtype=torch.float32, device=y.device)
    if Q:
        call('dir_diffusion_solve_local', ptr(lidx), ptr(lw), k, ptr(y), ptr(cid) if cid is not None else None, ldt, Q, T,
             float(alpha), int(iters), ptr(f), ldt, stream_ptr())
    return f[:, :T]


def diffusion_spread(scores, cid, f):
    """List scores back into score rows, IN PLACE (dir_diffusion_spread) -> scores.  scores [Q,N] fp32 CUDA (the plain
    similarities; unit column stride); cid [Q,T] int32 and f [Q,T] fp32 as diffusion_subgraph / diffusion_solve_local give
    them.  Every score drops by 4, then a live candidate's column takes max(f, -2) (a NaN f: -2): every candidate outranks
    every non-candidate, and the non-candidates keep their cosine order."""
    _on_device(scores, cid, f)
    if scores.dtype != torch.float32 or f.dtype != torch.float32 or cid.dtype != torch.int32:
        raise TypeError('float32 scores / f and int32 cid expected')
    if scores.dim() != 2 or cid.dim() != 2 or tuple(f.shape) != tuple(cid.shape) or cid.shape[0] != scores.shape[0]:
        raise ValueError('scores [Q,N], cid [Q,T] and f [Q,T] expected')
    Q, N = scores.shape
    T = cid.shape[1]
    if T > diffusion_local_max_rows():
        raise ValueError('T <= %d expected, got %d' % (diffusion_local_max_rows(), T))
    if Q == 0 or N == 0:
        return scores
    if scores.stride(1) != 1 or (Q > 1 and scores.stride(0) < N):
        raise ValueError('scores with unit column stride and a row pitch >= N expected (they are changed in place)')
    lds = int(scores.stride(0)) if Q > 1 else N
    (cid, ldc), (f, ldf) = _local_pitch(cid, T, 'cid'), _local_pitch(f, T, 'f')
    if ldc != ldf:
        cid, f, ldc = cid.contiguous(), f.contiguous(), T
    call('dir_diffusion_spread', ptr(scores), lds, Q, N, ptr(cid), ptr(f), ldc, T, stream_ptr())
    return scores


def stem_pool(s2d, w_packed, bias, out_hw):
    """Fused stem: s2d image [B,H2,W2,16] + packed 4x4x16 filter -> pooled [B,PH,PW,64];
    out_hw = (OH, OW) of the 7x7 s2 convolution."""
    _need_cuda(s2d, w_packed, bias)
    B, H2, W2, _ = s2d.shape
    OH, OW = out_hw
    y = torch.empty(B, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1, 64, dtype=s2d.dtype, device=s2d.device)
    call('dir_stem_pool', ptr(s2d), ptr(w_packed), ptr(bias), ptr(y), B, H2, W2, OH, OW,
         _dtype_code(s2d), stream_ptr())
    return y


# ---- the paired-fp16 head of DIR_FP16P (csrc/conv_pair.hip) ----------------------------------------------------------
def split_pair(t):
    """fp32 tensor -> (hi, lo) fp16 planes with hi = fp16(t), lo = fp16(t - hi): the storage format of the paired
    head (device-side torch casts: test tooling for operands, the kernels produce their own pairs)."""
    hi = t.to(torch.float16)
    return hi, (t - hi.to(torch.float32)).to(torch.float16)


def conv_bn_act_pair(x, w, bias, res=None, stride=1, pad=0, relu=True, pair_out=True):
    """dir_conv_bn_act_pair.  x = (hi, lo) or a single fp16 tensor, NHWC [B,H,W,Cin]; w = (hi, lo) [Cout,R,S,Cin];
    res = None, a single fp16 tensor or (hi, lo).  Returns (y_hi, y_lo), y_lo None when pair_out is False."""
    x_hi, x_lo = x if isinstance(x, (tuple, list)) else (x, None)
    w_hi, w_lo = w
    r_hi, r_lo = (res if isinstance(res, (tuple, list)) else (res, None))
    _need_cuda(x_hi, x_lo, w_hi, w_lo, bias, r_hi, r_lo)
    for t in (x_hi, x_lo, w_hi, w_lo, r_hi, r_lo):
        if t is not None and t.dtype != torch.float16:
            raise TypeError('fp16 planes expected')
    B, H, W, Cin = x_hi.shape
    Cout, R, S, Cin2 = w_hi.shape
    if Cin2 != Cin:
        raise ValueError('Cin mismatch')
    OH = (H + 2 * pad - R) // stride + 1
    OW = (W + 2 * pad - S) // stride + 1
    y_hi = torch.empty(B, OH, OW, Cout, dtype=torch.float16, device=x_hi.device)
    y_lo = torch.empty_like(y_hi) if pair_out else None
    call('dir_conv_bn_act_pair', ptr(x_hi), ptr(x_lo), ptr(w_hi), ptr(w_lo), ptr(bias), ptr(r_hi), ptr(r_lo),
         ptr(y_hi), ptr(y_lo), B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, int(bool(relu)), stream_ptr())
    return y_hi, y_lo


def conv_pair_dual(t2, x, wcat, bias, relu=True, pair_out=True):
    """dir_conv_pair_dual: y = act([w3 | wds] . [t2 ; x] + bias); t2, x = (hi, lo) [B,H,W,Cin], wcat = (hi, lo)
    [Cout, 2 Cin] (or [Cout,1,1,2 Cin]).  Returns (y_hi, y_lo)."""
    (t_hi, t_lo), (x_hi, x_lo), (w_hi, w_lo) = t2, x, wcat
    _need_cuda(t_hi, t_lo, x_hi, x_lo, w_hi, w_lo, bias)
    B, H, W, Cin = t_hi.shape
    Cout = w_hi.shape[0]
    if w_hi.numel() != Cout * 2 * Cin or x_hi.shape != t_hi.shape:
        raise ValueError('shape mismatch')
    y_hi = torch.empty(B, H, W, Cout, dtype=torch.float16, device=t_hi.device)
    y_lo = torch.empty_like(y_hi) if pair_out else None
    call('dir_conv_pair_dual', ptr(t_hi), ptr(t_lo), ptr(x_hi), ptr(x_lo), ptr(w_hi), ptr(w_lo), ptr(bias), ptr(y_hi),
         ptr(y_lo), B, H, W, Cin, Cout, int(bool(relu)), stream_ptr())
    return y_hi, y_lo


def prep_input_pair(img, mean=None, std=None):
    """fp32 NCHW (normalised) or uint8 NHWC image batch -> space-to-depth NHWC16 stem input as an fp16 pair."""
    _need_cuda(img)
    if img.dtype == torch.float32:
        B, C, H, W = img.shape
        fmt = _lib.DIR_IMG_F32_NCHW
    elif img.dtype == torch.uint8:
        B, H, W, C = img.shape
        fmt = _lib.DIR_IMG_U8_NHWC
    else:
        raise TypeError('image must be float32 NCHW or uint8 NHWC')
    if C != 3:
        raise ValueError('3-channel image expected')
    hi = torch.empty(B, (H + 1) // 2, (W + 1) // 2, 16, dtype=torch.float16, device=img.device)
    lo = torch.empty_like(hi)
    m = (ctypes.c_float * 3)(*(mean or (0, 0, 0)))
    s = (ctypes.c_float * 3)(*(std or (1, 1, 1)))
    call('dir_prep_input_pair', ptr(img), fmt, m, s, ptr(hi), ptr(lo), B, H, W, stream_ptr())
    return hi, lo


def stem_pool_pair(s2d, w_packed, bias, out_hw):
    """dir_stem_pool_pair: s2d = (hi, lo) [B,H2,W2,16], w_packed = (hi, lo) [64,4,4,16] (pack_stem_weight of the
    fp32 filter, then split_pair), out_hw = conv output size -> pooled (hi, lo) [B,PH,PW,64]."""
    (s_hi, s_lo), (w_hi, w_lo) = s2d, w_packed
    _need_cuda(s_hi, s_lo, w_hi, w_lo, bias)
    B, H2, W2, _ = s_hi.shape
    OH, OW = out_hw
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    y_hi = torch.empty(B, PH, PW, 64, dtype=torch.float16, device=s_hi.device)
    y_lo = torch.empty_like(y_hi)
    call('dir_stem_pool_pair', ptr(s_hi), ptr(s_lo), ptr(w_hi), ptr(w_lo), ptr(bias), ptr(y_hi), ptr(y_lo), B, H2, W2,
         OH, OW, stream_ptr())
    return y_hi, y_lo


def stem_pool_u8(img_u8, w_oihw, bn_scale, bn_bias, mean, std, seg_tiles=0):
    """dir_stem_pool_u8: raw uint8 NHWC image [B,H,W,3] (device) + conv1.weight [64,3,7,7], the folded bn1 scale / bias (host
    fp32) and the preprocess mean / std -> pooled (hi, lo) [B,PH,PW,64]: ToTensor + Normalize + conv 7x7 s2 + BN + ReLU +
    MaxPool 3x3 s2 with the normalisation folded into the filter pair (transforms.py:617-623, resnet.py:115-119)."""
    _need_cuda(img_u8)
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise TypeError('image must be uint8 NHWC [B,H,W,3]')
    B, H, W, _ = img_u8.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    w = w_oihw.detach().to('cpu', torch.float32).contiguous()
    sc = bn_scale.detach().to('cpu', torch.float32).contiguous()
    bi = bn_bias.detach().to('cpu', torch.float32).contiguous()
    assert tuple(w.shape) == (64, 3, 7, 7) and sc.numel() == 64 and bi.numel() == 64
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    ws = torch.empty(B * ((H + 1) // 2) * ((W + 1) // 2) * 32, dtype=torch.uint8, device=img_u8.device)
    y_hi = torch.empty(B, PH, PW, 64, dtype=torch.float16, device=img_u8.device)
    y_lo = torch.empty_like(y_hi)
    call('dir_stem_pool_u8', ptr(img_u8.contiguous()), ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(sc.data_ptr()),
         ctypes.c_void_p(bi.data_ptr()), m, s, ptr(ws), ptr(y_hi), ptr(y_lo), B, H, W, int(seg_tiles), stream_ptr())
    return y_hi, y_lo


def pca_whiten(X, components, mean=None, alpha=None, l2norm=False, eps_unused=None, unit_range=False):
    """out[n][j] = alpha[j] * <X[n] - mean, components[j]> (+ row L2 normalisation): dir_pca_whiten_l2, the PCA projection of
    common.whiten_features (dirtorch/utils/common.py:221-239).  unit_range=True (dir_pca_whiten_l2_unit): the caller guarantees
    |X - mean| < 64 and |components| < 64; sets of >= 32768 rows with a width that is a multiple of 32 then run as two fp16
    planes per operand on the matrix cores (csrc/sim_split.hip whiten_split_kernel) instead of the exact fp32 MFMA chain."""
    _need_cuda(X, components, mean, alpha)
    for t in (X, components, mean, alpha):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError('contiguous float32 tensors expected')
    N, D = X.shape
    v, D2 = components.shape
    if D != D2:
        raise ValueError('inner dimensions differ')
    out = torch.empty(N, v, dtype=torch.float32, device=X.device)
    if N == 0:
        return out
    call('dir_pca_whiten_l2_unit' if unit_range else 'dir_pca_whiten_l2', ptr(X), N, D, ptr(mean), ptr(components), v, ptr(alpha),
         int(bool(l2norm)), ptr(out), stream_ptr())
    return out
