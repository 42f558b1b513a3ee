"""The engine's fused, paired and stem launches (tests/engine_cases.py) at the tile counts the engine runs them at.

test_engine_launches_are_the_table: ResNet-101 and ResNet-50 on the synthetic checkpoint, one net per (arch, dtype), one profiled
forward per claimed workload and feed on random device inputs; the in-scope launch records (conv_c3c1<..>, conv_igemm<../dual>,
conv_pair<..>, stem_pool*) must be exactly what engine_cases.engine_launches() mirrors, every form emitted must have a row that is
one of its launches, and every row with a workload must be launched there.  (The plain conv_igemm picks are the picker gate's, the
head kernels and prep_input are out of scope.)

test_engine_case_vs_reference: every row through its per-op entry point against a CPU reference of every output element (three
whole images - first, interior, last - of the rows too large for that), plus bitwise checks over the whole tensor: the same entry
point on single images (or uneven pixel slices of one image) - a pixel of a 1x1 GEMM or a stem depends only on its own inputs, in a
fixed K order -, a repeated launch, and the twin form where the engine has one (DIRTORCH_AMD_NO_C3C1LC, DIRTORCH_AMD_NO_WREGD,
DIRTORCH_AMD_STEM_U8_PREP, DIRTORCH_AMD_STEM_PAIR_OLD).  Plain forms run on operands exact in both 16-bit formats against fp32 at
check_close's tolerance; paired forms run twice, with lo planes as large as the hi planes (a dropped, swapped or misplaced plane is
an O(1) error) and with realistic lo planes (ops.split_pair of fp32 values), against fp64 at the paired tests' bounds.  A failure
names the row, the bad-element count, the first bad (pixel m, channel n), its tile and the tile's place in the walk.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from engine_cases import ENGINE_CASES, WORKLOADS, engine_launches, family, launch_geometry, stem_maps, walk_position
from test_ops_gpu import DTYPES, RTOL

pytestmark = pytest.mark.gpu

IN_SCOPE = ('conv_c3c1<', 'conv_pair<', 'stem_pool')
ARCHS = ('resnet101', 'resnet50')


def _in_scope(kernel):
    return kernel.startswith(IN_SCOPE) or (kernel.startswith('conv_igemm<') and kernel.endswith('/dual>'))


def test_engine_launches_are_the_table():
    import dir_oracle as O
    from dirtorch_amd import nets
    rows = {(r[3], r[4], r[1]): r for r in ENGINE_CASES if r[3] != 'synthetic'}
    seen_rows, emitted, problems = set(), {}, []
    for arch in ARCHS:
        sd = O.synth_state_dict(arch, seed=7)
        for dtype in ('bf16', 'fp16', 'fp16p'):
            net = nets.create_model(arch + '_rmac', pretrained='')
            net.load_state_dict(sd)
            net.compute_dtype = dtype
            net.cuda().eval()
            g = torch.Generator(device='cuda').manual_seed(3)
            for wl, a, B, H, W in WORKLOADS:
                if a != arch:
                    continue
                for feed in ('u8', 'f32'):
                    x = (torch.randint(0, 256, (B, H, W, 3), generator=g, device='cuda', dtype=torch.uint8) if feed == 'u8'
                         else torch.randn(B, 3, H, W, generator=g, device='cuda'))
                    net.set_profiling(True)
                    with torch.no_grad():
                        net(x)
                    got = [(r['name'], r['kernel']) for r in net.get_profile() if _in_scope(r['kernel'])]
                    net.set_profiling(False)
                    del x
                    # the sub-form is not in the label: it is the mirror's (engine_launches mirrors the predicates - the role-split
                    # DS seam under the default switches, P2 and conv1's pairing from the next layer, the stem's raw / prep form from
                    # the feed and the width's parity)
                    want = engine_launches(wl, dtype, feed)
                    if sorted(got) != sorted((rec, label) for rec, label, _ in want):
                        problems.append('%s %s %s feed: the engine launched %s, the mirror says %s' % (
                            wl, dtype, feed, sorted(set(got) - {(r, l) for r, l, _ in want}),
                            sorted({(r, l) for r, l, _ in want} - set(got))))
                        continue
                    for rec, label, sub in want:
                        emitted.setdefault((label, sub), set()).add((wl, rec))
                        if (wl, rec, label) in rows and dtype in rows[(wl, rec, label)][6]:
                            seen_rows.add(rows[(wl, rec, label)][0])
            del net
            torch.cuda.empty_cache()
    for form, where in sorted(emitted.items(), key=str):
        if not any((r[1], r[2]) == form and (r[3], r[4]) in where for r in ENGINE_CASES):
            problems.append('%s %s: launched (e.g. %s %s) but no row of tests/engine_cases.py is one of its launches'
                            % (form + sorted(where)[0]))
    for r in ENGINE_CASES:
        if r[3] != 'synthetic' and r[0] not in seen_rows:
            problems.append('%s: the engine does not launch %s at %s %s in %s' % (r[0], r[1], r[3], r[4], r[6]))
    assert not problems, '\n'.join(problems)


# ---- the rows against a reference ------------------------------------------------------------------------------------------------
CASES = []
for _r in ENGINE_CASES:
    for _d in _r[6]:
        if _d == 'fp16p' and family(_r[1]) != 'stem':
            CASES += [(_r, 'fp16p-biglo'), (_r, 'fp16p-real')] if (',wp' in _r[1] or family(_r[1]) == 'pair') else [(_r, 'fp16')]
        elif _r[1] == 'stem_pool_pair':     # (stem_pool_u8 forms its filter pair itself, from fp32 weights: no large-lo run)
            CASES += [(_r, 'fp16p'), (_r, 'fp16p-biglo')]
        else:
            CASES.append((_r, _d))
CASES = list(dict.fromkeys(CASES))      # (a dual row's fp16p launch is the fp16 kernel)

FULL_PIXELS = 1 << 19       # rows with more pixels are checked on three whole images against the CPU


def _exact16(t):
    """Round to bf16 and flush what fp16 could not hold as a normal number: the result is exact in both formats."""
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def _images(B, npix):
    return list(range(B)) if B * npix <= FULL_PIXELS else sorted({0, B // 2, B - 1})


def _fail_report(what, form, shape, m0, got, ref, tol):
    """got / ref [m, n] (m from pixel m0 of the launch); None if every element is within tol, else the message, with the first bad
    element's work unit and its place in the walk (engine_cases.walk_position: each launcher's own unit order)."""
    bad = (got - ref).abs() > tol
    if not bad.any():
        return None
    m, n = (int(v) for v in bad.nonzero()[0])
    units, grid, _ = launch_geometry(form, shape)
    unit, wg, step, kind = walk_position(form, shape, m0 + m, n)
    return ('%s: %d / %d elements out of tolerance (max err %.4g); first bad m = %d, n = %d: got %.6g ref %.6g; %s %d = workgroup %d, '
            'walk step %d (%d units on %d workgroups)'
            % (what, int(bad.sum()), bad.numel(), float((got - ref).abs().max()), m0 + m, n, float(got[m, n]), float(ref[m, n]),
               kind, unit, wg, step, units, grid))


def _close(got, ref, dname):
    return RTOL[dname] * ref.abs() + RTOL[dname] * ref.abs().mean() + 1e-5


def _slices(B, H):
    """Pixel slices that change the walk: uneven blocks of images (the first alone, a third, the rest), or three uneven row
    bands of a single image."""
    if B > 1:
        cuts = sorted({0, 1, 1 + (B - 1) // 3, B})
        return [(b0, b1, 0, H) for b0, b1 in zip(cuts, cuts[1:])]
    h1, h2 = max(1, H // 5), max(2, (3 * H) // 5)
    return [(0, 1, 0, h1), (0, 1, h1, h2), (0, 1, h2, H)]


def _cut(t, sl):
    return t if sl is None else t[sl].contiguous()


def _gen(tag, mode):
    return torch.Generator(device='cuda').manual_seed(zlib.crc32(('%s/%s' % (tag, mode)).encode()))


def _twin(monkeypatch, switch, fn):
    monkeypatch.setenv(switch, '1')
    try:
        return fn()
    finally:
        monkeypatch.delenv(switch)


def _seam_case(row, mode, monkeypatch):
    from dirtorch_amd import ops
    tag, label, sub, wl, rec, shape, _ = row
    B, H, W, P, P2 = shape[:5]
    form, ds, wp = (label, sub), ',ds' in label, ',wp' in label
    g = _gen(tag, 'ops')
    relu = lambda t: torch.relu(t)      # noqa: E731
    rn = lambda *sh, s=1.0: torch.randn(*sh, generator=g, device='cuda') * s      # noqa: E731
    if not wp:
        dt = DTYPES[mode]
        t2 = _exact16(relu(rn(B, H, W, P))).to(dt)
        w3 = _exact16(rn(4 * P, P, s=math.sqrt(2.0 / P))).to(dt)
        b3 = rn(4 * P, s=0.2)
        w1 = _exact16(rn(P2, 4 * P, s=math.sqrt(2.0 / (4 * P)))).to(dt)
        b1 = rn(P2, s=0.2)
        if ds:
            xin = _exact16(relu(rn(B, H, W, 64))).to(dt)
            wcat = torch.cat([w3, _exact16(rn(256, 64, s=math.sqrt(2.0 / 64))).to(dt)], 1).contiguous()
            run = lambda sl=None: ops.conv_c3c1_ds(_cut(t2, sl), _cut(xin, sl), wcat, b3, w1, b1)   # noqa: E731
        else:
            res = _exact16(rn(B, H, W, 4 * P)).to(dt)        # signed residual
            run = lambda sl=None: ops.conv_c3c1(_cut(t2, sl), w3, b3, _cut(res, sl), w1, b1)   # noqa: E731

        def yref(b, c0, c1):      # fp32, as check_close's other references
            t = t2[b].reshape(-1, P)[c0:c1].float().cpu()
            if ds:
                return torch.relu(torch.cat([t, xin[b].reshape(-1, 64)[c0:c1].float().cpu()], 1) @ wcat.float().cpu().t() + b3.cpu())
            return torch.relu(t @ w3.float().cpu().t() + b3.cpu() + res[b].reshape(-1, 4 * P)[c0:c1].float().cpu())
        w1_eff = w1.float().cpu()
        bound = lambda got, ref: _close(got, ref, mode)      # noqa: E731
    else:
        # fp16 pairs; biglo: lo planes as large as the hi planes, real: split_pair of fp32 values
        big = mode == 'fp16p-biglo'
        pairw = lambda *sh, s: ((rn(*sh, s=s).half(), rn(*sh, s=s).half()) if big else ops.split_pair(rn(*sh, s=s)))   # noqa: E731
        t2 = relu(rn(B, H, W, 64)).half()
        w3 = pairw(256, 64, s=0.09)
        b3 = rn(256, s=0.5)
        w1_pair = sub != 'p2_128_w1single'
        w1 = pairw(P2, 256, s=0.04)
        if not w1_pair:
            w1 = (w1[0], None)
        b1 = rn(P2, s=0.5)
        if ds:
            xin = (relu(rn(B, H, W, 64)).half(), (rn(B, H, W, 64, s=0.5) if big else rn(B, H, W, 64, s=2.0 ** -12)).half())
            wd = pairw(256, 64, s=0.09)
            wcat = tuple(torch.cat([a, b], 1).contiguous() for a, b in zip(w3, wd))
            run = lambda sl=None: ops.conv_c3c1_ds_wpair(_cut(t2, sl), (_cut(xin[0], sl), _cut(xin[1], sl)), wcat, b3, w1, b1)   # noqa: E731
        else:
            res = rn(B, H, W, 256).half()
            run = lambda sl=None: ops.conv_c3c1_wpair(_cut(t2, sl), w3, b3, _cut(res, sl), w1, b1)   # noqa: E731
        d = lambda t: t.double().cpu()      # noqa: E731

        def yref(b, c0, c1):
            f = lambda t, C: d(t[b].reshape(-1, C)[c0:c1])      # noqa: E731
            if ds:      # (w_hi + w_lo) . [t2 ; x_hi] + w_ds_hi . x_lo: the lo x lo term is dropped by design
                wf = d(wcat[0]) + d(wcat[1])
                acc = f(t2, 64) @ wf[:, :64].t() + f(xin[0], 64) @ wf[:, 64:].t() + f(xin[1], 64) @ d(wcat[0])[:, 64:].t()
            else:
                acc = f(t2, 64) @ (d(w3[0]) + d(w3[1])).t() + f(res, 256)
            return torch.relu(acc + d(b3))
        w1_eff = d(w1[0]) + (d(w1[1]) if w1[1] is not None else 0)
        bound = lambda got, ref: 1.01 * 2.0 ** -11 * float(ref.abs().max()) + 1e-5 + 0 * ref      # noqa: E731
    y, t1 = run()
    torch.cuda.synchronize()
    what = '%s [%s]' % (tag, mode)
    npix = H * W
    for b in _images(B, npix):
        for c0 in range(0, npix, 1 << 16):
            c1 = min(npix, c0 + (1 << 16))
            ref = yref(b, c0, c1)
            got = y[b].reshape(-1, 4 * P)[c0:c1].to(ref.dtype).cpu()
            msg = _fail_report(what + ' block output y', form, shape, b * npix + c0, got, ref, bound(got, ref))
            assert msg is None, msg
            tref = torch.relu(got @ w1_eff.t() + b1.to(ref.dtype).cpu())          # conv1 of the kernel's own rounded y
            tg = t1[b].reshape(-1, P2)[c0:c1].to(ref.dtype).cpu()
            msg = _fail_report(what + ' conv1 output t1', form, shape, b * npix + c0, tg, tref, bound(tg, tref))
            assert msg is None, msg
    again = run()
    assert torch.equal(again[0], y) and torch.equal(again[1], t1), what + ': a repeated launch differs'
    for b0, b1_, h0, h1 in _slices(B, H):
        sl = (slice(b0, b1_), slice(h0, h1))
        ys, ts = run(sl)
        assert torch.equal(ys, y[sl]) and torch.equal(ts, t1[sl]), \
            '%s: the launch on images %d-%d, rows %d-%d differs from the whole launch in %d elements' % (
                what, b0, b1_ - 1, h0, h1 - 1, int((ys != y[sl]).sum() + (ts != t1[sl]).sum()))
    if sub == 'lc':       # the one-role DS kernel (conv_c3c1.hip) forms the same sums
        one = _twin(monkeypatch, 'DIRTORCH_AMD_NO_C3C1LC', run)
        assert torch.equal(one[0], y) and torch.equal(one[1], t1), what + ': the role-split and one-role DS seams differ'


def d_(t):
    return t.double().cpu()


def _dual_case(row, mode, monkeypatch):
    from dirtorch_amd import ops
    tag, label, sub, wl, rec, shape, _ = row
    B, OH, OW, Cin, Cin2, H2, W2, s2, Cout = shape[:9]
    dt = DTYPES[mode]
    g = _gen(tag, 'ops')
    rn = lambda *sh, s=1.0: torch.randn(*sh, generator=g, device='cuda') * s      # noqa: E731
    t2 = _exact16(torch.relu(rn(B, OH, OW, Cin))).to(dt)
    x = _exact16(torch.relu(rn(B, H2, W2, Cin2))).to(dt)
    wcat = torch.cat([_exact16(rn(Cout, Cin, s=math.sqrt(2.0 / Cin))), _exact16(rn(Cout, Cin2, s=math.sqrt(2.0 / Cin2)))], 1).to(dt).contiguous()
    bias = rn(Cout, s=0.2)

    def run(sl=None):
        if sl is None:
            return ops.conv_dual(t2, x, wcat, bias, stride2=s2, relu=True)
        (b0, b1, h0, h1) = sl
        return ops.conv_dual(t2[b0:b1, h0:h1].contiguous(), x[b0:b1, s2 * h0:s2 * (h1 - 1) + 1].contiguous(), wcat, bias, stride2=s2, relu=True)
    y = run()
    torch.cuda.synchronize()
    what = '%s [%s]' % (tag, mode)
    wd = wcat.float().cpu()
    npix = OH * OW
    for b in _images(B, npix):
        xs = x[b, ::s2, ::s2][:OH, :OW].reshape(-1, Cin2)
        for c0 in range(0, npix, 1 << 15):
            c1 = min(npix, c0 + (1 << 15))
            a = torch.cat([t2[b].reshape(-1, Cin)[c0:c1], xs[c0:c1]], 1).float().cpu()
            ref = torch.relu(a @ wd.t() + bias.cpu())
            got = y[b].reshape(-1, Cout)[c0:c1].float().cpu()
            msg = _fail_report(what, (label, sub), shape, b * npix + c0, got, ref, _close(got, ref, mode))
            assert msg is None, msg
    assert torch.equal(run(), y), what + ': a repeated launch differs'
    for sl in _slices(B, OH):
        b0, b1, h0, h1 = sl
        assert torch.equal(run(sl), y[b0:b1, h0:h1]), '%s: the launch on images %d-%d, rows %d-%d differs' % (what, b0, b1 - 1, h0, h1 - 1)
    if 'wregd' in label:      # the DUAL ring (conv_persist.hip) forms the same sums
        assert torch.equal(_twin(monkeypatch, 'DIRTORCH_AMD_NO_WREGD', run), y), what + ': wregd and the DUAL ring differ'


def _pair_case(row, mode):
    from dirtorch_amd import ops
    tag, label, sub, wl, rec, shape, _ = row
    B, H, W, Cin, Cout, k, stride, use_res, relu = shape
    assert k == 1 and stride == 1
    big = mode == 'fp16p-biglo'
    g = _gen(tag, mode)
    rn = lambda *sh, s=1.0: torch.randn(*sh, generator=g, device='cuda') * s      # noqa: E731
    pair = lambda *sh, s=1.0: ((rn(*sh, s=s).half(), rn(*sh, s=s).half()) if big else ops.split_pair(rn(*sh, s=s)))   # noqa: E731
    xp = (torch.relu(rn(B, H, W, Cin)).half(), None)
    if '_xw' in label:
        xp = (xp[0], (rn(B, H, W, Cin, s=0.5) if big else rn(B, H, W, Cin, s=2.0 ** -12)).half())
    wp = pair(Cout, 1, 1, Cin, s=1.0 / math.sqrt(Cin))
    bias = rn(Cout)
    res = rn(B, H, W, Cout).half() if use_res else None
    x_arg = xp if xp[1] is not None else xp[0]

    def run(sl=None, pair_out=True):
        if sl is None:
            return ops.conv_bn_act_pair(x_arg, wp, bias, res, relu=relu, pair_out=pair_out)
        xs = (x_arg[0][sl].contiguous(), x_arg[1][sl].contiguous()) if xp[1] is not None else x_arg[sl].contiguous()
        return ops.conv_bn_act_pair(xs, wp, bias, None if res is None else res[sl].contiguous(), relu=relu)
    y = run()
    torch.cuda.synchronize()
    what = '%s [%s]' % (tag, mode)
    wh, wl_ = d_(wp[0]).reshape(Cout, Cin), d_(wp[1]).reshape(Cout, Cin)
    npix = H * W
    for b in _images(B, npix):
        for c0 in range(0, npix, 1 << 16):
            c1 = min(npix, c0 + (1 << 16))
            acc = d_(xp[0][b].reshape(-1, Cin)[c0:c1]) @ (wh + wl_).t() + d_(bias)    # x_lo . w_lo is dropped by design
            if xp[1] is not None:
                acc = acc + d_(xp[1][b].reshape(-1, Cin)[c0:c1]) @ wh.t()
            if res is not None:
                acc = acc + d_(res[b].reshape(-1, Cout)[c0:c1])
            ref = torch.relu(acc) if relu else acc
            got = d_(y[0][b].reshape(-1, Cout)[c0:c1]) + d_(y[1][b].reshape(-1, Cout)[c0:c1])
            scale = max(1.0, float(ref.abs().max()))
            msg = _fail_report(what, (label, sub), shape, b * npix + c0, got, ref, 4e-6 * scale + 0 * ref)
            assert msg is None, msg
    again = run()
    assert torch.equal(again[0], y[0]) and torch.equal(again[1], y[1]), what + ': a repeated launch differs'
    single = run(pair_out=False)
    assert single[1] is None and torch.equal(single[0], y[0]), what + ': the single-plane output is not the pair\'s hi plane'
    for b0, b1, h0, h1 in _slices(B, H):
        sl = (slice(b0, b1), slice(h0, h1))
        ys = run(sl)
        assert torch.equal(ys[0], y[0][sl]) and torch.equal(ys[1], y[1][sl]), \
            '%s: the launch on images %d-%d, rows %d-%d differs' % (what, b0, b1 - 1, h0, h1 - 1)


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _stem_ref_f64(x, w, bias):
    """conv 7x7 s2 p3 + bias, ReLU, max-pool 3x3 s2 p1 in fp64 on the CPU -> [B, PH, PW, 64]."""
    return F.max_pool2d(F.relu(F.conv2d(x, w, bias, 2, 3)), 3, 2, 1).permute(0, 2, 3, 1)


def _unpack_s2d(s, H, W):
    """prep_input's space-to-depth NHWC16 plane(s) -> the image [B, 3, H, W] it holds."""
    x = torch.zeros(s.shape[0], 3, 2 * s.shape[1], 2 * s.shape[2], dtype=s.dtype)
    for dy in range(2):
        for dx in range(2):
            x[:, :, dy::2, dx::2] = s[..., (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3].permute(0, 3, 1, 2)
    return x[:, :, :H, :W]


def _unpack_w(p):
    """pack_stem_weight's [64, 4, 4, 16] -> the 7x7 OIHW filter."""
    w = torch.zeros(64, 3, 7, 7, dtype=p.dtype)
    for R in range(4):
        for S in range(4):
            for dy in range(2):
                for dx in range(2):
                    r, s = 2 * R + dy - 1, 2 * S + dx - 1
                    if 0 <= r < 7 and 0 <= s < 7:
                        w[:, :, r, s] = p[:, R, S, (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3]
    return w


def _stem_case(row, mode, monkeypatch):
    from dirtorch_amd import ops
    from test_stem_u8_gpu import reference_stem
    tag, label, sub, wl, rec, shape, _ = row
    B, H, W = shape
    form = (label, sub)
    _, _, PH, PW = stem_maps(H, W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = _gen(tag, 'ops')
    gc = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    w = torch.randn(64, 3, 7, 7, generator=gc) / 147 ** 0.5
    what = '%s [%s]' % (tag, mode)
    if label == 'stem_pool_u8':
        scale, bias = 0.5 + torch.rand(64, generator=gc), 0.3 * torch.randn(64, generator=gc)
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, device='cuda', dtype=torch.uint8)
        run = lambda b0=0, b1=B: ops.stem_pool_u8(img[b0:b1], w, scale, bias, MEAN, STD)     # noqa: E731
        ref_of = lambda b: reference_stem(img[b:b + 1].cpu(), w, scale, bias)[0]             # noqa: E731
        tol = lambda ref: 2e-6 * max(1.0, float(ref.abs().max()))                            # noqa: E731
        joined = lambda y, b: y[0][b].double().cpu() + y[1][b].double().cpu()                # noqa: E731
    elif label == 'stem_pool_pair':
        bias = (0.3 * torch.randn(64, generator=gc)).cuda()
        x = torch.randn(B, 3, H, W, generator=g, device='cuda')
        s2d = ops.prep_input_pair(x)
        wp = ops.split_pair(ops.pack_stem_weight(w.cuda(), torch.float32))
        if mode == 'fp16p-biglo':     # lo planes as large as the hi planes, where the hi plane holds an image / filter value
            s2d = (s2d[0], (torch.randn(s2d[0].shape, generator=g, device='cuda') * 0.5).half() * (s2d[0] != 0))
            wp = (wp[0], (torch.randn(wp[0].shape, generator=g, device='cuda') / 147 ** 0.5).half() * (wp[0] != 0))
        wh, wl = _unpack_w(d_(wp[0])), _unpack_w(d_(wp[1]))
        run = lambda b0=0, b1=B: ops.stem_pool_pair((s2d[0][b0:b1], s2d[1][b0:b1]), wp, bias, (OH, OW))   # noqa: E731

        def ref_of(b):      # the terms the kernel forms: x_hi . (w_hi + w_lo) + x_lo . w_hi (x_lo . w_lo is dropped by design)
            xh, xl = _unpack_s2d(d_(s2d[0][b:b + 1]), H, W), _unpack_s2d(d_(s2d[1][b:b + 1]), H, W)
            conv = F.conv2d(xh, wh + wl, d_(bias), 2, 3) + F.conv2d(xl, wh, None, 2, 3)
            return F.max_pool2d(F.relu(conv), 3, 2, 1).permute(0, 2, 3, 1)[0]
        tol = lambda ref: 4e-6 * max(1.0, float(ref.abs().max()))                            # noqa: E731
        joined = lambda y, b: y[0][b].double().cpu() + y[1][b].double().cpu()                # noqa: E731
    else:
        dt = DTYPES[mode]
        bias = (0.3 * torch.randn(64, generator=gc)).cuda()
        x = torch.randn(B, 3, H, W, generator=g, device='cuda')
        s2d = ops.prep_input(x, dt)
        wpk = ops.pack_stem_weight(w.cuda(), dt)
        w_eff = _unpack_w(d_(wpk))
        run = lambda b0=0, b1=B: (ops.stem_pool(s2d[b0:b1], wpk, bias, (OH, OW)),)          # noqa: E731
        ref_of = lambda b: _stem_ref_f64(_unpack_s2d(d_(s2d[b:b + 1]), H, W), w_eff, d_(bias))[0]   # noqa: E731
        tol = None
        joined = lambda y, b: y[0][b].double().cpu()                                         # noqa: E731
    y = run()
    torch.cuda.synchronize()
    for b in _images(B, H * W // 4):
        ref = ref_of(b).reshape(-1, 64)
        got = joined(y, b).reshape(-1, 64)
        t = _close(got, ref, mode) if tol is None else tol(ref) + 0 * ref
        msg = _fail_report(what + ' image %d' % b, form, shape, b * PH * PW, got, ref, t)
        assert msg is None, msg
    again = run()
    assert all(torch.equal(u, v) for u, v in zip(again, y)), what + ': a repeated launch differs'
    if B > 1:
        for b0, b1, _, _ in _slices(B, H):
            part = run(b0, b1)
            assert all(torch.equal(u, v[b0:b1]) for u, v in zip(part, y)), '%s: images %d-%d alone differ from the batch' % (what, b0, b1 - 1)
    twin = {('stem_pool_u8', 'raw'): 'DIRTORCH_AMD_STEM_U8_PREP', ('stem_pool_pair', 'walk'): 'DIRTORCH_AMD_STEM_PAIR_OLD',
            ('stem_pool_pair', 'twokernel'): 'DIRTORCH_AMD_STEM_PAIR_OLD'}.get(form)
    if twin:
        alt = _twin(monkeypatch, twin, run)
        assert all(torch.equal(u, v) for u, v in zip(alt, y)), '%s: differs from its twin under %s' % (what, twin)
    if form == ('stem_pool_pair', 'walk') and mode == 'fp16p' and row[3] != 'synthetic':
        _engine_raw_stem_twin(row, monkeypatch)


def _engine_raw_stem_twin(row, monkeypatch):
    """The 'walk' form reads the fp32 NCHW image itself (stem_pool_pair_raw_ok: RAW && XPAIR in stem_u8.hip), which only the engine
    launches - dir_stem_pool_pair takes the prep_input_pair planes.  At the row's workload the engine's trunk must equal, bit for bit,
    the trunk of the two-kernel form (DIRTORCH_AMD_STEM_U8_PREP: prep_input_pair, then the same kernel on the planes the rows above
    check against fp64)."""
    import dir_oracle as O
    from dirtorch_amd import nets
    tag, label, sub, wl, rec, shape, _ = row
    arch = next(w[1] for w in WORKLOADS if w[0] == wl)
    B, H, W = shape
    sd = O.synth_state_dict(arch, seed=7)
    x = torch.randn(B, 3, H, W, generator=_gen(tag, 'engine'), device='cuda')

    def run():
        net = nets.create_model(arch + '_rmac', pretrained='')      # (an engine copies the switches when it is created)
        net.load_state_dict(sd)
        net.compute_dtype = 'fp16p'
        net.cuda().eval()
        net.set_profiling(True)
        feat = net.forward_features(x)
        used = {r['name']: r['kernel'] for r in net.get_profile()}
        net.set_profiling(False)
        return feat, used
    raw, used = run()
    assert used.get('conv1+maxpool') == 'stem_pool_pair' and 'prep_input' not in used, used
    two, used2 = _twin(monkeypatch, 'DIRTORCH_AMD_STEM_U8_PREP', run)
    assert used2.get('prep_input') == 'prep_input_pair', used2
    assert torch.equal(raw, two), '%s: the engine\'s raw fp32 stem and its two-kernel form differ in %d trunk elements' % (
        tag, int((raw != two).sum()))


@pytest.mark.parametrize('row,mode', CASES, ids=['%s-%s' % (r[0], m) for r, m in CASES])
def test_engine_case_vs_reference(row, mode, monkeypatch):
    fam = family(row[1])
    if fam == 'seam':
        _seam_case(row, mode, monkeypatch)
    elif fam == 'dual':
        _dual_case(row, mode, monkeypatch)
    elif fam == 'pair':
        _pair_case(row, mode)
    else:
        _stem_case(row, mode, monkeypatch)
