"""The seam kernel (csrc/conv_c3c1.hip) at a stage exit and in place.

  * keep_stride = s: of the block output, only the pixels on rows and columns that are multiples of s reach memory - the ones
    a following 1x1 stride-s downsample reads; the next block's conv1 output is complete.  Checked bit for bit against the
    full-store entry point, with the output tensor pre-filled with a quiet NaN so that a store that should not happen shows.
  * y == res (an identity block written over its input): bit-identical to the out-of-place launch.
  * the engine's default (sparse stores at layer1 -> layer2, identity blocks of layers 2-4 in place) against the same build
    with DIRTORCH_AMD_SEAM_FULL_STORE and DIRTORCH_AMD_NO_INPLACE, on a workspace poisoned with NaNs: descriptors bit for bit.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
QNAN = {'bf16': 0x7FC0, 'fp16': 0x7E00}      # quiet NaN of the dtype, as a bit pattern

# (B, H, W): 2139 pixels = 33.4 tiles of 64 with odd rows and columns, tiles that straddle image borders and a ragged last
# tile; one row; fewer pixels than a tile
KEEP_SHAPES = [(3, 23, 31), (1, 1, 67), (2, 2, 2)]
# (P, P2, form): form 'plain' runs in bf16 and fp16; 'wp' = paired conv3 weights (fp16), conv1's a pair ('wp') or single ('wp1')
FORMS = [(64, 64, 'plain'), (64, 128, 'plain'), (128, 128, 'plain'), (64, 64, 'wp'), (64, 128, 'wp'), (64, 128, 'wp1')]
CASES = [(P, P2, form, d) for P, P2, form in FORMS for d in (['bf16', 'fp16'] if form == 'plain' else ['fp16'])]
CASE_IDS = ['P%d-P2_%d-%s-%s' % c for c in CASES]


def _bits(t):
    return t.view(torch.int16)


def _operands(B, H, W, P, P2, form, dname):
    """Device operands of one seam launch (ReLU'd activations: every stored value is finite) and the two entry points bound to
    them: full(y=None) -> (y, t1) through the EXISTING full-store wrapper, keep(s, y) -> (y, t1) through the new one."""
    from dirtorch_amd import ops
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W + P + P2)
    r = lambda *sh, s=1.0: (torch.randn(*sh, generator=g) * s)      # noqa: E731
    t2 = r(B, H, W, P).relu().to(dt).cuda()
    res = r(B, H, W, 4 * P).relu().to(dt).cuda()
    b3, b1 = r(4 * P, s=0.2).cuda(), r(P2, s=0.2).cuda()
    w3 = r(4 * P, P, s=(2.0 / P) ** 0.5).to(dt).cuda()
    w1 = r(P2, 4 * P, s=(2.0 / (4 * P)) ** 0.5).to(dt).cuda()
    if form == 'plain':
        full = lambda: ops.conv_c3c1(t2, w3, b3, res, w1, b1)      # noqa: E731
        keep = lambda s, y, rs=res: ops.conv_c3c1_keep(t2, w3, b3, rs, w1, b1, keep_stride=s, y=y)      # noqa: E731
    else:
        w3l = (r(4 * P, P, s=(2.0 / P) ** 0.5) / 64).to(dt).cuda()
        w1l = (r(P2, 4 * P, s=(2.0 / (4 * P)) ** 0.5) / 64).to(dt).cuda() if form == 'wp' else None
        full = lambda: ops.conv_c3c1_wpair(t2, (w3, w3l), b3, res, (w1, w1l), b1)      # noqa: E731
        keep = lambda s, y, rs=res: ops.conv_c3c1_wpair_keep(t2, (w3, w3l), b3, rs, (w1, w1l), b1, keep_stride=s, y=y)      # noqa: E731
    return res, full, keep


def _check_sparse(B, H, W, P, P2, form, dname, s):
    res, full, keep = _operands(B, H, W, P, P2, form, dname)
    y_full, t1_full = full()
    y = torch.empty_like(res)
    _bits(y).fill_(QNAN[dname])
    y_out, t1 = keep(s, y)
    torch.cuda.synchronize()
    assert y_out.data_ptr() == y.data_ptr()
    kept = torch.zeros(B, H, W, dtype=torch.bool, device='cuda')
    kept[:, ::s, ::s] = True
    yb, fb = _bits(y), _bits(y_full)
    assert torch.equal(yb[kept], fb[kept]), 'kept pixels differ from the full-store launch'
    assert bool((yb[~kept] == QNAN[dname]).all()), 'a dropped pixel was stored'
    assert not bool((fb[kept] == QNAN[dname]).any())       # (the sentinel cannot be mistaken for a stored value)
    assert torch.equal(_bits(t1), _bits(t1_full)), "the next block's conv1 output differs"


@pytest.mark.parametrize('P,P2,form,dname', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('B,H,W', KEEP_SHAPES)
def test_stage_exit_stores_only_the_pixels_a_stride_2_downsample_reads(B, H, W, P, P2, form, dname):
    _check_sparse(B, H, W, P, P2, form, dname, 2)


def test_stage_exit_store_at_stride_3():
    """"Even" is not hard-coded: rows and columns that are multiples of 3."""
    _check_sparse(3, 23, 31, 64, 128, 'plain', 'fp16', 3)


def test_keep_stride_0_and_1_store_every_pixel():
    res, full, keep = _operands(3, 23, 31, 64, 128, 'plain', 'bf16')
    y_full, t1_full = full()
    for s in (0, 1):
        y, t1 = keep(s, None)
        assert torch.equal(_bits(y), _bits(y_full)) and torch.equal(_bits(t1), _bits(t1_full))


@pytest.mark.parametrize('s', [0, 2], ids=['full', 'keep2'])
@pytest.mark.parametrize('P,P2,form,dname', [(64, 64, 'plain', 'bf16'), (128, 128, 'plain', 'fp16'), (64, 128, 'wp', 'fp16')],
                         ids=['plain-P64', 'plain-P128', 'wp-to-layer2'])
def test_in_place_equals_out_of_place(P, P2, form, dname, s):
    """y aliases (a clone of) res.  2 x 140 x 140 = 39200 pixels = 613 tiles (the last one ragged): every persistent workgroup
    walks more than two tiles, so the residual prefetched one tile ahead is the common case."""
    B, H, W = 2, 140, 140
    res, full, keep = _operands(B, H, W, P, P2, form, dname)
    y_out = torch.empty_like(res)
    _bits(y_out).fill_(QNAN[dname])
    y_out, t1_out = keep(s, y_out)
    buf = res.clone()
    y_in, t1_in = keep(s, buf, buf)
    torch.cuda.synchronize()
    assert y_in.data_ptr() == buf.data_ptr()
    kept = torch.zeros(B, H, W, dtype=torch.bool, device='cuda')
    kept[:, ::max(s, 1), ::max(s, 1)] = True
    assert torch.equal(_bits(y_in)[kept], _bits(y_out)[kept])
    assert torch.equal(_bits(y_in)[~kept], _bits(res)[~kept])      # dropped pixels: the residual is still there
    assert torch.equal(_bits(t1_in), _bits(t1_out))
    if s == 0:
        y_full, t1_full = full()
        assert torch.equal(_bits(y_in), _bits(y_full)) and torch.equal(_bits(t1_in), _bits(t1_full))


def test_ds_and_layer3_forms_refuse_a_keep_stride():
    """The forms that never close a stage have no sparse store: asked for one they fail instead of storing everything."""
    from dirtorch_amd import _lib, ops
    z = lambda *sh: torch.zeros(*sh, dtype=torch.float16, device='cuda')      # noqa: E731
    f = lambda n: torch.zeros(n, device='cuda')      # noqa: E731
    with pytest.raises(_lib.DirError):      # planes 256
        ops.conv_c3c1_keep(z(1, 8, 8, 256), z(1024, 256), f(1024), z(1, 8, 8, 1024), z(256, 1024), f(256), keep_stride=2)
    with pytest.raises(_lib.DirError):
        ops.conv_c3c1_keep(z(1, 8, 8, 64), z(256, 64), f(256), z(1, 8, 8, 256), z(64, 256), f(64), keep_stride=-1)


# ---- engine level ---------------------------------------------------------------------------------------------------------
def _make_net(factory, sd, dtype):
    from dirtorch_amd import nets
    net = nets.create_model(factory, pretrained='')
    net.load_state_dict(sd)
    net.compute_dtype = dtype
    net.cuda()
    return net.eval()


def _poisoned_forward(net, x, dtype):
    """One forward on a workspace filled with quiet NaNs (the workspace is a tensor the Python wrapper owns and reuses):
    whatever the forward reads without having written it shows in the output."""
    B, H, W, _ = x.shape
    net(x)                                       # builds the engine, allocates the workspace
    ws = net._workspace(B, H, W)
    ws[:ws.numel() // 2 * 2].view(torch.int16).fill_(QNAN['bf16' if dtype == 'bf16' else 'fp16'])
    out = net(x).clone()
    assert net._workspace(B, H, W).data_ptr() == ws.data_ptr()
    return out


def _two_arms(factory, sd, dtype, x, force, monkeypatch):
    for k in ('DIRTORCH_AMD_SEAM_FULL_STORE', 'DIRTORCH_AMD_NO_INPLACE', 'DIRTORCH_AMD_C3C1'):
        monkeypatch.delenv(k, raising=False)
    if force:
        monkeypatch.setenv('DIRTORCH_AMD_C3C1', 'force')
    net = _make_net(factory, sd, dtype)
    d_new = _poisoned_forward(net, x, dtype)
    net.set_profiling(True)
    net(x)
    prof = {r['name']: r for r in net.get_profile()}
    monkeypatch.setenv('DIRTORCH_AMD_SEAM_FULL_STORE', '1')
    monkeypatch.setenv('DIRTORCH_AMD_NO_INPLACE', '1')
    ref = _make_net(factory, sd, dtype)
    d_ref = ref(x)
    ref.set_profiling(True)
    ref(x)
    prof_ref = {r['name']: r for r in ref.get_profile()}
    return d_new, d_ref, prof, prof_ref


@pytest.mark.parametrize('dtype', ['fp16p', 'bf16'])
@pytest.mark.parametrize('B,H,W,force', [(2, 354, 482, True), (8, 512, 512, False)], ids=['b2_354x482_forced', 'b8_512'])
def test_engine_sparse_stores_in_place_bit_identical(B, H, W, force, dtype, monkeypatch):
    """ResNet-50: the layer1 map is 89 x 121 (odd both ways; the seam through DIRTORCH_AMD_C3C1=force) or 128 x 128 at batch 8
    (2048 tiles: the seam by the engine's own threshold)."""
    import dir_oracle as O
    sd = O.synth_state_dict('resnet50', seed=7)
    g = torch.Generator(device='cuda').manual_seed(31)
    x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8, device='cuda')
    d_new, d_ref, prof, prof_ref = _two_arms('resnet50_rmac', sd, dtype, x, force, monkeypatch)
    # the seam that closes layer1 ran in both arms, under its unchanged label, and the record counts the stores it makes
    seam, seam_ref = prof['layer1.2.c3c1'], prof_ref['layer1.2.c3c1']
    assert seam['kernel'] == seam_ref['kernel'] and seam['kernel'].startswith('conv_c3c1<64')
    h, w = (H + 1) // 2, (W + 1) // 2
    h, w = (h + 1) // 2, (w + 1) // 2           # the layer1 map
    dropped = 2.0 * 256 * B * (h * w - ((h + 1) // 2) * ((w + 1) // 2))
    assert seam_ref['bytes'] - seam['bytes'] == dropped, (seam_ref['bytes'], seam['bytes'], dropped)
    assert [r for r in prof] == [r for r in prof_ref]      # the same launches, in the same order
    assert torch.isfinite(d_new).all()
    assert torch.equal(d_new, d_ref)


def test_engine_fpn_head_keeps_layer3_bit_identical(monkeypatch):
    """An FPN head parks layer3's output in its own buffer (never in place, never sparse); layers 1-2 in front of it take the
    new default.  Same comparison."""
    import dir_oracle as O
    sd = O.synth_state_dict('resnet50', seed=9, out_dim=3072, gemp=2.6, pooling='gem', head='fpn')
    g = torch.Generator(device='cuda').manual_seed(37)
    x = torch.randint(0, 256, (2, 354, 482, 3), generator=g, dtype=torch.uint8, device='cuda')
    d_new, d_ref, prof, _ = _two_arms('resnet50_fpn_rmac', sd, 'fp16p', x, True, monkeypatch)
    assert 'layer1.2.c3c1' in prof
    assert torch.isfinite(d_new).all()
    assert torch.equal(d_new, d_ref)
