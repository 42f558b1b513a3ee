"""conv_patchw.hip's loader / consumer form after its consumers were re-scheduled (rolling fragment prefetch, patch image
swizzled by the pixel's column, pixel fragments read across the stage barrier): bit for bit against the one-role kernel,
which keeps the linear swizzle and the per-group fragment reads, at the smallest shapes where each of the three can go wrong."""
import pytest
import torch

from test_ops_gpu import DTYPES, RTOL

pytestmark = pytest.mark.gpu

# (H, W, Cin, Cout), B = 2 throughout.
#   Cin = 64: two planes - one plane switch, six stages; Cin = 128: four planes - the plane buffer parity flips three times,
#   planes 2 and 3 land in the buffers planes 0 and 1 were read from.  (Three planes, Cin = 96, would be the smallest such
#   case, but the library's conv entry point takes multiples of 64 only; the four-plane walk begins with the three-plane one.)
#   17 x 33: two tiles each way, the second one row / one column wide - the carried fragments and the column swizzle run along
#   a ragged edge where most of the patch is the out-of-range zero fill; 16 x 32: exactly one tile.
#   Cout = 128 / 256: one / two channel tiles (the packed weight stages of the second tile).
#   W = 70: three tile columns, the last 6 pixels wide - patch column and image column differ by -1, 31 and 63.
SHAPES = [(H, W, Cin, Cout) for (H, W) in ((17, 33), (16, 32)) for Cin in (64, 128) for Cout in (128, 256)] + [(17, 70, 128, 128)]


@pytest.mark.parametrize('H,W,Cin,Cout', SHAPES, ids=lambda v: str(v))
def test_patchw_rescheduled_consumers_are_bit_identical(H, W, Cin, Cout, monkeypatch):
    from dirtorch_amd import ops
    B = 2
    v = ops.conv_variant_names().index('512x128_patch3x3w')
    for dname, dt in DTYPES.items():
        g = torch.Generator(device='cuda').manual_seed(73)
        x = torch.relu(torch.randn(B, H, W, Cin, generator=g, device='cuda')).to(dt)
        w = (torch.randn(Cout, 3, 3, Cin, generator=g, device='cuda') * (2.0 / (9 * Cin)) ** 0.5).to(dt)
        bias = torch.randn(Cout, generator=g, device='cuda') * 0.1
        res = torch.randn(B, H, W, Cout, generator=g, device='cuda').to(dt)
        kw = dict(stride=1, pad=1, relu=True)
        for r in (None, res):
            tag = (dname, r is not None)
            monkeypatch.delenv('DIRTORCH_AMD_NO_PATCHW_LC', raising=False)
            lc = ops.conv_bn_act(x, w, bias, r, variant=v, **kw)
            monkeypatch.setenv('DIRTORCH_AMD_NO_PATCHW_LC', '1')
            one = ops.conv_bn_act(x, w, bias, r, variant=v, **kw)
            monkeypatch.delenv('DIRTORCH_AMD_NO_PATCHW_LC')
            assert torch.equal(lc, one), tag
            ref = ops.conv_bn_act(x, w, bias, r, naive=True, **kw).float()
            err = (lc.float() - ref).abs()
            tol = RTOL[dname] * ref.abs() + RTOL[dname] * ref.abs().mean()
            assert int((err > tol).sum()) == 0, (tag, float(err.max()))
            assert float(lc.float().abs().max()) > 0, tag
