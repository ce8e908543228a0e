"""hcir_conv2d_f16, hcir_resnet_stem and hcir_avgpool_nhwc_f16 against float64 references.

Convolution reference: F.conv2d in float64 on the same fp16-rounded x and w, then the float64 epilogue.  The bound is
derived and holds for EVERY element: the fp16 store contributes 2^-11 relative, fp32 accumulation of K terms is bounded
(loosely, with headroom) by 2^-20 * sum|a||w|:

    |out - ref| <= 2^-10 |ref| + 2^-20 (|x| * |w|) |scale| + 2^-24

with the convolution of absolute values computed here.  Every output buffer sits between two canary rows."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CANARY = 1234.0


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _guarded(shape):
    """fp16 output of `shape` (last dim = row) with one canary row in front and one behind."""
    row = shape[-1]
    n = math.prod(shape)
    buf = torch.full((n + 2 * row,), CANARY, dtype=torch.float16, device="cuda")
    return buf, buf[row:row + n].view(shape)


def _canaries_intact(buf, row):
    return bool((buf[:row] == CANARY).all()) and bool((buf[-row:] == CANARY).all())


def _conv_case(b, h, w, cin, cout, r, stride, relu, resid, seed=0, tile_n=64):
    """Runs the kernel twice; returns (max ratio err / bound, the two outputs equal, canaries intact).
    tile_n: the output-channel tile (kernel instantiation) the case is there for; asserted."""
    from hcir import _lib, ops
    pad = 1 if r == 3 else 0
    assert _lib.lib().hcir_conv2d_tile_n(b, h, w, cin, cout, r, r, stride, pad) == tile_n
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, h, w, generator=g).half()
    wt = (torch.randn(cout, cin, r, r, generator=g) / math.sqrt(cin * r * r)).half()
    scale = torch.randn(cout, generator=g)                  # both signs: ReLU must come after the affine
    scale[0], scale[1] = -1.5, 2.0
    bias = 0.5 * torch.randn(cout, generator=g)
    acc = F.conv2d(x.double(), wt.double(), None, stride, pad)
    absacc = F.conv2d(x.double().abs(), wt.double().abs(), None, stride, pad)
    sc, bi = scale.double().view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
    ref = acc * sc + bi
    res = None
    if resid:
        res = torch.randn(ref.shape, generator=g).half()
        ref = ref + res.double()
    if relu:
        ref = ref.clamp_min(0)
    bound = 2.0 ** -10 * ref.abs() + 2.0 ** -20 * absacc * sc.abs() + 2.0 ** -24

    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    wd = wt.permute(0, 2, 3, 1).contiguous().cuda()
    rd = None if res is None else res.permute(0, 2, 3, 1).contiguous().cuda()
    shape = (b, ref.shape[2], ref.shape[3], cout)
    outs = []
    ok = True
    for _ in range(2):
        buf, out = _guarded(shape)
        got = ops.conv2d_f16(xd, wd, scale.cuda(), bias.cuda(), stride, pad, resid=rd, relu=relu, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        ok = ok and _canaries_intact(buf, cout)
        outs.append(out.clone())
    o = outs[0].cpu().double().permute(0, 3, 1, 2)
    assert torch.isfinite(o).all()
    ratio = ((o - ref).abs() / bound).max().item()
    if relu:
        assert (o >= 0).all()
    return ratio, torch.equal(outs[0], outs[1]), ok


CONV_CASES = [
    # b, h, w, cin, cout, r, stride, relu, resid
    pytest.param(2, 7, 7, 64, 64, 3, 1, True, False, id="3x3s1-7x7-M98-tile-spans-two-images"),
    pytest.param(3, 9, 5, 64, 64, 3, 1, True, False, id="3x3s1-9x5-odd"),
    pytest.param(2, 14, 14, 128, 128, 3, 2, True, False, id="3x3s2-14to7"),
    pytest.param(2, 15, 15, 128, 128, 3, 2, True, False, id="3x3s2-15to8-odd"),
    pytest.param(2, 14, 14, 256, 512, 1, 2, False, False, id="1x1s2-downsample"),
    pytest.param(2, 7, 7, 512, 2048, 1, 1, True, True, id="1x1s1-512to2048-resid-relu"),
    pytest.param(1, 56, 56, 64, 256, 1, 1, True, False, id="1x1s1-56x56-M3136"),
    pytest.param(1, 1, 1, 512, 512, 3, 1, True, False, id="longK-1x1-input-only-centre-tap"),
    pytest.param(1, 3, 3, 512, 512, 3, 1, True, False, id="longK-3x3-input"),
    pytest.param(5, 28, 28, 64, 128, 3, 1, True, True, id="3x3s1-M3920-resid"),
]

# The 128-wide output-channel tile (conv2d_f16_kernel<128>: two n tiles per wave, 64 accumulators, 64 KB of LDS) runs
# only when the launch has >= 512 workgroups of 128 x 128, i.e. M * Cout >= 2^23: the smallest shapes that reach it.
# Every one has a ragged last M tile, and an image size that is no multiple of 128, so M tiles straddle images.
WIDE_CASES = [
    pytest.param(21, 56, 56, 64, 128, 3, 1, True, True, id="wide-3x3s1-56x56-M65856-resid"),       # 514.5 M tiles
    pytest.param(11, 109, 109, 64, 256, 3, 2, True, False, id="wide-3x3s2-109to55-M33275"),         # odd input
    pytest.param(3, 53, 53, 64, 1024, 1, 1, True, True, id="wide-1x1s1-64to1024-M8427-resid"),
    pytest.param(3, 105, 105, 256, 1024, 1, 2, False, False, id="wide-1x1s2-downsample-M8427"),
]


@pytest.mark.parametrize("b,h,w,cin,cout,r,stride,relu,resid", CONV_CASES)
def test_conv2d_f16_vs_float64(b, h, w, cin, cout, r, stride, relu, resid):
    ratio, same, canaries = _conv_case(b, h, w, cin, cout, r, stride, relu, resid)
    print(f"conv max err/bound {ratio:.3f}")
    assert canaries, "canary row overwritten"
    assert same, "two calls on the same input differ"
    assert ratio <= 1.0


@pytest.mark.parametrize("b,h,w,cin,cout,r,stride,relu,resid", WIDE_CASES)
def test_conv2d_f16_wide_tile_vs_float64(b, h, w, cin, cout, r, stride, relu, resid):
    ratio, same, canaries = _conv_case(b, h, w, cin, cout, r, stride, relu, resid, seed=3, tile_n=128)
    print(f"conv (128-wide tile) max err/bound {ratio:.3f}")
    assert canaries, "canary row overwritten"
    assert same, "two calls on the same input differ"
    assert ratio <= 1.0


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("resid", [False, True])
def test_conv2d_epilogue_switches(relu, resid):
    ratio, same, canaries = _conv_case(2, 6, 5, 64, 128, 3, 1, relu, resid, seed=7)
    print(f"conv max err/bound {ratio:.3f}")
    assert canaries and same and ratio <= 1.0


def test_conv2d_rejects_unsupported_and_mismatched():
    from hcir import HcirError, ops
    x = torch.zeros(1, 4, 4, 48, dtype=torch.float16, device="cuda")
    w = torch.zeros(64, 3, 3, 48, dtype=torch.float16, device="cuda")
    s = torch.ones(64, device="cuda")
    with pytest.raises(HcirError, match="status -2"):
        ops.conv2d_f16(x, w, s, s, 1, 1)
    x = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device="cuda")
    w = torch.zeros(64, 3, 3, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(HcirError):
        ops.conv2d_f16(x, w, s, s, 1, 1, resid=torch.zeros(1, 4, 4, 128, dtype=torch.float16, device="cuda"))
    with pytest.raises(HcirError):
        ops.conv2d_f16(x.cpu(), w, s, s, 1, 1)


@pytest.mark.parametrize("h,w", [(32, 32), (37, 41), (224, 224), (7, 9)])
def test_resnet_stem_vs_float64(h, w):
    """max_pool2d(relu(bn(conv2d))) in float64 on the fp16-rounded weights AND the fp16-rounded image (the kernel
    rounds the fp32 image to fp16 for the MFMA, include/hcir.h).  Pre-pool, the fp32 value differs from the float64 one
    by at most e = 2^-20 (|x| * |w|) |scale| + 2^-24; a max of values moves by at most the max of their moves, and the
    one fp16 store adds 2^-11 relative: |out - ref| <= 2^-10 |ref| + maxpool(e)."""
    from hcir import ops
    from hcir.resnet_engine import pack_stem_weight
    g = torch.Generator().manual_seed(h * 1000 + w)
    b = 2
    x = torch.randn(b, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147.0)
    scale = torch.randn(64, generator=g)
    bias = 0.5 * torch.randn(64, generator=g)
    x16, w16 = x.half().double(), wt.half().double()
    sc, bi = scale.double().view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
    pre = (F.conv2d(x16, w16, None, 2, 3) * sc + bi).clamp_min(0)
    e = 2.0 ** -20 * F.conv2d(x16.abs(), w16.abs(), None, 2, 3) * sc.abs() + 2.0 ** -24
    ref = F.max_pool2d(pre, 3, 2, 1)                       # pads with -inf: padding never wins
    bound = 2.0 ** -10 * ref.abs() + F.max_pool2d(e, 3, 2, 1)
    assert tuple(ref.shape[2:]) == (ops.stem_out_size(h), ops.stem_out_size(w))
    shape = (b, ref.shape[2], ref.shape[3], 64)
    outs = []
    for _ in range(2):
        buf, out = _guarded(shape)
        ops.resnet_stem(x.cuda(), pack_stem_weight(wt).cuda(), scale.cuda(), bias.cuda(), out=out)
        torch.cuda.synchronize()
        assert _canaries_intact(buf, 64), "canary row overwritten"
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    o = outs[0].cpu().double().permute(0, 3, 1, 2)
    assert torch.isfinite(o).all()
    ratio = ((o - ref).abs() / bound).max().item()
    print(f"stem {h}x{w} max err/bound {ratio:.3f}")
    assert ratio <= 1.0


def test_resnet_stem_padding_sentinel_never_leaks():
    """The pool's padding positions are excluded from the max (the kernel holds them as -inf).  Every window has its
    centre inside the conv map, so no -inf may reach the output: with scale = bias = 0 the conv map is all zeros
    and every pooled value, the border ones included, must be 0 at an odd, non-square size."""
    from hcir import ops
    from hcir.resnet_engine import pack_stem_weight
    x = torch.randn(1, 3, 9, 13, generator=torch.Generator().manual_seed(0)).cuda()
    wt = torch.randn(64, 3, 7, 7, generator=torch.Generator().manual_seed(1))
    z = torch.zeros(64, device="cuda")
    out = ops.resnet_stem(x, pack_stem_weight(wt).cuda(), z, z)
    assert tuple(out.shape) == (1, 3, 4, 64) and bool((out == 0).all())


@pytest.mark.parametrize("h,w,c", [(7, 7, 2048), (2, 2, 512)])
@pytest.mark.parametrize("signed", [False, True])
def test_avgpool_nhwc_vs_float64(h, w, c, signed):
    """Compensated fp32 summation: the sum is within 2 ulp (2^-23) of sum|x|, the division adds one rounding.
    signed=False is the required check: non-negative input (what the trunk feeds it, post-ReLU), sum|x| = |sum|, so
    every element is within 1e-6 RELATIVE to the float64 mean.  signed=True is an extra ABSOLUTE-error check, not the
    required relative bound: with cancellation no fp32 sum can be 1e-6 relative to a mean near zero, so the error is
    measured against mean|x| (the same absolute error as in the non-negative case)."""
    from hcir import ops
    b = 3
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(b, h, w, c, generator=g).half()
    if not signed:
        x = x.abs()
    ref = x.double().mean(dim=(1, 2))
    scale = ref.abs() if not signed else x.double().abs().mean(dim=(1, 2))
    xd = x.cuda()
    out = ops.avgpool_nhwc(xd)
    assert out.dtype == torch.float32 and tuple(out.shape) == (b, c)
    assert torch.equal(out, ops.avgpool_nhwc(xd))
    err = ((out.cpu().double() - ref).abs() / scale).max().item()
    print(f"avgpool {h}x{w}x{c} signed={signed} max rel err {err:.2e}")
    assert err <= 1e-6
    # l2_normalize: unit rows, same direction as F.normalize of the float64 mean
    buf = torch.full((b + 2, c), CANARY, dtype=torch.float32, device="cuda")
    nrm = ops.avgpool_nhwc(xd, l2_normalize=True, out=buf[1:b + 1])
    torch.cuda.synchronize()
    assert bool((buf[0] == CANARY).all()) and bool((buf[-1] == CANARY).all())
    assert torch.equal(nrm, ops.avgpool_nhwc(xd, l2_normalize=True))
    n64 = nrm.cpu().double()
    assert ((n64.norm(dim=1) - 1).abs() <= 1e-6).all()
    assert ((n64 - F.normalize(ref, dim=1)).abs().max().item()) <= 1e-6
