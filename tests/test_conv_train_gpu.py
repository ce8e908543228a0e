"""hcir_conv2d_wgrad_f16, hcir_spread2_nhwc_f16 and hcir.conv_train.conv2d_nhwc against float64 references.

Ground truth: float64 autograd of F.conv2d on the fp16-rounded x, w and dy.  Bounds hold for EVERY element:

    weight gradient (fp32 out)   |dw - ref| <= 2^-20 (|dy|^T |x_cols|) + 2^-24
    data gradient (fp16 out)     |dx - ref| <= 2^-10 |ref| + 2^-20 (|dy| * |w|) + 2^-24

i.e. the accumulation term of tests/test_conv_gpu.py (fp32 accumulation, loosely, with headroom) with the sums of
absolute products computed here, plus the one fp16 store for dx.  With plain fp32 accumulation on the CPU the worst
weight-gradient ratio over CASES was 0.27; one dropped pixel row exceeds the bound by more than 3000x.
Every case runs twice and the two runs must be bit-equal; directly written buffers sit between canary rows."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CANARY = 1234.0


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _guarded(shape, dtype):
    row = shape[-1]
    n = math.prod(shape)
    buf = torch.full((n + 2 * row,), CANARY, dtype=dtype, device="cuda")
    return buf, buf[row:row + n].view(shape)


def _canaries_intact(buf, row):
    return bool((buf[:row] == CANARY).all()) and bool((buf[-row:] == CANARY).all())


# b, h, w, cin, cout, r, stride
CASES = [
    pytest.param(2, 7, 7, 64, 64, 3, 1, id="3x3s1-7x7-M98"),
    pytest.param(3, 9, 5, 64, 128, 3, 1, id="3x3s1-9x5-odd"),
    pytest.param(2, 14, 14, 128, 64, 3, 2, id="3x3s2-14to7"),
    pytest.param(2, 15, 13, 64, 64, 3, 2, id="3x3s2-15x13-odd"),
    pytest.param(2, 14, 14, 256, 512, 1, 2, id="1x1s2-14to7"),
    pytest.param(2, 15, 13, 64, 128, 1, 2, id="1x1s2-15x13-odd"),
    pytest.param(2, 7, 7, 512, 2048, 1, 1, id="1x1s1-512to2048"),
    pytest.param(2, 7, 7, 2048, 512, 1, 1, id="1x1s1-2048to512"),
    pytest.param(1, 1, 1, 512, 512, 3, 1, id="3x3s1-1x1-input-only-centre-tap"),
    pytest.param(1, 2, 1, 64, 64, 3, 2, id="3x3s2-2x1-Ho-Wo-1"),
    pytest.param(4, 28, 28, 64, 64, 3, 1, id="3x3s1-28x28-M3136"),
]

# Chosen from the split plan (csrc/conv_plan.h): splits = min(steps, ceil(512 / tiles)) over steps = ceil(M / 64),
# rows per split = ceil(steps / splits) * 64.
#   256 -> 256 3x3 at 2 x 23 x 23: tiles 2 * 2 * 9 = 36, M = 1058, steps 17, 15 wanted -> 128 rows per split,
#       9 splits, the last one with 1058 - 8 * 128 = 34 rows: fewer steps than the others AND a ragged step
#   128 -> 64 1x1 at 1 x 8 x 7: M = 56 < 64, one ragged step, one split: written straight to dw, no workspace
SPLIT_CASES = [
    pytest.param(2, 23, 23, 256, 256, 3, 1, 9, id="splits9-last-split-34-rows"),
    pytest.param(1, 8, 7, 128, 64, 1, 1, 1, id="splits1-M56-no-workspace"),
]

_REFS = {}


def _reference(b, h, w, cin, cout, r, stride):
    """Inputs (fp16, NCHW / OIHW) and the float64 gradients and bounds of one case, computed once and shared."""
    key = (b, h, w, cin, cout, r, stride)
    if key not in _REFS:
        pad = 1 if r == 3 else 0
        g = torch.Generator().manual_seed(b * 1000 + h * 10 + cin + r + stride)
        x = torch.randn(b, cin, h, w, generator=g).half()
        wt = (torch.randn(cout, cin, r, r, generator=g) / math.sqrt(cin * r * r)).half()
        ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
        dy = torch.randn(b, cout, ho, wo, generator=g).half()

        def grads(xx, ww, gg):
            xx, ww = xx.double().requires_grad_(True), ww.double().requires_grad_(True)
            return torch.autograd.grad(F.conv2d(xx, ww, None, stride, pad), [xx, ww], gg.double())

        dx, dw = grads(x, wt, dy)
        adx, adw = grads(x.abs(), wt.abs(), dy.abs())
        _REFS[key] = dict(pad=pad, x=x, w=wt, dy=dy, dx=dx, dw=dw,
                          dw_bound=2.0 ** -20 * adw + 2.0 ** -24,
                          dx_bound=2.0 ** -10 * dx.abs() + 2.0 ** -20 * adx + 2.0 ** -24)
    return _REFS[key]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _wgrad_case(b, h, w, cin, cout, r, stride):
    from hcir import ops
    ref = _reference(b, h, w, cin, cout, r, stride)
    xd, dyd = _nhwc(ref["x"]), _nhwc(ref["dy"])
    outs = []
    for _ in range(2):
        buf, out = _guarded((cout, r, r, cin), torch.float32)
        got = ops.conv2d_wgrad(xd, dyd, r, stride, ref["pad"], out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert _canaries_intact(buf, cin), "canary row overwritten"
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]), "two calls on the same input differ"
    o = outs[0].cpu().double().permute(0, 3, 1, 2)      # [Cout,R,S,Cin] -> [Cout,Cin,R,S]
    assert torch.isfinite(o).all()
    return o, ((o - ref["dw"]).abs() / ref["dw_bound"]).max().item()


@pytest.mark.parametrize("b,h,w,cin,cout,r,stride", CASES)
def test_wgrad_vs_float64(b, h, w, cin, cout, r, stride):
    o, ratio = _wgrad_case(b, h, w, cin, cout, r, stride)
    print(f"wgrad max err/bound {ratio:.3f}")
    assert ratio <= 1.0
    if (h, w, r) == (1, 1, 3):      # a 1 x 1 input under a 3 x 3: only the centre tap ever sees a pixel
        centre = torch.zeros(3, 3, dtype=torch.bool)
        centre[1, 1] = True
        assert bool((o[:, :, ~centre] == 0).all()) and bool((o[:, :, 1, 1] != 0).any())


@pytest.mark.parametrize("b,h,w,cin,cout,r,stride,splits", SPLIT_CASES)
def test_wgrad_split_paths(b, h, w, cin, cout, r, stride, splits):
    from hcir import ops
    pad = 1 if r == 3 else 0
    assert ops.conv2d_wgrad_splits(b, h, w, cin, cout, r, stride, pad) == splits
    _, ratio = _wgrad_case(b, h, w, cin, cout, r, stride)
    print(f"wgrad ({splits} splits) max err/bound {ratio:.3f}")
    assert ratio <= 1.0


def test_wgrad_rejects_unsupported_and_mismatched():
    from hcir import HcirError, ops
    x = torch.zeros(1, 4, 4, 48, dtype=torch.float16, device="cuda")
    dy = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(HcirError, match="status -2"):
        ops.conv2d_wgrad(x, dy, 3, 1, 1)
    x = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(HcirError):
        ops.conv2d_wgrad(x, dy[:, :3].contiguous(), 3, 1, 1)          # dy is not the conv's output shape
    with pytest.raises(HcirError):
        ops.conv2d_wgrad(x, dy, 3, 1, 1, out=torch.zeros(64, 64, 3, 3, device="cuda"))     # [Cout,Cin,R,S], not [Cout,R,S,Cin]
    with pytest.raises(HcirError):
        ops.conv2d_wgrad(x.float(), dy, 3, 1, 1)


@pytest.mark.parametrize("b,h,w,cin,cout,r,stride", CASES)
def test_dgrad_through_the_function_backward(b, h, w, cin, cout, r, stride, monkeypatch):
    from hcir import conv_train, ops
    ref = _reference(b, h, w, cin, cout, r, stride)
    spreads = []
    real = ops.spread2_nhwc
    monkeypatch.setattr(ops, "spread2_nhwc", lambda *a, **k: spreads.append(real(*a, **k)) or spreads[-1])
    weight = ref["w"].float().cuda()             # the master weight: here fp16-representable, as the reference's
    dyd = _nhwc(ref["dy"])
    outs = []
    for _ in range(2):
        xd = _nhwc(ref["x"]).requires_grad_(True)
        y = conv_train.conv2d_nhwc(xd, weight, stride, ref["pad"])
        assert y.dtype == torch.float16 and tuple(y.shape) == tuple(dyd.shape)
        (dx,) = torch.autograd.grad(y, [xd], dyd)
        outs.append(dx)
    assert torch.equal(outs[0], outs[1]), "two calls on the same input differ"
    dx = outs[0]
    assert dx.dtype == torch.float16 and tuple(dx.shape) == (b, h, w, cin)
    o = dx.cpu().double().permute(0, 3, 1, 2)
    assert torch.isfinite(o).all()
    ratio = ((o - ref["dx"]).abs() / ref["dx_bound"]).max().item()
    print(f"dgrad max err/bound {ratio:.3f}")
    assert ratio <= 1.0
    assert len(spreads) == (2 if stride == 2 else 0)
    if stride == 2 and r == 3:      # the spread buffer is dy on the even grid of the INPUT's size, zero elsewhere
        z = spreads[0]
        assert tuple(z.shape) == (b, h, w, cout)
        assert bool((z[:, 1::2] == 0).all()) and bool((z[:, :, 1::2] == 0).all())
        assert torch.equal(z[:, ::2, ::2], dyd)
    if stride == 2 and r == 1:      # a stride-2 1x1 never reads the odd positions: their gradient is exactly zero
        assert bool((dx[:, 1::2] == 0).all()) and bool((dx[:, :, 1::2] == 0).all())


@pytest.mark.parametrize("hs,ws,h,w", [(7, 7, 14, 14), (8, 7, 15, 13), (1, 1, 2, 1), (1, 1, 1, 1)])
def test_spread2_bitwise(hs, ws, h, w):
    from hcir import ops
    b, c = 3, 64
    src = torch.randn(b, hs, ws, c, generator=torch.Generator().manual_seed(hs * 10 + w)).half().cuda()
    want = torch.zeros(b, h, w, c, dtype=torch.float16, device="cuda")
    want[:, 0:2 * hs:2, 0:2 * ws:2] = src
    buf, out = _guarded((b, h, w, c), torch.float16)       # the canary value also fills `out`: every element is written
    ops.spread2_nhwc(src, h, w, out=out)
    torch.cuda.synchronize()
    assert _canaries_intact(buf, c), "canary row overwritten"
    assert torch.equal(out, want)


def test_spread2_rejects_a_map_that_does_not_fit():
    from hcir import HcirError, ops
    src = torch.zeros(1, 8, 7, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(HcirError, match="status -1"):
        ops.spread2_nhwc(src, 14, 13)             # 2 * (8 - 1) > 14 - 1
    with pytest.raises(HcirError):
        ops.spread2_nhwc(src.float(), 15, 13)


def test_conv2d_nhwc_end_to_end():
    """Both gradients of a random-weighted sum from torch.autograd.grad, with an fp32 master weight that is NOT
    fp16-representable (the reference is taken on its fp16 rounding, which is what the kernels multiply)."""
    from hcir import conv_train
    b, h, w, cin, cout, r, stride, pad = 2, 9, 6, 128, 64, 3, 2, 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, cin, h, w, generator=g).half()
    wm = torch.randn(cout, cin, r, r, generator=g) / math.sqrt(cin * r * r)
    ho, wo = (h + 2 - r) // 2 + 1, (w + 2 - r) // 2 + 1
    rw = torch.randn(b, cout, ho, wo, generator=g).half()

    def grads(xx, ww, gg):
        xx, ww = xx.double().requires_grad_(True), ww.double().requires_grad_(True)
        return torch.autograd.grad(F.conv2d(xx, ww, None, stride, pad), [xx, ww], gg.double())

    dx64, dw64 = grads(x, wm.half(), rw)
    adx, adw = grads(x.abs(), wm.half().abs(), rw.abs())
    xd = _nhwc(x).requires_grad_(True)
    weight = torch.nn.Parameter(wm.cuda())
    y = conv_train.conv2d_nhwc(xd, weight, stride, pad)
    y64 = F.conv2d(x.double(), wm.half().double(), None, stride, pad)
    assert ((y.detach().cpu().double().permute(0, 3, 1, 2) - y64).abs() <= 2.0 ** -10 * y64.abs() + 2.0 ** -20 * F.conv2d(
        x.double().abs(), wm.half().double().abs(), None, stride, pad) + 2.0 ** -24).all()
    dx, dw = torch.autograd.grad((y * _nhwc(rw)).sum(), [xd, weight])
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (cout, cin, r, r) and dw.is_contiguous()
    rx = ((dx.cpu().double().permute(0, 3, 1, 2) - dx64).abs() / (2.0 ** -10 * dx64.abs() + 2.0 ** -20 * adx + 2.0 ** -24))
    rwt = ((dw.cpu().double() - dw64).abs() / (2.0 ** -20 * adw + 2.0 ** -24))
    print(f"conv2d_nhwc dx err/bound {rx.max().item():.3f}, dw err/bound {rwt.max().item():.3f}")
    assert rx.max().item() <= 1.0 and rwt.max().item() <= 1.0


def test_conv2d_nhwc_accumulates_and_follows_the_optimizer():
    from hcir import conv_train, ops
    from hcir.resnet_engine import pack_conv_weight
    g = torch.Generator().manual_seed(12)
    weight = torch.nn.Parameter((torch.randn(64, 64, 3, 3, generator=g) / 24.0).cuda())
    x1 = torch.randn(2, 5, 5, 64, generator=g).half().cuda()
    x2 = torch.randn(2, 5, 5, 64, generator=g).half().cuda()
    r1 = torch.randn(2, 5, 5, 64, generator=g).half().cuda()
    r2 = torch.randn(2, 5, 5, 64, generator=g).half().cuda()
    (g1,) = torch.autograd.grad((conv_train.conv2d_nhwc(x1, weight, 1, 1) * r1).sum(), [weight])
    (g2,) = torch.autograd.grad((conv_train.conv2d_nhwc(x2, weight, 1, 1) * r2).sum(), [weight])
    # two uses of one weight in one graph (the views of a step): autograd adds the two weight gradients
    ((conv_train.conv2d_nhwc(x1, weight, 1, 1) * r1).sum() + (conv_train.conv2d_nhwc(x2, weight, 1, 1) * r2).sum()).backward()
    assert torch.equal(weight.grad, g1 + g2) and bool((g1 != 0).any()) and not torch.equal(g1, g2)
    # x without requires_grad: no data gradient asked for, only dW came back
    assert x1.grad is None
    # an optimizer step bumps the parameter's version: the cached fp16 copies follow
    w16_before, _ = conv_train.weights.get(weight)
    y_before = conv_train.conv2d_nhwc(x1, weight, 1, 1).detach()
    torch.optim.SGD([weight], lr=0.5).step()
    w16_after, wt16_after = conv_train.weights.get(weight)
    assert not torch.equal(w16_before, w16_after) and torch.equal(w16_after, pack_conv_weight(weight))
    assert torch.equal(wt16_after, pack_conv_weight(weight.detach().flip(2, 3).permute(1, 0, 2, 3)))
    y_after = conv_train.conv2d_nhwc(x1, weight, 1, 1).detach()
    one, zero = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    assert torch.equal(y_after, ops.conv2d_f16(x1, w16_after, one, zero, 1, 1)) and not torch.equal(y_after, y_before)


def test_conv2d_nhwc_refuses_what_has_no_kernel():
    from hcir import HcirError, conv_train
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(HcirError):
        conv_train.conv2d_nhwc(x, torch.zeros(64, 64, 5, 5, device="cuda"), 1, 2)
    with pytest.raises(HcirError):
        conv_train.conv2d_nhwc(x, torch.zeros(64, 64, 3, 3, device="cuda").half(), 1, 1)
