"""The train-mode stem kernels (csrc/stem_train.hip, hcir_bn2d_stats_nhwc_f16) one by one, and stem_train end to end.

Every kernel is checked against float64 on the SAME fp16 / fp32 inputs the kernel sees, with a bound that is derived
and holds for every element; the printed figure is max err / bound.  Directly written buffers sit between canary rows.

  conv        |c - c64| <= 2^-11 |c64| + 2^-20 (|x16| * |w16|) + 2^-24: one fp16 store, fp32 accumulation of 147
              products (the stem bound of tests/test_conv_gpu.py)
  statistics  the kernels of hcir_bn2d_fwd_nhwc_f16: bit-equal to what that call returns
  pool        |p - p64| <= 2^-11 |p64| + 2^-21 max_window(|s| |c - mean| + |beta|) + 2^-24: one fp16 rounding, the
              fp32 evaluation of y (c - mean, s = rstd * gamma and the fma round once each: 3 * 2^-24 of the terms'
              sizes), and a max moves by at most the max of its arguments' moves
  pool bwd    |g - g64| <= 2^-10 |g64| + 2^-24, and g == 0 exactly where g64 == 0: an fp32 sum of at most four fp16
              terms rounded once; the selection is exact, the mask is unambiguous where |y64| >= 1e-4 (asserted on
              the inputs)
  wgrad       |dw - dw64| <= 2^-20 sum |dc| |x16| + 2^-24 (tests/test_conv_train_gpu.py's dw_bound); bit-equal twice

stem_train against a float64 CPU copy of the torch stem: e_hip <= max(2 e_ref, floor), e_ref = the torch stem under
autocast(fp16), floors 2^-11 (fp16 tensors) and 2^-20 (fp32 vectors) as in tests/test_bn2d_gpu.py."""
import copy
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stem_ref as ref  # noqa: E402
from _fp64 import rel  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 1234.0
SHAPES = [(1, 7, 7), (2, 9, 13), (2, 30, 23), (3, 33, 47), (4, 64, 64)]
FLOOR16, FLOOR32 = 2.0 ** -11, 2.0 ** -20


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _guarded(shape, dtype=torch.float16):
    """Output of `shape` (last dim = row) with one canary row in front and one behind; the canary also fills it."""
    row, n = shape[-1], math.prod(shape)
    buf = torch.full((n + 2 * row,), CANARY, dtype=dtype, device="cuda")
    return buf, buf[row:row + n].view(shape)


def _canaries_intact(buf, row):
    return bool((buf[:row] == CANARY).all()) and bool((buf[-row:] == CANARY).all())


def _sizes(h, w):
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return hc, wc, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1


def _nhwc(t, dtype=torch.float16):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def _nchw64(t):
    return t.cpu().double().permute(0, 3, 1, 2)


def _twice(run, shape, row, dtype=torch.float16):
    """`run(out)` twice into fresh guarded buffers: canaries intact, every element written, the two results equal."""
    outs = []
    for _ in range(2):
        buf, out = _guarded(shape, dtype)
        run(out)
        torch.cuda.synchronize()
        assert _canaries_intact(buf, row), "canary row overwritten"
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]), "two calls on the same input differ"
    assert torch.isfinite(outs[0]).all()
    return outs[0]


# ------------------------------------------------------------------ conv
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_stem_conv_vs_float64(b, h, w):
    from hcir import ops
    from hcir.resnet_engine import pack_stem_weight
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.randn(b, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147.0)
    x16, w16 = x.half().double(), wt.half().double()
    c64 = F.conv2d(x16, w16, None, 2, 3)
    bound = 2.0 ** -11 * c64.abs() + 2.0 ** -20 * F.conv2d(x16.abs(), w16.abs(), None, 2, 3) + 2.0 ** -24
    hc, wc, _, _ = _sizes(h, w)
    assert tuple(c64.shape) == (b, 64, hc, wc)
    xg, wp = x.cuda(), pack_stem_weight(wt).cuda()
    o = _nchw64(_twice(lambda out: ops.stem_conv(xg, wp, out=out), (b, hc, wc, 64), 64))
    ratio = ((o - c64).abs() / bound).max().item()
    print(f"stem conv {(b, h, w)} max err/bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_stats_are_the_forwards_bits(b, h, w):
    from hcir import ops
    hc, wc, _, _ = _sizes(h, w)
    g = torch.Generator().manual_seed(7 + h)
    c = (torch.randn(b, hc, wc, 64, generator=g) * 1.5 + 0.3).half().cuda()
    gamma, beta = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    rm0, rv0 = torch.randn(64, generator=g).cuda(), (torch.rand(64, generator=g) + 0.5).cuda()
    rm_a, rv_a, rm_b, rv_b = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    _, mean_a, rstd_a = ops.bn2d_fwd(c, gamma, beta, 1e-5, 0.1, None, False, rm_a, rv_a)
    mean_b, rstd_b = ops.bn2d_stats(c, 1e-5, 0.1, rm_b, rv_b)
    torch.cuda.synchronize()
    assert torch.equal(mean_a, mean_b) and torch.equal(rstd_a, rstd_b)
    assert torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b) and not torch.equal(rm_b, rm0)
    # ... and they are the batch's statistics
    c64 = c.cpu().double().view(-1, 64)
    assert rel(mean_b.cpu(), c64.mean(0)) <= 1e-5 and rel(rstd_b.cpu(), (c64.var(0, unbiased=False) + 1e-5).rsqrt()) <= 1e-5
    mean_c, rstd_c = ops.bn2d_stats(c, 1e-5, 0.1)            # without running statistics
    assert torch.equal(mean_c, mean_b) and torch.equal(rstd_c, rstd_b)


# ------------------------------------------------------------------ normalise + ReLU + pool
def _pool_case(b, h, w, gamma, beta, seed):
    from hcir import ops
    hc, wc, hp, wp = _sizes(h, w)
    g = torch.Generator().manual_seed(seed)
    c = (torch.randn(b, 64, hc, wc, generator=g) * 1.5 + 0.3).half()
    mean, rstd = 0.3 + 0.1 * torch.randn(64, generator=g), torch.rand(64, generator=g) + 0.4
    s = (rstd * gamma).double().view(1, -1, 1, 1)                 # the fp32 product the kernel forms
    d = c.double() - mean.double().view(1, -1, 1, 1)
    y = d * s + beta.double().view(1, -1, 1, 1)
    p64 = F.max_pool2d(F.relu(y), 3, 2, 1)                        # pads with -inf: padding never wins
    e = s.abs() * d.abs() + beta.double().abs().view(1, -1, 1, 1)
    bound = 2.0 ** -11 * p64.abs() + 2.0 ** -21 * F.max_pool2d(e, 3, 2, 1) + 2.0 ** -24
    cg = _nhwc(c)
    args = [t.cuda() for t in (gamma, beta, mean, rstd)]
    o = _nchw64(_twice(lambda out: ops.stem_bn_relu_pool(cg, *args, out=out), (b, hp, wp, 64), 64))
    return o, p64, ((o - p64).abs() / bound).max().item(), y


@pytest.mark.parametrize("b,h,w", SHAPES)
def test_bn_relu_pool_vs_float64(b, h, w):
    g = torch.Generator().manual_seed(h + w)
    gamma = (torch.rand(64, generator=g) + 0.5) * torch.where(torch.rand(64, generator=g) < 0.3, -1.0, 1.0)
    beta = 0.5 * torch.randn(64, generator=g)
    o, p64, ratio, _ = _pool_case(b, h, w, gamma, beta, seed=h * 100 + w)
    print(f"stem pool {(b, h, w)} max err/bound {ratio:.3f}")
    assert (p64 > 0).any() and ratio <= 1.0


def test_bn_relu_pool_zero_gamma_gives_beta():
    """gamma = 0, beta > 0: y = fma(c - mean, 0, beta) = beta at every position, the border windows included."""
    beta = torch.rand(64, generator=torch.Generator().manual_seed(0)) + 0.1
    o, p64, ratio, _ = _pool_case(2, 30, 23, torch.zeros(64), beta, seed=5)
    assert ratio <= 1.0
    assert torch.equal(o, beta.half().double().view(1, -1, 1, 1).expand_as(o))


def test_bn_relu_pool_all_negative_gives_exact_zero():
    """Every y < 0: the output is exactly 0 everywhere - the ReLU's zero, with nothing of the padding (excluded from
    the max, held as -inf) leaking through at the windows that hang over the edges."""
    g = torch.Generator().manual_seed(1)
    gamma, beta = 0.01 * torch.randn(64, generator=g), -1.0 - torch.rand(64, generator=g)
    o, p64, ratio, y = _pool_case(2, 30, 23, gamma, beta, seed=6)
    assert y.max() < 0 and bool((p64 == 0).all())
    assert bool((o == 0).all()) and ratio <= 1.0


# ------------------------------------------------------------------ pool + ReLU backward
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_pool_relu_bwd_vs_float64_autograd(b, h, w):
    from hcir import ops
    hc, wc, hp, wp = _sizes(h, w)
    i = ref.pool_inputs(b, hc, wc, seed=3)
    # preconditions on the INPUTS: ties are frequent, and no selected position has y so close to 0 that fp32 and
    # float64 could disagree about the mask
    tied, ymin = ref.tied_fraction(i), ref.min_selected_abs_y(i)
    assert tied > 0.2 and ymin >= 1e-4
    g64 = ref.g64_autograd(i)
    vec = [i[k].cuda() for k in ("gamma", "beta", "mean", "rstd")]
    dp, c = _nhwc(i["dp"]), _nhwc(i["c"])
    o = _nchw64(_twice(lambda out: ops.stem_pool_relu_bwd(dp, c, *vec, out=out), (b, hc, wc, 64), 64))
    ratio = ((o - g64).abs() / (2.0 ** -10 * g64.abs() + 2.0 ** -24)).max().item()
    print(f"stem pool bwd {(b, h, w)}: tied windows {tied:.3f}, min |y| selected {ymin:.4f}, max err/bound {ratio:.3f}")
    assert (g64 != 0).any() and ratio <= 1.0
    assert bool((o[g64 == 0] == 0).all())


# ------------------------------------------------------------------ weight gradient
def _wgrad_case(b, h, w):
    from hcir import ops
    hc, wc, _, _ = _sizes(h, w)
    g = torch.Generator().manual_seed(b * 10000 + h * 100 + w)
    x = torch.randn(b, 3, h, w, generator=g)
    dc = torch.randn(b, 64, hc, wc, generator=g).half()
    x16, dc64 = x.half().double(), dc.double()
    dw64 = torch.nn.grad.conv2d_weight(x16, (64, 3, 7, 7), dc64, stride=2, padding=3)
    bound = 2.0 ** -20 * torch.nn.grad.conv2d_weight(x16.abs(), (64, 3, 7, 7), dc64.abs(), stride=2, padding=3) \
        + 2.0 ** -24
    xg, dcg = x.cuda(), _nhwc(dc)
    o = _twice(lambda out: ops.stem_wgrad(xg, dcg, out=out.view(64, 3, 7, 7)), (64, 147), 147, torch.float32)
    ratio = ((o.cpu().double().view(64, 3, 7, 7) - dw64).abs() / bound).max().item()
    print(f"stem wgrad {(b, h, w)} parts {ops.stem_wgrad_parts(b, h, w)} max err/bound {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("b,h,w", SHAPES)
def test_stem_wgrad_vs_float64(b, h, w):
    assert _wgrad_case(b, h, w) <= 1.0


def test_stem_wgrad_one_part_and_ragged_last_part():
    from hcir import ops
    assert ops.stem_wgrad_parts(1, 7, 7) == 1 and ops.stem_wgrad_parts(2, 30, 23) == 1    # run above: one part
    # 5 conv tiles at 4 a part: the smallest shape with several parts and a last part that holds fewer
    assert ops.stem_wgrad_parts(5, 7, 7) == 2 and ops.stem_wgrad_parts(4, 7, 7) == 1
    assert _wgrad_case(5, 7, 7) <= 1.0
    # ... and one whose tiles differ in size as well: 3 x 2 x 3 = 18 tiles, 4 + 4 + 4 + 4 + 2
    assert ops.stem_wgrad_parts(3, 33, 65) == 5
    assert _wgrad_case(3, 33, 65) <= 1.0


def test_wrappers_reject_what_the_kernels_cannot_take():
    from hcir import HcirError, ops
    from hcir.resnet_engine import pack_stem_weight
    wp = pack_stem_weight(torch.zeros(64, 3, 7, 7)).cuda()
    with pytest.raises(HcirError, match="status -2"):
        ops.stem_conv(torch.zeros(1, 3, 6, 9, device="cuda"), wp)
    with pytest.raises(HcirError):
        ops.stem_conv(torch.zeros(1, 3, 9, 9), wp)                                   # a CPU tensor
    with pytest.raises(HcirError):
        ops.stem_wgrad(torch.zeros(1, 3, 9, 9, device="cuda"), torch.zeros(1, 4, 5, 64, dtype=torch.float16, device="cuda"))
    v = torch.zeros(64, device="cuda")
    with pytest.raises(HcirError):
        ops.stem_bn_relu_pool(torch.zeros(1, 5, 5, 128, dtype=torch.float16, device="cuda"), v, v, v, v)


# ------------------------------------------------------------------ stem_train end to end
def _stem_modules(seed=11):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    bn = torch.nn.BatchNorm2d(64)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(64, generator=g) + 0.5)
        bn.bias.copy_(0.2 * torch.randn(64, generator=g))
    return conv.train(), bn.train()


def _run_stem(forward, conv, bn, x, rmat):
    for p in (conv.weight, bn.weight, bn.bias):
        p.grad = None
    p = forward(x)
    (p.double() * rmat.to(p.device)).sum().backward()
    return {"p": p.detach().cpu().double(), "dw": conv.weight.grad.cpu().double(),
            "dgamma": bn.weight.grad.cpu().double(), "dbeta": bn.bias.grad.cpu().double(),
            "running_mean": bn.running_mean.detach().cpu().double(),
            "running_var": bn.running_var.detach().cpu().double()}


def test_stem_train_vs_float64_and_autocast():
    from hcir import conv_train
    b, h, w = 4, 64, 64
    conv, bn = _stem_modules()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(b, 3, h, w, generator=gen)
    rmat = torch.randn(b, 64, 16, 16, generator=gen).double()
    pool = torch.nn.MaxPool2d(3, 2, 1)

    c64, b64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    G = _run_stem(lambda t: pool(F.relu(b64(c64(t)))), c64, b64, x.double(), rmat)

    cr, br = copy.deepcopy(conv).cuda(), copy.deepcopy(bn).cuda()

    def autocast_stem(t):
        with torch.autocast("cuda", dtype=torch.float16):
            return pool(F.relu(br(cr(t))))

    REF = _run_stem(autocast_stem, cr, br, x.cuda(), rmat)

    ch, bh = copy.deepcopy(conv).cuda(), copy.deepcopy(bn).cuda()

    def hip_stem(t):
        p = conv_train.stem_train(t, ch, bh)
        assert p.dtype == torch.float16 and tuple(p.shape) == (b, 16, 16, 64) and p.is_contiguous()
        return p.permute(0, 3, 1, 2)

    HIP = _run_stem(hip_stem, ch, bh, x.cuda(), rmat)
    assert int(bh.num_batches_tracked) == 1
    for k in G:
        e_ref, e_hip, floor = rel(REF[k], G[k]), rel(HIP[k], G[k]), FLOOR16 if k == "p" else FLOOR32
        print(f"stem_train {k}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    for k in G:
        e_ref, e_hip, floor = rel(REF[k], G[k]), rel(HIP[k], G[k]), FLOOR16 if k == "p" else FLOOR32
        assert e_hip <= max(2.0 * e_ref, floor), f"{k}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, floor {floor:.3e}"

    # a second backward accumulates into .grad (same input, statistics from the same batch: the same gradient again)
    g1 = {n: p.grad.clone() for n, p in (("w", ch.weight), ("g", bh.weight), ("b", bh.bias))}
    (hip_stem(x.cuda()).double() * rmat.cuda()).sum().backward()
    assert int(bh.num_batches_tracked) == 2
    for n, p in (("w", ch.weight), ("g", bh.weight), ("b", bh.bias)):
        assert torch.equal(p.grad, g1[n] + g1[n]), n

    # the packed weight follows an optimizer step
    (wp0,) = conv_train.stem_weights.get(ch.weight)
    assert conv_train.stem_weights.get(ch.weight)[0] is wp0
    torch.optim.SGD([ch.weight], lr=0.1).step()
    (wp1,) = conv_train.stem_weights.get(ch.weight)
    from hcir.resnet_engine import pack_stem_weight
    assert wp1 is not wp0 and not torch.equal(wp1, wp0) and torch.equal(wp1, pack_stem_weight(ch.weight))
    with torch.no_grad():
        p_new = conv_train.stem_train(x.cuda(), ch, bh)
    assert not torch.equal(p_new, HIP["p"].permute(0, 2, 3, 1).half().cuda())


def test_stem_train_rejects_what_it_cannot_serve():
    from hcir import HcirError, conv_train
    conv, bn = _stem_modules()
    conv, bn = conv.cuda(), bn.cuda()
    x = torch.randn(2, 3, 32, 32, device="cuda")
    with pytest.raises(HcirError):
        conv_train.stem_train(x, conv, bn.eval())
    bn.train()
    with pytest.raises(HcirError):
        conv_train.stem_train(x, conv, torch.nn.BatchNorm2d(64, momentum=None).cuda())
    with pytest.raises(HcirError):
        conv_train.stem_train(x.clone().requires_grad_(True), conv, bn)
    assert int(bn.num_batches_tracked) == 0
