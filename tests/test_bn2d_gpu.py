"""The batch-statistics BatchNorm2d (+ residual) (+ ReLU) kernels (csrc/bn2d.hip) and bn_act_nhwc against a float64
ground truth.

Ground truth G: F.batch_norm(training=True) (+ resid) (+ ReLU) and its autograd in float64 on the CPU, from
fp16-representable inputs.  e_ref = the error against G (tests/_fp64.rel) of torch itself on the GPU doing the same on
the same fp16 channels_last tensors with fp32 parameters; e_hip = ours.  The project's criterion,

    e_hip <= max(2 e_ref, floor)

with floors that are derived, not measured: 2^-11 for tensors stored in fp16 (y, dx, dresid: one fp16 rounding) and
2^-20 for fp32 vectors (save_mean, save_rstd, running statistics, dgamma, dbeta: 16 fp32 ulps over a vector norm).
Every pair is printed; the recorded values are in profiles/bn2d_errors.txt and DESIGN.md §3.4.

G1 to G5 run small maps (at most 4 passes per chunk, one apply trip, one chunk per finalize lane); G6 keeps this
end-to-end comparison at the plans a training batch runs.  A norm over 10^5 to 10^7 elements does not see a wrong or
unwritten row: tests/test_bn2d_elements_gpu.py holds every element and channel."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fp64 import rel  # noqa: E402

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
FLOOR16, FLOOR32 = 2.0 ** -11, 2.0 ** -20
F16_NAMES = ("y", "dx", "dresid", "input")


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


def _inputs(shape, seed, large_mean=False, random_buffers=False):
    g = torch.Generator().manual_seed(seed)
    c = shape[3]
    x = torch.randn(shape, generator=g)
    if large_mean:
        x = 100.0 + 0.25 * x
    d = dict(x=x.half(), resid=torch.randn(shape, generator=g).half(), dy=torch.randn(shape, generator=g).half(),
             gamma=torch.rand(c, generator=g) + 0.5, beta=0.2 * torch.randn(c, generator=g),
             rm=torch.zeros(c), rv=torch.ones(c))
    if random_buffers:
        d["rm"], d["rv"] = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return d


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _torch_run(inp, relu, resid, device, dtype):
    """F.batch_norm (+ resid) (+ ReLU) and autograd: float64 on the CPU (G), or the activations' own fp16 with fp32
    parameters on the GPU (the reference: channels_last tensors, as the trunk holds them)."""
    act = torch.float64 if dtype == torch.float64 else torch.float16
    par = torch.float64 if dtype == torch.float64 else torch.float32
    x = _nchw(inp["x"].to(device, act)).detach().requires_grad_(True)
    r = _nchw(inp["resid"].to(device, act)).detach().requires_grad_(True)
    w = inp["gamma"].to(device, par).requires_grad_(True)
    b = inp["beta"].to(device, par).requires_grad_(True)
    rm, rv = inp["rm"].to(device, par).clone(), inp["rv"].to(device, par).clone()
    # torch's own batch-norm kernels for every shape: with the vendor library enabled the dispatcher would hand it the
    # tensors that are NCHW-contiguous as well (the 1 x 1 maps) and keep the channels_last ones, two references in one
    # table
    with torch.backends.cudnn.flags(enabled=False):
        out = F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS)
        if resid:
            out = out + r
        if relu:
            out = F.relu(out)
        out.backward(_nchw(inp["dy"].to(device, act)))
    res = dict(y=out.detach().permute(0, 2, 3, 1), running_mean=rm, running_var=rv,
               dx=x.grad.permute(0, 2, 3, 1), dgamma=w.grad, dbeta=b.grad)
    if resid:
        res["dresid"] = r.grad.permute(0, 2, 3, 1)
    if dtype == torch.float64:
        x64 = inp["x"].double()
        res["save_mean"] = x64.mean(dim=(0, 1, 2))
        res["save_rstd"] = 1.0 / torch.sqrt(x64.var(dim=(0, 1, 2), unbiased=False) + EPS)
    else:           # the statistics torch's kernels save for the backward
        _, res["save_mean"], res["save_rstd"] = torch.native_batch_norm(
            x.detach(), w.detach(), b.detach(), rm.clone(), rv.clone(), True, MOMENTUM, EPS)
    return {k: v.detach().cpu().double() for k, v in res.items()}


def _hip_run(inp, relu, resid):
    from hcir import ops
    dev = "cuda"
    x, r, dy = inp["x"].to(dev), (inp["resid"].to(dev) if resid else None), inp["dy"].to(dev)
    gamma, beta = inp["gamma"].to(dev), inp["beta"].to(dev)
    rm, rv = inp["rm"].to(dev).clone(), inp["rv"].to(dev).clone()
    y, mean, rstd = ops.bn2d_fwd(x, gamma, beta, EPS, MOMENTUM, r, relu, rm, rv)
    dx, dresid, dgamma, dbeta = ops.bn2d_bwd(dy, x, y if relu else None, gamma, mean, rstd, want_dresid=resid)
    assert y.dtype == dx.dtype == torch.float16 and mean.dtype == rstd.dtype == dgamma.dtype == torch.float32
    res = dict(y=y, save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma,
               dbeta=dbeta)
    if resid:
        res["dresid"] = dresid
    return {k: v.detach().cpu().double() for k, v in res.items()}


def _hold(tag, G, REF, HIP):
    """Print every e_ref / e_hip pair, then assert the criterion for each."""
    assert set(HIP) == set(G) == set(REF)
    rows = []
    for k in sorted(G):
        assert torch.isfinite(HIP[k]).all(), k
        floor = FLOOR16 if k in F16_NAMES else FLOOR32
        rows.append((k, rel(REF[k], G[k]), rel(HIP[k], G[k]), floor))
        print(f"{tag} {k}: e_ref {rows[-1][1]:.3e} e_hip {rows[-1][2]:.3e}")
    for k, e_ref, e_hip, floor in rows:
        assert e_hip <= max(2.0 * e_ref, floor), f"{tag} {k}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, floor {floor:.3e}"


def _case(shape, relu, resid, seed, **kw):
    inp = _inputs(shape, seed, **kw)
    return (_torch_run(inp, relu, resid, "cpu", torch.float64), _torch_run(inp, relu, resid, "cuda", torch.float16),
            _hip_run(inp, relu, resid))


def _plan_c64(m):
    """csrc/bn2d_plan.h restated for C = 64 (a wavefront covers 8 rows, a workgroup 32 per pass): (chunks, rows per
    chunk)."""
    passes = -(-m // 32)
    chunks = min(-(-passes // 4), 2048)
    rows = -(-passes // chunks) * 32
    return -(-m // rows), rows


G1_SHAPES = [(2, 1, 1, 64),        # M = 2: the smallest legal
             (3, 5, 5, 64),        # M = 75: ragged against the 8 rows of a wavefront and the 32 of a pass
             (4, 7, 7, 2048),      # the widest C: a row is four wavefronts' work
             (4, 14, 14, 256),
             (3, 28, 28, 128)]
G3_SHAPE = (4, 14, 14, 64)
G4_SAME_BITS_SHAPES = [(1, 56, 56, 64), (4, 7, 7, 2048)]
G4_MASK_SHAPES = [(3, 5, 5, 64), (4, 14, 14, 256)]
G4_BUFFERS_SHAPE = (4, 14, 14, 256)
G4_RUNNING_SHAPE = (3, 5, 5, 64)
G5_SHAPE = (4, 14, 14, 256)
G5_SHORTCUT_SHAPE = (4, 14, 14, 64)
G6_SHAPES = [(61, 13, 13, 2048), (3, 67, 67, 320)]


def _g2_pick():
    """the smallest B x 56 x 56 x 64 map with at least 3 chunks and a ragged last one: (B, M, chunks, rows per chunk)"""
    for b in range(1, 9):
        m = b * 56 * 56
        chunks, rows = _plan_c64(m)
        if chunks >= 3 and m % rows != 0:
            return b, m, chunks, rows
    return None


def small_map_shapes():
    """every shape G1 to G5 run (tests/test_bn2d_host.py asserts that they all take the small-map branch of the plan)"""
    return (G1_SHAPES + [(_g2_pick()[0], 56, 56, 64), G3_SHAPE, G4_BUFFERS_SHAPE, G4_RUNNING_SHAPE, G5_SHAPE,
                         G5_SHORTCUT_SHAPE] + G4_SAME_BITS_SHAPES + G4_MASK_SHAPES)


@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", G1_SHAPES)
def test_g1_shapes_vs_float64(shape, relu, resid):
    _hold(f"G1 {shape} relu={int(relu)} resid={int(resid)}", *_case(shape, relu, resid, seed=11))


def test_g2_several_chunks_with_a_ragged_last_one():
    from hcir import ops
    pick = _g2_pick()
    assert pick is not None
    b, m, chunks, rows = pick
    assert ops.bn2d_chunks(m, 64) == chunks >= 3 and m - (chunks - 1) * rows < rows     # the plan the kernel ran
    assert ops.bn2d_chunks(2, 64) == 1                                                  # ... and G1's smallest case
    print(f"G2: B = {b}, M = {m}: {chunks} chunks of {rows} rows, the last {m - (chunks - 1) * rows}")
    _hold(f"G2 {(b, 56, 56, 64)} relu=1 resid=1", *_case((b, 56, 56, 64), True, True, seed=12))


def test_g3_large_mean():
    """x = 100 + 0.25 randn: sum x^2 - (sum x)^2 / n in fp32 loses mean^2 / var = 1.6e5 of its 1.7e7, the variance
    would be off by percents; save_rstd and running_var are held to the same criterion as everything else."""
    shape = G3_SHAPE
    G, REF, HIP = _case(shape, False, False, seed=13, large_mean=True)
    assert abs(G["save_mean"].mean().item() - 100.0) < 0.1 and abs(G["save_rstd"].mean().item() - 4.0) < 0.5
    _hold(f"G3 {shape} mean=100", G, REF, HIP)


def test_g4_two_calls_same_bits():
    from hcir import ops
    for shape in G4_SAME_BITS_SHAPES:
        inp = {k: v.cuda() for k, v in _inputs(shape, seed=14).items()}
        outs = []
        for _ in range(2):
            rm, rv = inp["rm"].clone(), inp["rv"].clone()
            f = ops.bn2d_fwd(inp["x"], inp["gamma"], inp["beta"], EPS, MOMENTUM, inp["resid"], True, rm, rv)
            bw = ops.bn2d_bwd(inp["dy"], inp["x"], f[0], inp["gamma"], f[1], f[2], want_dresid=True)
            outs.append((*f, rm, rv, *bw))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


def test_g4_relu_mask_and_residual_gradient_exact():
    from hcir import ops
    for shape in G4_MASK_SHAPES:
        inp = {k: v.cuda() for k, v in _inputs(shape, seed=15).items()}
        y, mean, rstd = ops.bn2d_fwd(inp["x"], inp["gamma"], inp["beta"], EPS, MOMENTUM, inp["resid"], True)
        assert (y >= 0).all() and (y == 0).any() and (y > 0).any()
        _, dresid, _, _ = ops.bn2d_bwd(inp["dy"], inp["x"], y, inp["gamma"], mean, rstd, want_dresid=True)
        assert torch.equal(dresid, torch.where(y > 0, inp["dy"], torch.zeros_like(inp["dy"])))
        # without the ReLU the residual branch's gradient is dy itself
        y2, mean2, rstd2 = ops.bn2d_fwd(inp["x"], inp["gamma"], inp["beta"], EPS, MOMENTUM, inp["resid"], False)
        _, dresid2, _, _ = ops.bn2d_bwd(inp["dy"], inp["x"], None, inp["gamma"], mean2, rstd2, want_dresid=True)
        assert torch.equal(dresid2, inp["dy"])
        assert torch.equal(torch.relu(y2), y)             # the ReLU is a clamp of the same rounded value


def test_g4_without_running_buffers():
    from hcir import ops
    inp = {k: v.cuda() for k, v in _inputs(G4_BUFFERS_SHAPE, seed=16).items()}
    rm, rv = inp["rm"].clone(), inp["rv"].clone()
    y0, mean0, rstd0 = ops.bn2d_fwd(inp["x"], inp["gamma"], inp["beta"], EPS, MOMENTUM, None, False, rm, rv)
    y1, mean1, rstd1 = ops.bn2d_fwd(inp["x"], inp["gamma"], inp["beta"], EPS, MOMENTUM, None, False, None, None)
    assert torch.equal(y0, y1) and torch.equal(mean0, mean1) and torch.equal(rstd0, rstd1)
    assert not torch.equal(rm, inp["rm"]) and not torch.equal(rv, inp["rv"])


@pytest.mark.parametrize("random_buffers", [False, True])
def test_g4_running_statistics_move_toward_the_unbiased_variance(random_buffers):
    shape = G4_RUNNING_SHAPE    # M = 75: M / (M - 1) = 1.0135, far outside the criterion if the biased variance is used
    inp = _inputs(shape, seed=17, random_buffers=random_buffers)
    G, REF, HIP = (_torch_run(inp, False, False, "cpu", torch.float64),
                   _torch_run(inp, False, False, "cuda", torch.float16), _hip_run(inp, False, False))
    x64 = inp["x"].double()
    want_var = (1 - MOMENTUM) * inp["rv"].double() + MOMENTUM * x64.var(dim=(0, 1, 2), unbiased=True)
    want_mean = (1 - MOMENTUM) * inp["rm"].double() + MOMENTUM * x64.mean(dim=(0, 1, 2))
    assert rel(G["running_var"], want_var) < 1e-12 and rel(G["running_mean"], want_mean) < 1e-12
    for k in ("running_mean", "running_var"):
        e_ref, e_hip = rel(REF[k], G[k]), rel(HIP[k], G[k])
        print(f"G4 running random_buffers={int(random_buffers)} {k}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
        assert e_hip <= max(2.0 * e_ref, FLOOR32)


def _bn(c, inp):
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"])
        bn.bias.copy_(inp["beta"])
    return bn.cuda().train()


def test_g5_bn_act_autograd():
    from hcir.conv_train import bn_act_nhwc
    shape = G5_SHAPE
    inp = _inputs(shape, seed=18)
    G, REF = _torch_run(inp, True, True, "cpu", torch.float64), _torch_run(inp, True, True, "cuda", torch.float16)
    bn = _bn(shape[3], inp)
    x = inp["x"].cuda().requires_grad_(True)
    r = inp["resid"].cuda().requires_grad_(True)
    y = bn_act_nhwc(x, bn, resid=r, relu=True)
    assert y.requires_grad and y.dtype == torch.float16 and tuple(y.shape) == shape
    y.backward(inp["dy"].cuda())
    assert int(bn.num_batches_tracked) == 1
    HIP = dict(y=y, dx=x.grad, dresid=r.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
               running_var=bn.running_var)
    HIP = {k: v.detach().cpu().double() for k, v in HIP.items()}
    keep = set(HIP)
    _hold(f"G5 bn_act_nhwc {shape}", {k: G[k] for k in keep}, {k: REF[k] for k in keep}, HIP)


def test_g5_identity_shortcut_sums_both_gradients():
    """relu(bn(conv(a)) + a): `a` feeds the convolution and is the residual, the wiring of a BasicBlock without a
    downsample branch; autograd adds the convolution's data gradient and the residual branch's."""
    from hcir.conv_train import bn_act_nhwc, conv2d_nhwc
    shape = G5_SHORTCUT_SHAPE
    inp = _inputs(shape, seed=19)
    w = (torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(20)) / 24.0).half().float()

    def torch_path(device, dtype):
        act = torch.float64 if dtype == torch.float64 else torch.float16
        par = torch.float64 if dtype == torch.float64 else torch.float32
        a = _nchw(inp["x"].to(device, act)).detach().requires_grad_(True)
        wt = w.to(device, par).requires_grad_(True)
        g, b = inp["gamma"].to(device, par).requires_grad_(True), inp["beta"].to(device, par).requires_grad_(True)
        rm, rv = inp["rm"].to(device, par).clone(), inp["rv"].to(device, par).clone()
        conv = F.conv2d(a, wt.to(act), padding=1)
        out = F.relu(F.batch_norm(conv, rm, rv, g, b, True, MOMENTUM, EPS) + a)
        out.backward(_nchw(inp["dy"].to(device, act)))
        res = dict(y=out.permute(0, 2, 3, 1), input=a.grad.permute(0, 2, 3, 1))
        return {k: v.detach().cpu().double() for k, v in res.items()}

    G, REF = torch_path("cpu", torch.float64), torch_path("cuda", torch.float16)
    bn = _bn(64, inp)
    a = inp["x"].cuda().requires_grad_(True)
    wt = w.cuda().requires_grad_(True)
    out = bn_act_nhwc(conv2d_nhwc(a, wt, 1, 1), bn, resid=a, relu=True)
    out.backward(inp["dy"].cuda())
    assert wt.grad is not None and bn.weight.grad is not None and bn.bias.grad is not None
    HIP = dict(y=out, input=a.grad)
    HIP = {k: v.detach().cpu().double() for k, v in HIP.items()}
    # the residual branch alone would give where(y > 0, dy, 0): the sum must differ from it by the data gradient
    alone = torch.where(HIP["y"] > 0, inp["dy"].double(), torch.zeros(()).double())
    assert rel(HIP["input"], alone) > 0.1
    _hold(f"G5 shortcut {shape}", G, REF, HIP)


@pytest.mark.parametrize("shape", G6_SHAPES, ids=str)
def test_g6_capped_and_strided_plans(shape):
    """The same end-to-end criterion against torch's kernels at the plans a training batch runs: the chunk count
    clamped by the grid cap with 6 passes per chunk and 6 apply trips, and 2 apply trips over 5 channel slabs; both
    with several chunks per finalize lane (tests/test_bn2d_elements_gpu.py holds every element of these shapes)."""
    from hcir import ops
    from oracle import bn2d as ob
    m, c = ob.rows_of(shape), shape[3]
    p = ob.plan(m, c)
    assert ops.bn2d_chunks(m, c) == p.chunks and p.per >= 2 and p.trips >= 2
    assert (p.clamped, p.chunk_passes, p.trips, p.slabs) == ((True, 6, 6, 4) if c == 2048 else (False, 4, 2, 5))
    _hold(f"G6 {shape} relu=1 resid=1", *_case(shape, True, True, seed=21))
