"""Float64 restatements shared by tests/test_stem_train_host.py and tests/test_stem_train_gpu.py: the backward of the
stem's ReLU + max pool by torch autograd (the ground truth), and the selection rule of hcir_stem_pool_relu_bwd_f16
(include/hcir.h) written out position by position.  Test infrastructure, like tests/_fp64.py: no test lives here."""
import torch
import torch.nn.functional as F


def pool_inputs(b, hc, wc, seed):
    """c fp16-representable and quantised to multiples of 0.25 (ties are frequent), channels with positive, negative
    and zero gamma, dp of order 1: float64 NCHW tensors and [64] vectors.  s = rstd * gamma is the fp32 product the
    kernel forms, so its sign - and every channel with s == 0 - is the kernel's."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.randn(b, 64, hc, wc, generator=g) * 2).round() / 4      # sigma 0.5 in steps of 0.25
    gamma = torch.rand(64, generator=g) + 0.5
    gamma[1::3] *= -1.0
    gamma[[5, 17, 40]] = 0.0
    beta = 0.3 * torch.randn(64, generator=g)
    mean = 0.1 * torch.randn(64, generator=g)
    rstd = torch.rand(64, generator=g) + 0.5
    dp = torch.randn(b, 64, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, generator=g).half().float()
    assert torch.equal(c, c.half().float())
    return dict(c=c, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dp=dp)


def y64(i):
    s = (i["rstd"] * i["gamma"]).double().view(1, -1, 1, 1)
    return (i["c"].double() - i["mean"].double().view(1, -1, 1, 1)) * s + i["beta"].double().view(1, -1, 1, 1)


def g64_autograd(i):
    """d loss / d y of loss = sum(dp * max_pool2d(relu(y))) by torch autograd in float64 on the CPU."""
    y = y64(i).requires_grad_(True)
    F.max_pool2d(F.relu(y), 3, 2, 1).backward(i["dp"].double())
    return y.grad


def min_selected_abs_y(i):
    """min |y| over the windows' selected positions: the pooled maximum of y is the selected position's value."""
    return F.max_pool2d(y64(i), 3, 2, 1).abs().min().item()


def tied_fraction(i):
    """Fraction of (window, channel) whose extreme of c is attained at more than one position inside the map."""
    c = i["c"].double()
    s = (i["rstd"] * i["gamma"]).view(1, -1, 1, 1)
    key = torch.where(s > 0, c, torch.where(s < 0, -c, torch.zeros_like(c)))
    u = F.unfold(F.pad(key, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(c.shape[0], 64, 9, -1)
    return ((u == u.max(dim=2, keepdim=True).values).sum(dim=2) > 1).double().mean().item()


def g_rule(i):
    """The kernel's rule, restated: per window and channel the selected position is the first, in row-major order of
    the window, among the positions inside the map, with the maximal c where s > 0, the minimal c where s < 0, and
    simply the first where s == 0; it receives dp if y there is > 0."""
    c, dp = i["c"].double(), i["dp"].double()
    s = (i["rstd"] * i["gamma"]).double()
    y = y64(i)
    b, _, hc, wc = c.shape
    g = torch.zeros_like(c)
    for ph in range(dp.shape[2]):
        for pw in range(dp.shape[3]):
            pos = [(r, q) for r in range(2 * ph - 1, 2 * ph + 2) for q in range(2 * pw - 1, 2 * pw + 2)
                   if 0 <= r < hc and 0 <= q < wc]
            vals = torch.stack([c[:, :, r, q] for r, q in pos], dim=-1)            # [b, 64, positions]
            key = torch.where(s.view(1, -1, 1) > 0, vals, torch.where(s.view(1, -1, 1) < 0, -vals,
                                                                      torch.zeros_like(vals)))
            first = (key == key.max(dim=-1, keepdim=True).values).double().argmax(dim=-1)   # first maximal position
            for k, (r, q) in enumerate(pos):
                hit = (first == k) & (y[:, :, r, q] > 0)
                g[:, :, r, q] += torch.where(hit, dp[:, :, ph, pw], torch.zeros_like(dp[:, :, ph, pw]))
    return g
