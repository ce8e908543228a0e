"""The wiring of the ResNet body - resnet_engine's table run by conv_train.walk - against torch itself, on the CPU in
float64 with stand-in callables and no library call: conv = F.conv2d on the [B,C,H,W] view, norm = conv_train.torch_norm.
The walk and the trunk's own forward then run the same float64 operations and differ only in the order of the two-term
residual add, which is exact: 1e-12 relative holds with room, and anything larger is a wiring error.  Three mutations
of the table (a lost residual, a flipped ReLU, a conv fed from the wrong tensor) show that the comparison sees one:
each must miss the bound by at least 10^6."""
import copy
import dataclasses

import pytest
import torch
import torch.nn.functional as F
from torch import nn

B, SIZE, TOL = 2, 32, 1e-12


def _trunk(name):
    from hcir import _tv_resnet
    torch.manual_seed(11)
    net = getattr(_tv_resnet, name)(weights=None)
    return nn.Sequential(*list(net.children())[:-1]).double().train()


def _conv(a, sp):
    return F.conv2d(a.permute(0, 3, 1, 2), sp.conv.weight, None, sp.stride, sp.pad).permute(0, 2, 3, 1)


def _run(trunk, features, x, rmat):
    """features, {name: grad (zeros where the graph never reached the parameter)} and {name: buffer}."""
    f = features(x)
    (f * rmat).sum().backward()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in trunk.named_parameters()}
    return f.detach(), grads, dict(trunk.named_buffers())


def _walk_features(trunk, mutate=None):
    """train_trunk's frame (stem, NHWC, walk, pool) around the stand-in callables, over a table `mutate` may edit."""
    from hcir.conv_train import torch_norm, walk
    from hcir.resnet_engine import layer_table
    table = layer_table(trunk)
    if mutate is not None:
        mutate(table)
    kids = list(trunk.children())

    def features(x):
        a = kids[3](kids[2](kids[1](kids[0](x)))).permute(0, 2, 3, 1)
        return kids[8](walk(table, a, conv=_conv, norm=torch_norm).permute(0, 3, 1, 2)).flatten(1)
    return features


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _edit(name, **fields):
    def mutate(table):
        (i,) = [i for i, sp in enumerate(table) if sp.name == name]
        table[i] = dataclasses.replace(table[i], **fields)
    return mutate


_CASES = {}


def _case(name):
    """The trunk, its input and torch's own result, computed once per architecture."""
    if name not in _CASES:
        trunk = _trunk(name)
        gen = torch.Generator().manual_seed(12)
        x = torch.randn(B, 3, SIZE, SIZE, generator=gen, dtype=torch.float64)
        rmat = torch.randn(B, 512 if name == "resnet18" else 2048, generator=gen, dtype=torch.float64)
        ref = copy.deepcopy(trunk)
        _CASES[name] = (trunk, x, rmat, _run(ref, lambda t: ref(t).flatten(1), x, rmat))
    return _CASES[name]


def _worst(name, mutate=None):
    """Largest relative error of the walk against torch over the features and every parameter gradient, and the
    result of the walk."""
    trunk, x, rmat, (f0, g0, _) = _case(name)
    mine = copy.deepcopy(trunk)
    f, g, bufs = _run(mine, _walk_features(mine, mutate), x, rmat)
    assert set(g) == set(g0)
    return max([_rel(f, f0)] + [_rel(g[n], g0[n]) for n in g0]), bufs


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_walk_is_the_trunk(name):
    bufs0 = _case(name)[3][2]
    worst, bufs = _worst(name)
    print(f"{name}: walk vs trunk, worst relative error over features and gradients {worst:.3e}")
    assert worst <= TOL
    assert set(bufs) == set(bufs0) and any(n.endswith("running_var") for n in bufs)
    for n, b0 in bufs0.items():
        if n.endswith("num_batches_tracked"):
            assert int(bufs[n]) == int(b0) == 1, n
        else:
            assert _rel(bufs[n], b0) <= TOL, n


# the first block with a downsample branch: its input never has the output's shape (that is why the branch exists), so
# the residual cannot be rewired to "x" and is dropped instead
_LAST_OF_DOWNSAMPLE_BLOCK = {"resnet18": "layer2.0.conv2", "resnet50": "layer1.0.conv3"}


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
@pytest.mark.parametrize("mutation", ["residual_dropped", "relu_flipped_on_conv1", "conv2_fed_from_x"])
def test_a_wiring_error_is_seen(name, mutation):
    mutate = {"residual_dropped": _edit(_LAST_OF_DOWNSAMPLE_BLOCK[name], resid=None),
              "relu_flipped_on_conv1": _edit("layer1.0.conv1", relu=False),
              # layer1.0: the block's input, conv1's output and conv2's input all have 64 channels at stride 1
              "conv2_fed_from_x": _edit("layer1.0.conv2", inp="x")}[mutation]
    worst, _ = _worst(name, mutate)
    print(f"{name}, {mutation}: worst relative error {worst:.3e}")
    assert worst >= 1e6 * TOL


def test_an_edit_after_a_successful_walk_is_refused():
    """The table is built on every call: a conv swapped or edited in place after the trunk has been walked - same
    object, same number of modules - raises like a fresh trunk does."""
    from hcir._lib import HcirError
    from hcir.conv_train import train_trunk
    from hcir.resnet_engine import layer_table
    trunk = copy.deepcopy(_case("resnet18")[0])
    x = _case("resnet18")[1]
    _walk_features(trunk)(x)
    trunk[5][0].conv1.dilation = (2, 2)
    with pytest.raises(HcirError):
        layer_table(trunk)
    for fused in (False, True):                    # refused before the stem runs: nothing here needs a device
        with pytest.raises(HcirError):
            train_trunk(trunk.float(), x.float(), fused_norm=fused)
