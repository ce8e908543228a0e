"""Host side of hcir.resnet_engine: BatchNorm folding, weight packing, the layer table against the module tree,
output-size arithmetic, and the unsupported-shape answer of hcir_conv2d_f16 - none of it needs a device."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn


def _trunk(name):
    from hcir import _tv_resnet
    net = getattr(_tv_resnet, name)(weights=None)
    return nn.Sequential(*list(net.children())[:-1]).eval()


@pytest.mark.parametrize("var", [None, 1e-6])
def test_fold_bn_matches_batch_norm_eval(var):
    from hcir.resnet_engine import fold_bn
    g = torch.Generator().manual_seed(3)
    c = 96
    bn = nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g))
        bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5 if var is None else torch.full((c,), var))
    scale, bias = fold_bn(bn)
    assert scale.dtype == torch.float32 and bias.dtype == torch.float32
    x = torch.randn(4, c, 5, 3, generator=g, dtype=torch.float64)
    ref = F.batch_norm(x, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(),
                       False, 0.1, bn.eps)
    got = x * scale.double().view(1, c, 1, 1) + bias.double().view(1, c, 1, 1)
    # scale and bias are each one fp32 rounding of the float64 value: 2^-24 relative on either term
    bound = 2.0 ** -23 * (x.abs() * scale.double().abs().view(1, c, 1, 1) + bias.double().abs().view(1, c, 1, 1))
    assert bool(((got - ref).abs() <= bound + 1e-30).all())
    if var is not None:   # gamma / sqrt(1e-6 + 1e-5) ~ 300 gamma: finite in fp32, and the reason scale stays out of fp16 weights
        assert torch.isfinite(scale).all() and scale.abs().max() > 100


def test_pack_conv_weight_round_trip():
    from hcir.resnet_engine import pack_conv_weight, unpack_conv_weight
    w = torch.randn(128, 64, 3, 3, generator=torch.Generator().manual_seed(0))
    p = pack_conv_weight(w)
    assert p.dtype == torch.float16 and tuple(p.shape) == (128, 3, 3, 64) and p.is_contiguous()
    assert torch.equal(unpack_conv_weight(p), w.half())
    assert p[5, 2, 1, 7] == w[5, 7, 2, 1].half()


def test_pack_stem_weight_fragment_order():
    from hcir.resnet_engine import pack_stem_weight
    w = torch.randn(64, 3, 7, 7, generator=torch.Generator().manual_seed(1))
    p = pack_stem_weight(w)
    assert p.dtype == torch.float16 and tuple(p.shape) == (10, 2, 64, 8)
    flat = w.half().reshape(64, 147)
    for kk, nt, lane, j in [(0, 0, 0, 0), (3, 1, 37, 5), (9, 0, 31, 2), (9, 1, 63, 7), (9, 0, 0, 3)]:
        k = 16 * kk + 8 * (lane >> 5) + j
        want = flat[nt * 32 + (lane & 31), k] if k < 147 else torch.tensor(0.0, dtype=torch.float16)
        assert p[kk, nt, lane, j] == want
    assert int((p != 0).sum()) == int((flat != 0).sum())
    with pytest.raises(Exception):
        pack_stem_weight(torch.zeros(64, 3, 3, 3))


@pytest.mark.parametrize("name,nconv", [("resnet18", 19), ("resnet50", 52)])
def test_layer_table_matches_module_tree(name, nconv):
    from hcir.resnet_engine import layer_table
    trunk = _trunk(name)
    table = layer_table(trunk)
    convs = [(n, m) for n, m in trunk.named_modules() if isinstance(m, nn.Conv2d)]
    assert len(convs) == nconv + 1 and len(table) == nconv        # the stem has a kernel of its own
    by_module = {id(sp.conv): sp for sp in table}
    assert len(by_module) == nconv
    for n, m in convs[1:]:
        sp = by_module[id(m)]
        assert (sp.r, sp.stride, sp.pad, sp.cin, sp.cout) == (m.kernel_size[0], m.stride[0], m.padding[0],
                                                              m.in_channels, m.out_channels), n
    kids = list(trunk.children())
    pos = {id(sp.conv): i for i, sp in enumerate(table)}
    for li, layer in enumerate(kids[4:8], start=1):
        for bi, blk in enumerate(layer):
            last = blk.conv3 if hasattr(blk, "conv3") else blk.conv2
            inner = [blk.conv1] + ([blk.conv2] if hasattr(blk, "conv3") else [])
            sp = by_module[id(last)]
            # the block's last conv carries the residual and the single ReLU after the add
            assert sp.relu and sp.out == "y" and sp.resid == ("ds" if blk.downsample is not None else "x")
            assert sp.bn is (blk.bn3 if hasattr(blk, "conv3") else blk.bn2)
            for c in inner:
                assert by_module[id(c)].resid is None and by_module[id(c)].relu
                assert pos[id(c)] < pos[id(last)]
            if blk.downsample is not None:
                ds = by_module[id(blk.downsample[0])]
                assert ds.out == "ds" and not ds.relu and ds.resid is None and ds.r == 1 and ds.inp == "x"
                assert ds.bn is blk.downsample[1] and pos[id(blk.downsample[0])] < pos[id(last)]
                assert ds.stride == (1 if li == 1 else 2)
            assert sp.group == f"layer{li}"
    assert sum(sp.resid is not None for sp in table) == sum(len(l) for l in kids[4:8])
    assert table[-1].cout == (512 if name == "resnet18" else 2048)


@pytest.mark.parametrize("h", [7, 32, 37, 64, 224])
def test_output_size_arithmetic(h):
    from hcir import ops
    from hcir.resnet_engine import trunk_out_hw
    x = torch.zeros(1, 3, h, h + 3)
    conv = F.conv2d(x, torch.zeros(1, 3, 7, 7), None, 2, 3)
    pooled = F.max_pool2d(conv, 3, 2, 1)
    assert (ops.stem_out_size(h), ops.stem_out_size(h + 3)) == tuple(pooled.shape[2:])
    hc = (h - 1) // 2 + 1
    assert ops.stem_out_size(h) == (hc - 1) // 2 + 1
    for r, pad in ((1, 0), (3, 1)):
        for stride in (1, 2):
            y = F.conv2d(torch.zeros(1, 1, h, h + 3), torch.zeros(1, 1, r, r), None, stride, pad)
            assert (ops.conv_out_size(h, r, stride, pad), ops.conv_out_size(h + 3, r, stride, pad)) == tuple(y.shape[2:])
    with torch.no_grad():
        assert trunk_out_hw(h, h + 3) == tuple(_trunk("resnet18")[:8](x).shape[2:])


def test_unsupported_shapes_without_a_device(hcir_built):
    from hcir._lib import HcirError
    from hcir.resnet_engine import _spec, conv_supported
    L = hcir_built

    def status(cin, cout, r, stride, pad, h=8, w=8):
        # null pointers: the shape is judged before any pointer is looked at, and nothing is launched
        return L.hcir_conv2d_f16(None, 2, h, w, cin, None, cout, r, r, stride, pad, None, None, None, 0, None, None)

    assert status(48, 64, 3, 1, 1) == -2            # Cin = 48
    assert status(64, 96, 1, 1, 0) == -2            # Cout % 64
    assert status(64, 64, 5, 1, 2) == -2            # 5 x 5
    assert status(64, 64, 3, 3, 1) == -2            # stride 3
    assert status(64, 64, 3, 1, 0) == -2            # 3 x 3 without padding
    assert status(64, 64, 3, 1, 1) == -1            # a supported shape gets as far as the null-pointer check
    assert status(64, 64, 3, 1, 1, h=0) == -1
    assert L.hcir_resnet_stem(None, 1, 6, 9, None, None, None, None, None) == -2
    assert L.hcir_avgpool_nhwc_f16(None, 1, 7, 7, 64, 0, 1e-12, None, None) == -1
    assert not conv_supported(3, 3, 1, 1, 48, 64) and conv_supported(1, 1, 2, 0, 256, 512)
    with pytest.raises(HcirError, match="no HIP kernel"):
        _spec("odd", "layer1", nn.Conv2d(48, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), True, "x", "o1")


def test_trunk_that_the_kernels_do_not_compute_is_refused():
    """The stem kernel hard-codes 7x7 / 2 / pad 3 without bias, the 3 / 2 / 1 floor-mode pool and affine BatchNorms with
    running statistics: a trunk that differs must raise, not compute something else."""
    from hcir._lib import HcirError
    from hcir.resnet_engine import layer_table

    def edited(fn):
        kids = list(_trunk("resnet18").children())
        fn(kids)
        return nn.Sequential(*kids)

    def set_(i, m):
        return lambda kids: kids.__setitem__(i, m)

    layer_table(edited(lambda kids: None))
    for edit in (set_(0, nn.Conv2d(3, 64, 7, 1, 3, bias=False)), set_(0, nn.Conv2d(3, 64, 7, 2, 2, bias=False)),
                 set_(0, nn.Conv2d(3, 64, 7, 2, 3, bias=True)), set_(1, nn.BatchNorm2d(64, affine=False)),
                 set_(1, nn.BatchNorm2d(64, track_running_stats=False)), set_(2, nn.GELU()),
                 set_(3, nn.MaxPool2d(3, 2, 1, ceil_mode=True)), set_(3, nn.MaxPool2d(2, 2, 0)),
                 set_(8, nn.AdaptiveAvgPool2d((2, 2)))):
        with pytest.raises(HcirError):
            layer_table(edited(edit))
    t = _trunk("resnet18")
    t[4][0].bn2 = nn.BatchNorm2d(64, affine=False)
    with pytest.raises(HcirError):
        layer_table(t)


def test_hip_trunk_gate_falls_back_for_inputs_the_kernels_do_not_take():
    """A CPU tensor never qualifies; the predicate's shape / dtype / mode terms are exercised on a stand-in that
    reports a HIP device (autocast is checked on the device, tests/test_resnet_engine_gpu.py)."""
    from hcir.resnet_engine import hip_trunk_active
    trunk = _trunk("resnet18")
    with torch.no_grad():
        assert not hip_trunk_active(True, trunk, torch.zeros(1, 3, 8, 8))          # CPU

        class _Dev:    # shape / dtype / device facts of a tensor, nothing else is read
            def __init__(self, shape, dtype=torch.float32):
                self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

            def dim(self):
                return len(self.shape)

        assert hip_trunk_active(True, trunk, _Dev((2, 3, 7, 9)))
        assert not hip_trunk_active(False, trunk, _Dev((2, 3, 7, 9)))
        assert not hip_trunk_active(True, trunk, _Dev((2, 3, 6, 9)))
        assert not hip_trunk_active(True, trunk, _Dev((2, 3, 9, 6)))
        assert not hip_trunk_active(True, trunk, _Dev((2, 1, 32, 32)))
        assert not hip_trunk_active(True, trunk, _Dev((3, 32, 32)))
        assert not hip_trunk_active(True, trunk, _Dev((2, 3, 32, 32), torch.float16))
        trunk.train()
        assert not hip_trunk_active(True, trunk, _Dev((2, 3, 32, 32)))
        trunk.eval()
    assert not hip_trunk_active(True, trunk, _Dev((2, 3, 32, 32)))                 # autograd on


def test_conv_tile_choice(hcir_built):
    L = hcir_built
    assert L.hcir_conv2d_tile_n(2, 7, 7, 64, 64, 3, 3, 1, 1) == 64
    assert L.hcir_conv2d_tile_n(5, 28, 28, 64, 128, 3, 3, 1, 1) == 64        # 31 tiles of 128 x 128: too few
    assert L.hcir_conv2d_tile_n(21, 56, 56, 64, 128, 3, 3, 1, 1) == 128      # 515
    assert L.hcir_conv2d_tile_n(64, 56, 56, 64, 192, 1, 1, 1, 0) == 64       # Cout % 128 != 0
    assert L.hcir_conv2d_tile_n(64, 56, 56, 64, 256, 1, 1, 1, 0) == 128
    assert L.hcir_conv2d_tile_n(1, 8, 8, 48, 64, 3, 3, 1, 1) == -2
