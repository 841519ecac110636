"""CPU (no GPU): which AAConv2d head widths the HIP attention kernels take (AAConv2d.kernel_support / unsupported()), on the
configurations of the reference's CIFAR harness (--attn_k / --attn_v / --attn_nh) and its DenseNet / ResNet constructors."""
import pytest


def attn(k, v, nh, d):
    return {"k": k, "v": v, "nh": nh, "relative": True, "input_dims": d}


def _aa_layers(model):
    from chexpert_amd.models.densenet import AAConv2d
    return [(n, m) for n, m in model.named_modules() if isinstance(m, AAConv2d)]


def _heads(model, name):
    m = dict(model.named_modules())[name]
    return m.dk, m.dv, m.nh, m.dk // m.nh, m.dv // m.nh


def test_reference_head_widths_are_supported():
    """The rows of the head-width table: every AAConv2d of these networks passes kernel_support, including the layers whose heads are
    not 20 key channels (wider keys, more than 13 value channels, head offsets that are not multiples of 4)."""
    from chexpert_amd.models import BasicBlock, Bottleneck, DenseNet, ResNet, WideResNet
    cases = [
        (WideResNet(BasicBlock, 16, 4, num_classes=10, attn_params=attn(.5, .25, 4, (32, 32))), "layer3.0.conv1", (128, 64, 4, 32, 16)),
        (WideResNet(BasicBlock, 28, 10, num_classes=100, attn_params=attn(.4, .1, 8, (32, 32))), "layer3.0.conv1", (256, 64, 8, 32, 8)),
        (DenseNet(32, (6, 12, 24, 16), 64, attn_params=attn(.5, .1, 8, (320, 320))), "features.transition3.conv", (256, 48, 8, 32, 6)),
        (ResNet(Bottleneck, [3, 4, 6, 3], attn_params=attn(.5, .1, 8, (224, 224))), "layer4.0.conv2", (256, 48, 8, 32, 6)),
        (DenseNet(32, (6, 4, 2, 2), 64, attn_params=attn(1.6, .25, 8, (64, 64))), "features.transition1.conv", (200, 32, 8, 25, 4)),
    ]
    for model, name, want in cases:
        assert _heads(model, name) == want, (name, _heads(model, name))
        layers = _aa_layers(model)
        assert layers
        for n, m in layers:
            assert m.kernel_support and m.unsupported() == "", (n, m.dk, m.dv, m.nh, m.unsupported())
    dn = cases[-1][0]
    assert _heads(dn, "features.transition2.conv") == (200, 32, 8, 25, 4)


def test_wideresnet_with_wide_heads_builds_its_engine_on_the_cpu():
    from chexpert_amd.models import BasicBlock, WideResNet
    WideResNet(BasicBlock, 16, 4, num_classes=10, attn_params=attn(.5, .25, 4, (32, 32)))._eng()
    WideResNet(BasicBlock, 28, 10, num_classes=100, attn_params=attn(.4, .1, 8, (32, 32)))._eng()


def test_shapes_outside_the_kernels_still_raise_naming_the_condition():
    from chexpert_amd.models import BasicBlock, DenseNet, ResNet, WideResNet
    # dv = 128 > 104 (ResNet18 layer4 at .25 / .25 / 8 heads): the out-projection limit
    with pytest.raises(NotImplementedError, match="dv = 128 is above 104"):
        ResNet(BasicBlock, [2, 2, 2, 2], attn_params=attn(.25, .25, 8, (224, 224)))._eng()
    # 2 heads on WRN-16-4 at the harness defaults: layer3 has dk 50, dv 24 -> 124 qkv channels, not a multiple of 8
    m = WideResNet(BasicBlock, 16, 4, num_classes=10, attn_params=attn(.2, .1, 2, (32, 32)))
    assert (m.layer3[0].conv1.dk, m.layer3[0].conv1.dv) == (50, 24)
    assert not m.layer3[0].conv1.kernel_support
    with pytest.raises(NotImplementedError, match="not a multiple of 8"):
        m._eng()
    # one head of 128 key channels (k = .5 on the 256-channel stage of WRN-16-4)
    m = WideResNet(BasicBlock, 16, 4, num_classes=10, attn_params=attn(.5, .25, 1, (32, 32)))
    assert m.layer3[0].conv1.dk == 128 and not m.layer3[0].conv1.kernel_support
    with pytest.raises(NotImplementedError, match="dk/nh = 128 is outside 1 .. 64"):
        m._eng()
    # value heads above 64 channels (one head, v = .5 on 256 channels of a DenseNet transition is dv = 64 ... at v = .75, 96)
    m = DenseNet(32, (6, 4, 2, 2), 64, attn_params=attn(.2, .75, 1, (64, 64)))
    t1 = m.features.transition1.conv
    assert t1.dv == 96 and "dv/nh = 96 is outside 1 .. 64" in t1.unsupported()
    with pytest.raises(NotImplementedError, match="dv/nh = 96"):
        m._eng()


def test_the_dkh_20_layers_keep_their_support():
    """What ran before runs now: the attention DenseNet / ResNet / WRN settings of chexpert.py and the CIFAR harness defaults."""
    from chexpert_amd.models import BasicBlock, DenseNet, WideResNet
    for model in (DenseNet(32, (6, 12, 24, 16), 64, attn_params=attn(.2, .1, 8, (320, 320))),
                  WideResNet(BasicBlock, 16, 4, num_classes=10, attn_params=attn(.2, .1, 8, (32, 32))),
                  WideResNet(BasicBlock, 10, 10, num_classes=10, attn_params=attn(.2, .1, 8, (32, 32)))):
        for n, m in _aa_layers(model):
            assert m.dk // m.nh == 20 and m.kernel_support, n
        model._eng()
