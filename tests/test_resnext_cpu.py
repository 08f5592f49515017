"""ResNeXt models: block widths and groups, CPU forward, state-dict round
trip, conv/BN pairs; the plain zoo and the default Bottleneck are unchanged."""
import pytest
import torch

from mi355x_ddp.models import Bottleneck, build_model
from mi355x_ddp.models.resnet import _FACTORIES, conv_bn_pairs
from mi355x_ddp.ops.conv import _grouped_ok

# name -> (base width, blocks in stage 3, image size, conv/BN pairs)
RESNEXTS = {"resnext50_32x4d": (4, 6, 16, 53),
            "resnext101_32x8d": (8, 23, 16, 104),
            "resnext50_32x4d_imagenet": (4, 6, 32, 53)}


@pytest.mark.parametrize("arch", sorted(RESNEXTS))
def test_resnext_model(arch):
    base_width, stage3, size, pairs = RESNEXTS[arch]
    torch.manual_seed(0)
    model = build_model(arch, 100)
    assert len(model.layer3) == stage3
    for i, cout in enumerate((64, 128, 256, 512)):
        for block in getattr(model, f"layer{i + 1}"):
            width = cout * base_width // 64 * 32
            assert block.conv2.groups == 32
            assert block.conv2.weight.shape == (width, width // 32, 3, 3)
            assert block.conv1.out_channels == width
            assert block.conv3.weight.shape == (cout * 4, width, 1, 1)
    assert sum(1 for _ in conv_bn_pairs(model)) == pairs
    with torch.no_grad():
        assert model(torch.randn(2, 3, size, size)).shape == (2, 100)
    twin = build_model(arch, 100)
    twin.load_state_dict(model.state_dict())
    assert all(torch.equal(a, b) for a, b in
               zip(model.state_dict().values(), twin.state_dict().values()))


def test_plain_zoo_is_unchanged():
    assert set(_FACTORIES) == {"resnet18", "resnet34", "resnet50", "resnet101",
                               "resnet152", "resnet18_imagenet",
                               "resnet50_imagenet"}
    shapes = {k: tuple(v.shape)
              for k, v in Bottleneck(64, 64).state_dict().items()
              if v.dim() == 4}
    assert shapes == {"conv1.weight": (64, 64, 1, 1),
                      "conv2.weight": (64, 64, 3, 3),
                      "conv3.weight": (256, 64, 1, 1),
                      "downsample.0.weight": (256, 64, 1, 1)}
    with pytest.raises(ValueError):
        build_model("resnext50")


def test_grouped_ok_is_false_on_cpu():
    x = torch.randn(2, 64, 8, 8).bfloat16().contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(64, 8, 3, 3).bfloat16()
    assert not _grouped_ok(x, w, (1, 1), (1, 1), (1, 1), 8)
