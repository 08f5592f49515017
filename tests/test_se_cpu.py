"""Squeeze-and-Excitation without a GPU: the torch definition inside
`se_add_relu` and the SE model factories."""
import pytest
import torch

from mi355x_ddp.models import build_model
from mi355x_ddp.models.resnet import conv_bn_pairs
from mi355x_ddp.ops import SqueezeExcite, se_add_relu
from mi355x_ddp.ops.se import se_calls

SE_ARCHS = ["se_resnet18", "se_resnet50", "se_resnext50_32x4d",
            "se_resnet50_imagenet"]


def _composition(u, identity, se):
    s = u.mean(dim=(2, 3))
    g = torch.sigmoid(se.fc2(torch.relu(se.fc1(s))))
    return torch.relu(u * g[:, :, None, None] + identity)


def test_cpu_path_is_the_torch_composition():
    torch.manual_seed(3)
    se = SqueezeExcite(8, 4).double()
    u = torch.randn(3, 8, 2, 3, dtype=torch.float64, requires_grad=True)
    idn = torch.randn(3, 8, 2, 3, dtype=torch.float64, requires_grad=True)
    params = list(se.parameters())
    se_calls.reset()
    out = se_add_relu(u, idn, se)
    ref = _composition(u, idn, se)
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)
    dout = torch.randn_like(ref)
    got = torch.autograd.grad(out, [u, idn] + params, dout)
    want = torch.autograd.grad(ref, [u, idn] + params, dout)
    for a, b in zip(got, want):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    assert torch.autograd.gradcheck(
        lambda a, b, *p: se_add_relu(a, b, se), [u, idn] + params)
    assert (se_calls.fwd, se_calls.bwd) == (0, 0)


@pytest.mark.parametrize("arch", SE_ARCHS)
def test_se_factories(arch):
    model = build_model(arch, 10)
    out = model(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())
    keys = set(model.state_dict())
    for name in ("layer1.0.se.fc1.weight", "layer1.0.se.fc1.bias",
                 "layer4.1.se.fc2.weight", "layer4.1.se.fc2.bias"):
        assert name in keys
    n_blocks = sum(hasattr(m, "se") for m in model.modules())
    assert n_blocks == (8 if arch == "se_resnet18" else 16)


def test_se_resnet50_folds_the_pairs_of_resnet50():
    se_pairs = list(conv_bn_pairs(build_model("se_resnet50")))
    pairs = list(conv_bn_pairs(build_model("resnet50")))
    assert len(se_pairs) == len(pairs) == 53
    assert [c.weight.shape for c, _ in se_pairs] == \
        [c.weight.shape for c, _ in pairs]


def test_resnet50_keeps_its_keys():
    keys = list(build_model("resnet50").state_dict())
    assert len(keys) == 53 * 6 + 2    # per pair: weight + 5 of BN; fc
    assert not any(".se." in k for k in keys)
    block = build_model("resnet50").layer1[0]
    assert [n for n, _ in block.named_children()] == \
        ["conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "downsample"]
