"""GroupNorm without a GPU: the torch definition inside `gn_relu` /
`gn_add_relu`, the conversion of the zoo (`build_model(..., norm="gn")`) and
the config plumbing."""
import argparse
import copy

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.config import TrainConfig, add_common_args, config_from_args
from mi355x_ddp.core.inference import folded_modules, fused_inference
from mi355x_ddp.models import build_model
from mi355x_ddp.ops import gn_add_relu, gn_relu
from mi355x_ddp.ops.groupnorm import gn_calls


def _count(model, kind):
    return sum(isinstance(m, kind) for m in model.modules())


def test_conversion():
    bn_model = build_model("resnet18")
    model = build_model("resnet18", norm="gn")
    assert _count(model, nn.BatchNorm2d) == 0
    assert _count(model, nn.GroupNorm) == _count(bn_model, nn.BatchNorm2d) == 20
    assert not any("running_" in k or "num_batches" in k
                   for k in model.state_dict())
    assert model.layer2[0].downsample[1].num_groups == 32
    mobile = build_model("mobilenet_v1", norm="gn")
    assert (mobile.bn1.num_channels, mobile.bn1.num_groups) == (32, 16)
    assert build_model("resnet18", norm="gn", gn_groups=8).bn1.num_groups == 8
    with pytest.raises(ValueError, match="gn_groups=48"):
        build_model("resnet18", norm="gn", gn_groups=48)
    with pytest.raises(ValueError, match="unknown norm 'ln'"):
        build_model("resnet18", norm="ln")


def test_default_is_the_batchnorm_model():
    shapes = lambda m: [(k, v.shape) for k, v in m.state_dict().items()]
    assert shapes(build_model("resnet18")) == \
        shapes(build_model("resnet18", norm="bn"))
    assert _count(build_model("resnet18", norm="bn"), nn.GroupNorm) == 0


@pytest.mark.parametrize("arch", ["resnet18", "se_resnet18",
                                  "resnext50_32x4d"])
def test_cpu_logits_against_float64(arch):
    torch.manual_seed(5)
    model = build_model(arch, 100, norm="gn").eval()
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        plain = model(x)
        with fused_inference(model):   # folds nothing, raises nothing
            assert folded_modules(model) == []
            fused = model(x)
        ref = copy.deepcopy(model).double()(x.double())
    assert torch.isfinite(ref).all() and float(ref.norm()) > 0
    assert torch.equal(plain, fused)
    err = float((plain.double() - ref).norm() / ref.norm())
    assert err <= 1e-5, err


@pytest.mark.parametrize("mode", ["linear", "add_relu"])
def test_cpu_autograd_against_float64(mode):
    gen = torch.Generator().manual_seed(2)
    gn = nn.GroupNorm(3, 12)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(12, generator=gen))
        gn.bias.copy_(torch.randn(12, generator=gen))
    x = (torch.randn(2, 12, 3, 5, generator=gen) + 3).requires_grad_(True)
    idn = torch.randn(2, 12, 3, 5, generator=gen, requires_grad=True)
    dout = torch.randn(2, 12, 3, 5, generator=gen)
    gn_calls.reset()
    out = gn_relu(x, gn, relu=False) if mode == "linear" \
        else gn_add_relu(x, idn, gn)
    wrt = [x, gn.weight, gn.bias] + ([idn] if mode == "add_relu" else [])
    got = [out.detach()] + list(torch.autograd.grad(out, wrt, dout))
    assert (gn_calls.fwd, gn_calls.bwd) == (0, 0)

    xd, ga, be, idd = (t.detach().double().requires_grad_(True)
                       for t in (x, gn.weight, gn.bias, idn))
    xg = xd.reshape(2, 3, -1)
    xhat = ((xg - xg.mean(-1, keepdim=True)) /
            (xg.var(-1, unbiased=False, keepdim=True) + gn.eps).sqrt())
    ref = xhat.reshape(xd.shape) * ga[None, :, None, None] \
        + be[None, :, None, None]
    if mode == "add_relu":
        ref = torch.relu(ref + idd)
    wrt = [xd, ga, be] + ([idd] if mode == "add_relu" else [])
    want = [ref.detach()] + list(torch.autograd.grad(ref, wrt, dout.double()))
    for a, b in zip(got, want):
        assert a.dtype == torch.float32
        assert float((a.double() - b).norm() / b.norm()) <= 1e-5


def test_config():
    cfg = TrainConfig(norm="gn")
    assert (cfg.norm, cfg.gn_groups) == ("gn", 32)
    assert TrainConfig().norm == "bn"
    with pytest.raises(ValueError, match="norm must be"):
        TrainConfig(norm="xx")
    with pytest.raises(ValueError, match="gn_groups must be"):
        TrainConfig(norm="gn", gn_groups=0)
    parser = add_common_args(argparse.ArgumentParser())
    cfg = config_from_args(parser.parse_args(["--norm", "gn",
                                              "--gn_groups", "16"]))
    assert (cfg.norm, cfg.gn_groups) == ("gn", 16)
    assert config_from_args(parser.parse_args([])).norm == "bn"
