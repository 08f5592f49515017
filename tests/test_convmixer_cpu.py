"""ConvMixer and the `_depthwise_large_ok` decision table, without a GPU."""
import argparse

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.config import add_common_args
from mi355x_ddp.models import ConvMixer, build_model
from mi355x_ddp.models.resnet import conv_bn_pairs
from mi355x_ddp.ops import _backend
from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import MIOPEN, _depthwise_large_ok

CL = torch.channels_last
BF, HALF = torch.bfloat16, torch.float16

# arch -> (dim, depth, kernel, patch)
ARCHS = {"convmixer_256_8": (256, 8, 5, 2),
         "convmixer_256_16": (256, 16, 9, 1),
         "convmixer_768_32_imagenet": (768, 32, 7, 7)}


@pytest.mark.parametrize("arch", ARCHS)
def test_factories(arch):
    dim, depth, k, p = ARCHS[arch]
    model = build_model(arch, 10)
    assert isinstance(model, ConvMixer) and len(model.blocks) == depth
    assert model.stem.kernel_size == model.stem.stride == (p, p)
    assert model.stem.out_channels == dim
    for blk in model.blocks:
        assert blk.dw.kernel_size == (k, k) and blk.dw.padding == (k // 2,) * 2
        assert blk.dw.groups == blk.dw.in_channels == dim
        assert blk.pw.kernel_size == (1, 1)
    assert all(m.bias is None for m in model.modules()
               if isinstance(m, nn.Conv2d))
    count = 3 * dim * p * p + 2 * dim + \
        depth * (dim * k * k + 2 * dim + dim * dim + 2 * dim) + dim * 10 + 10
    assert sum(q.numel() for q in model.parameters()) == count
    assert list(conv_bn_pairs(model)) == []
    assert add_common_args(argparse.ArgumentParser()) \
        .parse_args(["--arch", arch]).arch == arch


def test_forward_state_dict_and_groupnorm():
    model = build_model("convmixer_256_8", 100)
    x = torch.randn(2, 3, 32, 32)
    assert model(x).shape == (2, 100)
    twin = build_model("convmixer_256_8", 100)
    twin.load_state_dict(model.state_dict())
    model.eval(), twin.eval()
    assert torch.equal(model(x), twin(x))
    gn = build_model("convmixer_256_8", norm="gn")
    assert not any(isinstance(m, nn.BatchNorm2d) for m in gn.modules())
    assert torch.isfinite(gn(x)).all()
    with pytest.raises(ValueError, match="unknown arch"):
        build_model("convmixer")


def _ok(C=64, K=None, Cg=1, k=5, kw=None, dt=BF, wdt=None, nchw=False,
        stride=(1, 1), padding=None, dilation=(1, 1), groups=None):
    x = torch.zeros(2, C, 8, 8, dtype=dt)
    if not nchw:
        x = x.contiguous(memory_format=CL)
    w = torch.zeros(K or C, Cg, k, kw or k, dtype=wdt or dt)
    return _depthwise_large_ok(x, w, stride, padding or (k // 2, k // 2),
                               dilation, C if groups is None else groups)


@pytest.fixture
def native(monkeypatch):
    monkeypatch.setattr(_backend, "native_enabled", lambda t=None: True)
    for name in ("MI355X_NATIVE_DEPTHWISE", "MI355X_NATIVE_CONV",
                 "MI355X_NATIVE_CONV_FP16"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("deviation", [
    dict(k=3), dict(k=11), dict(k=6), dict(kw=7),
    dict(stride=(2, 2)),
    dict(padding=(1, 1)),
    dict(dilation=(2, 2)),
    dict(K=128),                              # a channel multiplier
    dict(Cg=2, groups=32),
    dict(C=12),
    dict(nchw=True),
    dict(wdt=HALF),                           # mixed 16-bit dtypes
    dict(dt=torch.float32),
], ids=str)
def test_depthwise_large_ok_refuses_each_single_deviation(native, deviation):
    assert _ok() is True
    assert _ok(**deviation) is False


def test_depthwise_large_ok_supported_convs_and_switches(native, monkeypatch):
    assert all(_ok(k=k) is True for k in (5, 7, 9))
    assert _ok(dt=HALF) is True and _ok(C=8) is True
    native.setenv("MI355X_NATIVE_DEPTHWISE", "0")
    assert _ok() is False
    native.setenv("MI355X_NATIVE_DEPTHWISE", "1")
    native.setenv("MI355X_NATIVE_CONV_FP16", "0")
    assert _ok(dt=HALF) is False and _ok() is True
    native.setenv("MI355X_NATIVE_CONV_FP16", "1")
    native.setenv("MI355X_NATIVE_CONV", "0")
    assert _ok() is False
    monkeypatch.undo()                        # CPU tensors, nothing patched
    assert _ok() is False


def test_tune_report_labels_the_large_depthwise_keys(monkeypatch):
    xs = torch.Size((2, 64, 12, 12))
    cache = {("dwk_fwd", BF, xs, 7): 0,
             ("dwk_dgrad", BF, xs, 7): MIOPEN,
             ("dwk_wgrad", BF, xs, 7): ("splits", 0),
             ("dwk_wgrad", HALF, xs, 7): ("splits", 64)}
    monkeypatch.setattr(convmod, "_TUNE_CACHE", cache)
    labels = [ln.split("-> ")[1] for ln in convmod.tune_report().splitlines()]
    assert sorted(labels) == ["MIOpen", "native depthwise KxK",
                              "native depthwise KxK, splits 64",
                              "native depthwise KxK, splits auto"]
