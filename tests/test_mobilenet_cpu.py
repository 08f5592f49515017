"""MobileNet-v1 and the `_depthwise_ok` decision table, without a GPU."""
import pytest
import torch
import torch.nn as nn

from mi355x_ddp.models import build_model
from mi355x_ddp.models.resnet import conv_bn_pairs
from mi355x_ddp.ops import _backend
from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import MIOPEN, _depthwise_ok

CL = torch.channels_last
BF, HALF = torch.bfloat16, torch.float16


def test_mobilenet_v1_model():
    model = build_model("mobilenet_v1", 100)
    assert model(torch.randn(2, 3, 32, 32)).shape == (2, 100)
    # 3x3x3x32 + 64 for the stem, per block 9c + 2c + c*k + 2k, 1024*100 + 100
    assert sum(p.numel() for p in model.parameters()) == 3206976 + 102500
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    assert sum(m.groups == m.in_channels for m in convs) == 13
    pairs = list(conv_bn_pairs(model))
    assert len(pairs) == 27 == len(convs)
    assert all(bn.num_features == conv.out_channels for conv, bn in pairs)
    assert build_model("mobilenet_v1_imagenet", 10).conv1.stride == (2, 2)


def _ok(C=64, K=None, Cg=1, k=3, dt=BF, wdt=None, nchw=False, stride=(1, 1),
        padding=(1, 1), dilation=(1, 1), groups=None):
    x = torch.zeros(2, C, 8, 8, dtype=dt)
    if not nchw:
        x = x.contiguous(memory_format=CL)
    w = torch.zeros(K or C, Cg, k, k, dtype=wdt or dt)
    return _depthwise_ok(x, w, stride, padding, dilation,
                         C if groups is None else groups)


@pytest.fixture
def native(monkeypatch):
    monkeypatch.setattr(_backend, "native_enabled", lambda t=None: True)
    for name in ("MI355X_NATIVE_DEPTHWISE", "MI355X_NATIVE_CONV",
                 "MI355X_NATIVE_CONV_FP16"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_depthwise_ok_is_false_off_the_gpu():
    assert _ok() is False                     # CPU tensors, nothing patched


def test_depthwise_ok_takes_the_supported_convs(native):
    assert _ok() is True                      # the baseline of the table below
    assert _ok(stride=(2, 2)) is True
    assert _ok(dt=HALF) is True
    assert _ok(C=8) is True


@pytest.mark.parametrize("deviation", [
    dict(Cg=2, groups=32),                    # groups != C
    dict(groups=1),
    dict(K=128),                              # a channel multiplier
    dict(k=5),
    dict(padding=(0, 0)),
    dict(dilation=(2, 2)),
    dict(stride=(3, 3)),
    dict(nchw=True),
    dict(wdt=HALF),                           # mixed 16-bit dtypes
    dict(wdt=torch.float32),
    dict(C=12),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()).replace(
    "torch.", ""))
def test_depthwise_ok_refuses_each_single_deviation(native, deviation):
    assert _ok() is True
    assert _ok(**deviation) is False


def test_depthwise_ok_switches(native):
    native.setenv("MI355X_NATIVE_DEPTHWISE", "0")
    assert _ok() is False
    native.setenv("MI355X_NATIVE_DEPTHWISE", "1")
    native.setenv("MI355X_NATIVE_CONV_FP16", "0")
    assert _ok(dt=HALF) is False
    assert _ok() is True                      # bf16 is not that switch's
    native.setenv("MI355X_NATIVE_CONV_FP16", "1")
    native.setenv("MI355X_NATIVE_CONV", "0")
    assert _ok() is False


def test_tune_report_labels_the_depthwise_keys(monkeypatch):
    xs = torch.Size((2, 64, 12, 12))
    cache = {("dw_fwd", BF, xs, 1): 0,
             ("dw_dgrad", BF, xs, xs, 1): MIOPEN,
             ("dw_wgrad", BF, xs, xs, 1): ("splits", 0),
             ("dw_wgrad", HALF, xs, xs, 1): ("splits", 8)}
    monkeypatch.setattr(convmod, "_TUNE_CACHE", cache)
    labels = [ln.split("-> ")[1] for ln in convmod.tune_report().splitlines()]
    assert sorted(labels) == ["MIOpen", "native depthwise",
                              "native depthwise, splits 8",
                              "native depthwise, splits auto"]
