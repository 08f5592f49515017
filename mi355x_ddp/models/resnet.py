"""CIFAR-variant ResNet-18/34/50 (capability parity with reference utils/model.py).

Same architecture family as the reference model zoo (3x3 stem, no maxpool,
32x32 inputs, four stages, num_classes=100 — reference utils/model.py:61-127)
but written for the MI355X execution path: every BatchNorm+ReLU pair and the
residual BN+add+ReLU join dispatch to fused HIP kernels through
ops.bn_relu / ops.bn_add_relu (one kernel instead of 2-3 ATen launches), with
the module tree kept as standard nn.Conv2d/nn.BatchNorm2d so checkpoints,
SyncBN conversion and torch-eager parity A/B all operate on the same state.
Convolutions run through nn.Conv2d (MIOpen) or the native implicit-GEMM HIP
kernel when enabled (ops.conv, added by the kernel campaign).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import bn_relu, bn_add_relu
from ..ops.fused_eval import FOLDED_ATTR, conv_bn_act
from ..ops.pool import GlobalAvgPool2d


def conv_bn(x, conv, bn, relu: bool = True, identity=None):
    """`bn_relu(conv(x), bn, relu)`, or `bn_add_relu(conv(x), identity, bn)`
    when `identity` is given: every conv + BatchNorm pair of the zoo. That is
    exactly what runs, in that order, unless `bn` carries folded tables
    (core/inference.py) and is not training; then the pair is one
    `conv_bn_act`. `identity` may be a function without arguments, called
    where the join needs its value: after the conv on the plain path, as the
    blocks always ordered it, and before the fused call that consumes it."""
    if not bn.training:
        # the tables are a plain instance attribute; looking in __dict__
        # spares a training or unfolded forward nn.Module's __getattr__
        folded = bn.__dict__.get(FOLDED_ATTR)
        if folded is not None:
            if callable(identity):
                identity = identity()
            return conv_bn_act(x, conv, folded, relu, identity, bn=bn)
    out = conv(x)
    if identity is None:
        return bn_relu(out, bn, relu)
    if callable(identity):
        identity = identity()
    return bn_add_relu(out, identity, bn)


def _identity(block, x):
    """The residual branch of a block: x, or its 1x1 projection."""
    if block.downsample is None:
        return x
    return conv_bn(x, block.downsample[0], block.downsample[1], relu=False)


def _conv3x3(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


def _conv1x1(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    """Two 3x3 convs; expansion 1 (reference utils/model.py:3-28)."""

    expansion = 1

    def __init__(self, cin: int, cout: int, stride: int = 1):
        super().__init__()
        self.conv1 = _conv3x3(cin, cout, stride)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = _conv3x3(cout, cout)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout * self.expansion:
            self.downsample = nn.Sequential(
                _conv1x1(cin, cout * self.expansion, stride),
                nn.BatchNorm2d(cout * self.expansion),
            )

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        return conv_bn(out, self.conv2, self.bn2,
                       identity=lambda: _identity(self, x))


class Bottleneck(nn.Module):
    """1x1 -> 3x3 -> 1x1; expansion 4 (reference utils/model.py:32-59, minus
    its stray debug print at :37)."""

    expansion = 4

    def __init__(self, cin: int, cout: int, stride: int = 1):
        super().__init__()
        self.conv1 = _conv1x1(cin, cout)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = _conv3x3(cout, cout, stride)
        self.bn2 = nn.BatchNorm2d(cout)
        self.conv3 = _conv1x1(cout, cout * self.expansion)
        self.bn3 = nn.BatchNorm2d(cout * self.expansion)
        self.downsample = None
        if stride != 1 or cin != cout * self.expansion:
            self.downsample = nn.Sequential(
                _conv1x1(cin, cout * self.expansion, stride),
                nn.BatchNorm2d(cout * self.expansion),
            )

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        out = conv_bn(out, self.conv2, self.bn2)
        return conv_bn(out, self.conv3, self.bn3,
                       identity=lambda: _identity(self, x))


class ResNet(nn.Module):
    def __init__(self, block, num_blocks, num_classes: int = 100,
                 imagenet_stem: bool = False):
        super().__init__()
        self.in_channels = 64
        if imagenet_stem:
            # standard ImageNet stem: 7x7 s2 + 3x3 s2 maxpool (4x spatial
            # reduction before stage 1) — beyond the reference zoo, for
            # 224px inputs; the PADC conv path handles the 7x7 C=3 stem
            self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2,
                                   padding=3, bias=False)
            self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        else:
            # CIFAR stem: single 3x3, stride 1, no maxpool (reference
            # utils/model.py:66-70)
            self.conv1 = _conv3x3(3, 64)
            self.maxpool = None
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = self._make_layer(block, 64, num_blocks[0], 1)
        self.layer2 = self._make_layer(block, 128, num_blocks[1], 2)
        self.layer3 = self._make_layer(block, 256, num_blocks[2], 2)
        self.layer4 = self._make_layer(block, 512, num_blocks[3], 2)
        self.avgpool = GlobalAvgPool2d()  # native HIP global-avg-pool kernel
        self.fc = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, cout, blocks, stride):
        strides = [stride] + [1] * (blocks - 1)
        layers = []
        for s in strides:
            layers.append(block(self.in_channels, cout, s))
            self.in_channels = cout * block.expansion
        return nn.Sequential(*layers)

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        if self.maxpool is not None:
            out = self.maxpool(out)
        out = self.layer1(out)
        out = self.layer2(out)
        out = self.layer3(out)
        out = self.layer4(out)
        out = self.avgpool(out)
        out = torch.flatten(out, 1)
        return self.fc(out)


def conv_bn_pairs(model: nn.Module):
    """Every (conv, BatchNorm) pair that `conv_bn` runs in `model`, in module
    order: what core/inference.py folds."""
    for m in model.modules():
        if isinstance(m, (ResNet, BasicBlock, Bottleneck)):
            for i in (1, 2, 3):
                conv = getattr(m, f"conv{i}", None)
                if conv is not None:
                    yield conv, getattr(m, f"bn{i}")
        if isinstance(m, (BasicBlock, Bottleneck)) and \
                m.downsample is not None:
            yield m.downsample[0], m.downsample[1]


def resnet18(num_classes: int = 100) -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes)


def resnet34(num_classes: int = 100) -> ResNet:
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes)


def resnet50(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes)


def resnet101(num_classes: int = 100) -> ResNet:
    """Beyond the reference zoo (which stops at resnet50) — same Bottleneck
    family, deeper stage 3."""
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes)


def resnet152(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 8, 36, 3], num_classes)


def resnet50_imagenet(num_classes: int = 100) -> ResNet:
    """ImageNet-topology ResNet50 (7x7 s2 stem + maxpool, stages at
    56/28/14/7 px for 224px inputs) — beyond the reference zoo, which is
    CIFAR-only; the BASELINE 'ImageNet-shape' config can run either this
    or the CIFAR-stem resnet50 on 224px data."""
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, imagenet_stem=True)


def resnet18_imagenet(num_classes: int = 100) -> ResNet:
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, imagenet_stem=True)


_FACTORIES = {"resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50,
              "resnet101": resnet101, "resnet152": resnet152,
              "resnet18_imagenet": resnet18_imagenet,
              "resnet50_imagenet": resnet50_imagenet}


def build_model(arch: str, num_classes: int = 100) -> ResNet:
    if arch not in _FACTORIES:
        raise ValueError(f"unknown arch {arch!r}; choose from {sorted(_FACTORIES)}")
    return _FACTORIES[arch](num_classes)
