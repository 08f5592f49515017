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
from ..ops.groupnorm import convert_group_norm, gn_add_relu, gn_relu
from ..ops.pool import GlobalAvgPool2d
from ..ops.se import SqueezeExcite, se_add_relu


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
    # a GroupNorm layer (`build_model(..., norm="gn")`) never folds: it has no
    # running statistics, and runs ops/groupnorm.py in training and evaluation
    gn = isinstance(bn, nn.GroupNorm)
    if identity is None:
        return gn_relu(out, bn, relu) if gn else bn_relu(out, bn, relu)
    if callable(identity):
        identity = identity()
    if gn:
        return gn_add_relu(out, identity, bn)
    return bn_add_relu(out, identity, bn)


def _identity(block, x):
    """The residual branch of a block: x, or its 1x1 projection."""
    if block.downsample is None:
        return x
    return conv_bn(x, block.downsample[0], block.downsample[1], relu=False)


def _conv3x3(cin: int, cout: int, stride: int = 1,
             groups: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1,
                     groups=groups, bias=False)


def _conv1x1(cin: int, cout: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False)


def _add_se(block, channels: int, se_reduction: int) -> None:
    """A non-zero `se_reduction` makes `block` a Squeeze-and-Excitation block:
    it owns `se` and ends with `se_add_relu` on its last BatchNorm's output.
    At 0 the block has the modules and the forward it always had."""
    block.se_reduction = se_reduction
    if se_reduction:
        block.se = SqueezeExcite(channels, se_reduction)


class BasicBlock(nn.Module):
    """Two 3x3 convs; expansion 1 (reference utils/model.py:3-28)."""

    expansion = 1

    def __init__(self, cin: int, cout: int, stride: int = 1,
                 se_reduction: int = 0):
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
        _add_se(self, cout * self.expansion, se_reduction)

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        if self.se_reduction:
            return se_add_relu(conv_bn(out, self.conv2, self.bn2, relu=False),
                               _identity(self, x), self.se)
        return conv_bn(out, self.conv2, self.bn2,
                       identity=lambda: _identity(self, x))


class Bottleneck(nn.Module):
    """1x1 -> 3x3 -> 1x1; expansion 4 (reference utils/model.py:32-59, minus
    its stray debug print at :37). `groups` and `base_width` make it the
    ResNeXt block: the inner width is int(cout * base_width / 64) * groups and
    the 3x3 is grouped; the defaults give the plain block."""

    expansion = 4

    def __init__(self, cin: int, cout: int, stride: int = 1,
                 groups: int = 1, base_width: int = 64,
                 se_reduction: int = 0):
        super().__init__()
        width = int(cout * base_width / 64) * groups
        self.conv1 = _conv1x1(cin, width)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv3x3(width, width, stride, groups)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = _conv1x1(width, cout * self.expansion)
        self.bn3 = nn.BatchNorm2d(cout * self.expansion)
        self.downsample = None
        if stride != 1 or cin != cout * self.expansion:
            self.downsample = nn.Sequential(
                _conv1x1(cin, cout * self.expansion, stride),
                nn.BatchNorm2d(cout * self.expansion),
            )
        _add_se(self, cout * self.expansion, se_reduction)

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        out = conv_bn(out, self.conv2, self.bn2)
        if self.se_reduction:
            return se_add_relu(conv_bn(out, self.conv3, self.bn3, relu=False),
                               _identity(self, x), self.se)
        return conv_bn(out, self.conv3, self.bn3,
                       identity=lambda: _identity(self, x))


class ResNet(nn.Module):
    def __init__(self, block, num_blocks, num_classes: int = 100,
                 imagenet_stem: bool = False, groups: int = 1,
                 base_width: int = 64, se_reduction: int = 0):
        super().__init__()
        self.in_channels = 64
        # ResNeXt (Bottleneck only): passed to every block when not default
        self.block_kwargs = {} if (groups, base_width) == (1, 64) else \
            {"groups": groups, "base_width": base_width}
        if se_reduction:   # Squeeze-and-Excitation blocks (ops/se.py)
            self.block_kwargs["se_reduction"] = se_reduction
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
            layers.append(block(self.in_channels, cout, s,
                                **self.block_kwargs))
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
    # imported here: models/mobilenet.py builds on this module
    from .mobilenet import DepthwiseSeparable, MobileNetV1
    for m in model.modules():
        if isinstance(m, (ResNet, BasicBlock, Bottleneck, MobileNetV1,
                          DepthwiseSeparable)):
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


def resnext50_32x4d(num_classes: int = 100) -> ResNet:
    """ResNeXt-50 32x4d on the CIFAR stem: the Bottleneck zoo with a grouped
    3x3 (32 groups of 4, 8, 16, 32 channels over the four stages), which runs
    on the packed grouped kernels (ops/conv.py)."""
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, groups=32,
                  base_width=4)


def resnext101_32x8d(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes, groups=32,
                  base_width=8)


def resnext50_32x4d_imagenet(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, imagenet_stem=True,
                  groups=32, base_width=4)


def se_resnet18(num_classes: int = 100) -> ResNet:
    """SE-ResNet (Hu et al. 2018) on the CIFAR stem: every block ends with the
    Squeeze-and-Excitation join of ops/se.py, reduction 16."""
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes, se_reduction=16)


def se_resnet50(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, se_reduction=16)


def se_resnext50_32x4d(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, groups=32,
                  base_width=4, se_reduction=16)


def se_resnet50_imagenet(num_classes: int = 100) -> ResNet:
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, imagenet_stem=True,
                  se_reduction=16)


_FACTORIES = {"resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50,
              "resnet101": resnet101, "resnet152": resnet152,
              "resnet18_imagenet": resnet18_imagenet,
              "resnet50_imagenet": resnet50_imagenet}


# kept apart from _FACTORIES, whose key set is the plain ResNet zoo
_RESNEXT_FACTORIES = {"resnext50_32x4d": resnext50_32x4d,
                      "resnext101_32x8d": resnext101_32x8d,
                      "resnext50_32x4d_imagenet": resnext50_32x4d_imagenet}


_SE_FACTORIES = {"se_resnet18": se_resnet18, "se_resnet50": se_resnet50,
                 "se_resnext50_32x4d": se_resnext50_32x4d,
                 "se_resnet50_imagenet": se_resnet50_imagenet}


def build_model(arch: str, num_classes: int = 100, norm: str = "bn",
                gn_groups: int = 32) -> nn.Module:
    """`norm="gn"` gives the same model with every BatchNorm2d replaced by a
    GroupNorm of `min(gn_groups, C // 2)` groups (ops/groupnorm.py); the
    default is the BatchNorm model, module for module."""
    from .convmixer import _CONVMIXER_FACTORIES
    from .mobilenet import _MOBILENET_FACTORIES
    factories = {**_FACTORIES, **_RESNEXT_FACTORIES, **_SE_FACTORIES,
                 **_MOBILENET_FACTORIES, **_CONVMIXER_FACTORIES}
    if arch not in factories:
        raise ValueError(f"unknown arch {arch!r}; choose from {sorted(factories)}")
    if norm not in ("bn", "gn"):
        raise ValueError(f"unknown norm {norm!r}; choose from ['bn', 'gn']")
    model = factories[arch](num_classes)
    if norm == "gn":
        model = convert_group_norm(model, gn_groups)
    return model
