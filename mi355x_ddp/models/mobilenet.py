"""MobileNet-v1 (Howard et al. 2017, arXiv:1704.04861), width 1.0: a 3x3 stem
to 32 channels, 13 depthwise-separable blocks and a linear classifier.

Beyond the reference zoo, like the ResNeXt models. Every conv + BatchNorm pair
runs through `resnet.conv_bn` with plain ReLU, so the fused BN kernels and the
folded evaluation forward serve it unchanged; the 1x1 convs and the stem run
on the dense igemm kernels and the depthwise 3x3 convs on the kernels of
csrc/conv_depthwise.hip (ops/conv.py). The module tree is plain nn.Conv2d /
nn.BatchNorm2d, as in the ResNet zoo.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.pool import GlobalAvgPool2d
from .resnet import _conv1x1, _conv3x3, conv_bn

# (out_channels, stride) of the 13 blocks; the input of the first has 32
_BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2),
           (512, 1), (512, 1), (512, 1), (512, 1), (512, 1), (1024, 2),
           (1024, 1))


class DepthwiseSeparable(nn.Module):
    """3x3 depthwise (stride here) + BN + ReLU, then 1x1 + BN + ReLU."""

    def __init__(self, cin: int, cout: int, stride: int = 1):
        super().__init__()
        self.conv1 = _conv3x3(cin, cin, stride, groups=cin)
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv2 = _conv1x1(cin, cout)
        self.bn2 = nn.BatchNorm2d(cout)

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        return conv_bn(out, self.conv2, self.bn2)


class MobileNetV1(nn.Module):
    def __init__(self, num_classes: int = 100, imagenet_stem: bool = False):
        super().__init__()
        # CIFAR: stride-1 stem, so a 32 px input ends at 2 x 2; 224 px inputs
        # take the paper's stride-2 stem and end at 7 x 7
        self.conv1 = _conv3x3(3, 32, 2 if imagenet_stem else 1)
        self.bn1 = nn.BatchNorm2d(32)
        blocks, cin = [], 32
        for cout, stride in _BLOCKS:
            blocks.append(DepthwiseSeparable(cin, cout, stride))
            cin = cout
        self.blocks = nn.Sequential(*blocks)
        self.avgpool = GlobalAvgPool2d()
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        out = conv_bn(x, self.conv1, self.bn1)
        out = self.blocks(out)
        out = self.avgpool(out)
        return self.fc(torch.flatten(out, 1))


def mobilenet_v1(num_classes: int = 100) -> MobileNetV1:
    return MobileNetV1(num_classes)


def mobilenet_v1_imagenet(num_classes: int = 100) -> MobileNetV1:
    return MobileNetV1(num_classes, imagenet_stem=True)


_MOBILENET_FACTORIES = {"mobilenet_v1": mobilenet_v1,
                        "mobilenet_v1_imagenet": mobilenet_v1_imagenet}
