"""ConvMixer (Trockman & Kolter, "Patches Are All You Need?", arXiv:2201.09792):
a patch stem, then `depth` blocks of a residual K x K depthwise conv and a 1x1
conv, each followed by GELU and a norm, then global pooling and a classifier.

Beyond the reference zoo, like the ResNeXt and MobileNet models. The 1x1 convs
and the patch stem run on the dense igemm kernels, the depthwise K x K convs
(K in {5, 7, 9}, stride 1, "same") on the kernels of
csrc/conv_depthwise_large.hip (ops/conv.py), the norms on the fused BatchNorm
kernels, or on the GroupNorm ones under `norm="gn"`. GELU is `F.gelu` and the
residual add a plain add.

Every conv is bias-free, unlike the paper's: `MI355Conv2d.convert` only takes
over bias-free convs, and a bias in front of a norm is absorbed by the norm's
shift. The module tree is plain nn.Conv2d / nn.BatchNorm2d. With GELU between
each conv and its norm there is nothing to fold: `conv_bn_pairs` yields
nothing for this model and `--fused_eval` runs it unfused.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import bn_relu
from ..ops.groupnorm import gn_relu
from ..ops.pool import GlobalAvgPool2d


def _norm(h, bn):
    """The block's norm without an activation: the fused BatchNorm kernels, or
    the GroupNorm ones once `build_model(..., norm="gn")` swapped the layer."""
    if isinstance(bn, nn.GroupNorm):
        return gn_relu(h, bn, False)
    return bn_relu(h, bn, relu=False)


class ConvMixerBlock(nn.Module):
    """x = x + BN(GELU(dw_KxK(x))); x = BN(GELU(conv1x1(x)))."""

    def __init__(self, dim: int, kernel_size: int):
        super().__init__()
        self.dw = nn.Conv2d(dim, dim, kernel_size, padding=kernel_size // 2,
                            groups=dim, bias=False)
        self.bn1 = nn.BatchNorm2d(dim)
        self.pw = nn.Conv2d(dim, dim, kernel_size=1, bias=False)
        self.bn2 = nn.BatchNorm2d(dim)

    def forward(self, x):
        x = x + _norm(F.gelu(self.dw(x)), self.bn1)
        return _norm(F.gelu(self.pw(x)), self.bn2)


class ConvMixer(nn.Module):
    def __init__(self, dim: int, depth: int, kernel_size: int,
                 patch_size: int, num_classes: int = 100):
        super().__init__()
        self.dim, self.depth = dim, depth
        self.kernel_size, self.patch_size = kernel_size, patch_size
        self.stem = nn.Conv2d(3, dim, patch_size, stride=patch_size,
                              bias=False)
        self.bn = nn.BatchNorm2d(dim)
        self.blocks = nn.Sequential(*[ConvMixerBlock(dim, kernel_size)
                                      for _ in range(depth)])
        self.avgpool = GlobalAvgPool2d()
        self.fc = nn.Linear(dim, num_classes)

    def forward(self, x):
        out = _norm(F.gelu(self.stem(x)), self.bn)
        out = self.blocks(out)
        out = self.avgpool(out)
        return self.fc(torch.flatten(out, 1))


def convmixer_256_8(num_classes: int = 100) -> ConvMixer:
    """The paper's CIFAR model: 5x5 depthwise convs on 16 x 16 maps."""
    return ConvMixer(256, 8, 5, 2, num_classes)


def convmixer_256_16(num_classes: int = 100) -> ConvMixer:
    """Patch size 1: 9x9 depthwise convs on 32 x 32 maps."""
    return ConvMixer(256, 16, 9, 1, num_classes)


def convmixer_768_32_imagenet(num_classes: int = 100) -> ConvMixer:
    """ConvMixer-768/32 for 224 px inputs: 7x7 on 32 x 32 maps."""
    return ConvMixer(768, 32, 7, 7, num_classes)


_CONVMIXER_FACTORIES = {"convmixer_256_8": convmixer_256_8,
                        "convmixer_256_16": convmixer_256_16,
                        "convmixer_768_32_imagenet": convmixer_768_32_imagenet}
