from .resnet import (ResNet, BasicBlock, Bottleneck, resnet18, resnet34,
                     resnet50, resnet101, resnet152, resnext50_32x4d,
                     resnext101_32x8d, resnext50_32x4d_imagenet,
                     se_resnet18, se_resnet50, se_resnext50_32x4d,
                     se_resnet50_imagenet, build_model)  # noqa: F401
from .mobilenet import (MobileNetV1, DepthwiseSeparable, mobilenet_v1,
                        mobilenet_v1_imagenet)  # noqa: F401
from .convmixer import (ConvMixer, ConvMixerBlock, convmixer_256_8,
                        convmixer_256_16,
                        convmixer_768_32_imagenet)  # noqa: F401
