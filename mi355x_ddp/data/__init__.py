from .cifar import (PickleCIFAR100, SyntheticCIFAR, build_datasets,
                    build_loaders, normalize, random_crop_padded)
from .device import DeviceCIFAR, DeviceLoader

__all__ = ["PickleCIFAR100", "SyntheticCIFAR", "build_datasets",
           "build_loaders", "normalize", "random_crop_padded",
           "DeviceCIFAR", "DeviceLoader"]
