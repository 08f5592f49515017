"""Device-resident CIFAR input path (opt-in: ``TrainConfig.device_data``).

CIFAR-100 is 150 MB as uint8 and an MI355X has 288 GB of HBM, so the dataset
is uploaded once and every batch is produced by ONE ``ops.batch_augment``
launch: no per-sample Python, no worker processes, no per-step host-to-device
copy, no layout-conversion or autocast-cast kernel. Per EPOCH the host uploads
two small int32 tensors: this rank's index list (torch's own
DistributedSampler, so sharding is identical to the DataLoader path) and the
augmentation table (``ops.draw_aug_params``). With CutMix
(``cutmix_alpha > 0``) two more small tables go up per epoch
(``ops.draw_cutmix_params``) and the batches come from
``ops.batch_augment_cutmix``, whose target is ``(labels_a, labels_b, lam)``.

Unlike the DataLoader path (``cifar.py``), whose crop is seeded per index and
therefore the same in every epoch, the augmentation here is redrawn each epoch
as the reference's RandomCrop does (reference utils/dataset.py:6).
"""
from __future__ import annotations

import os
import pickle
from typing import Iterator, Optional, Tuple

import torch
from torch.utils.data.distributed import DistributedSampler

from ..config import TrainConfig
from ..ops.augment import (batch_augment, batch_augment_cutmix,
                           build_norm_lut, draw_aug_params,
                           draw_cutmix_params)
from .cifar import _real_cifar_available

# synthetic split sizes (CIFAR-100's)
SYNTHETIC_TRAIN_N = 50000
SYNTHETIC_TEST_N = 10000


class DeviceCIFAR:
    """``images_u8`` [M, H, W, 3] uint8 (NHWC) and ``labels`` [M] int64, both
    resident on ``device``."""

    def __init__(self, images_u8: torch.Tensor, labels: torch.Tensor,
                 device=None):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 \
                or images_u8.shape[3] != 3:
            raise ValueError("images_u8 must be uint8 [M, H, W, 3]")
        if labels.shape != (images_u8.shape[0],):
            raise ValueError("labels must be [M]")
        device = images_u8.device if device is None else torch.device(device)
        self.images_u8 = images_u8.contiguous().to(device)
        self.labels = labels.to(torch.int64).contiguous().to(device)

    def __len__(self) -> int:
        return self.images_u8.shape[0]

    @property
    def device(self) -> torch.device:
        return self.images_u8.device

    @classmethod
    def from_pickle(cls, root: str, train: bool = True,
                    device=None) -> "DeviceCIFAR":
        """The standard CIFAR-100 python-pickle dump (same file discovery as
        PickleCIFAR100); the bytes are permuted to NHWC and never converted
        to float on the host."""
        path = os.path.join(root, "cifar-100-python",
                            "train" if train else "test")
        with open(path, "rb") as f:
            d = pickle.load(f, encoding="bytes")
        data = torch.frombuffer(bytearray(b"".join(d[b"data"])), dtype=torch.uint8) \
            if isinstance(d[b"data"], list) else torch.from_numpy(d[b"data"].copy())
        images = data.reshape(-1, 3, 32, 32).permute(0, 2, 3, 1).contiguous()
        labels = torch.tensor([int(x) for x in d[b"fine_labels"]],
                              dtype=torch.int64)
        return cls(images, labels, device)

    @classmethod
    def synthetic(cls, n: int = SYNTHETIC_TRAIN_N, num_classes: int = 100,
                  size: int = 32, train: bool = True, seed: int = 0,
                  device=None) -> "DeviceCIFAR":
        """One seeded randint for all images plus one for the labels:
        deterministic per (seed, train). Not SyntheticCIFAR's per-index
        floats."""
        gen = torch.Generator().manual_seed(
            (int(seed) * 1_000_003) * 2 + int(train))
        images = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8,
                               generator=gen)
        labels = torch.randint(0, num_classes, (n,), generator=gen)
        return cls(images, labels, device)


class DeviceLoader:
    """Drop-in for the DataLoader of ``build_loaders``: iterating yields
    ``(images, labels)`` already on the dataset's device, in the layout and
    dtype asked for, one ``batch_augment`` call per batch.

    ``set_epoch(e)`` computes this rank's indices with DistributedSampler over
    ``range(M)`` (seeded by (seed, epoch) at world size 1 too — the global RNG
    is not used) and, with ``augment``, draws that epoch's augmentation table.
    Both are uploaded once per epoch. ``drop_last`` applies to the sampler
    (trim rather than pad to a multiple of the world size) and to the last
    short batch, as the train DataLoader it replaces does.

    ``cutmix_alpha > 0`` turns CutMix on: each sample is mixed with
    probability ``cutmix_prob`` with a partner drawn over the whole DATASET
    (not the batch), so a sample's image is the same at every world size,
    rank and batch size. Iterating then yields ``(images, (labels_a,
    labels_b, lam))`` from one ``batch_augment_cutmix`` launch per batch."""

    def __init__(self, dataset: DeviceCIFAR, batch_size: int,
                 world_size: int = 1, rank: int = 0, shuffle: bool = False,
                 drop_last: bool = False, seed: int = 0, augment: bool = False,
                 pad: int = 4, hflip: bool = False,
                 channels_last: bool = False,
                 out_dtype: torch.dtype = torch.float32,
                 cutmix_alpha: float = 0.0, cutmix_prob: float = 0.5):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if cutmix_alpha < 0:
            raise ValueError("cutmix_alpha must be >= 0")
        if not 0.0 <= cutmix_prob <= 1.0:
            raise ValueError("cutmix_prob must be in [0, 1]")
        self.dataset = dataset
        self.batch_size = batch_size
        self.drop_last = drop_last
        self.seed = seed
        self.augment = augment
        self.pad = pad
        self.hflip = hflip
        self.channels_last = channels_last
        self.out_dtype = out_dtype
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_prob = cutmix_prob
        self.sampler = DistributedSampler(
            range(len(dataset)), num_replicas=world_size, rank=rank,
            shuffle=shuffle, seed=seed, drop_last=drop_last)
        self.lut = build_norm_lut().to(dataset.device)
        self.epoch: Optional[int] = None
        self.indices: Optional[torch.Tensor] = None   # int32 [len(sampler)]
        self.aug: Optional[torch.Tensor] = None       # int32 [M] or None
        self.mix: Optional[torch.Tensor] = None       # int32 [M, 3] or None
        self.lam: Optional[torch.Tensor] = None       # float32 [M] or None

    def set_epoch(self, epoch: int) -> None:
        self.sampler.set_epoch(epoch)
        dev = self.dataset.device
        self.indices = torch.tensor(list(self.sampler),
                                    dtype=torch.int32).to(dev)
        self.aug = draw_aug_params(len(self.dataset), self.pad, self.hflip,
                                   self.seed, epoch).to(dev) \
            if self.augment else None
        if self.cutmix_alpha > 0:
            _, H, W, _ = self.dataset.images_u8.shape
            mix, lam = draw_cutmix_params(len(self.dataset), H, W,
                                          self.cutmix_alpha, self.cutmix_prob,
                                          self.seed, epoch)
            self.mix, self.lam = mix.to(dev), lam.to(dev)
        self.epoch = epoch

    def __len__(self) -> int:
        n = len(self.sampler)
        if self.drop_last:
            return n // self.batch_size
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        if self.indices is None:
            self.set_epoch(0)
        indices, aug, ds, bs = self.indices, self.aug, self.dataset, \
            self.batch_size
        if self.cutmix_alpha > 0:
            mix, lam = self.mix, self.lam
            for b in range(len(self)):
                images, labels_a, labels_b, lam_b = batch_augment_cutmix(
                    ds.images_u8, ds.labels, indices[b * bs:(b + 1) * bs],
                    aug, mix, lam, self.lut, self.pad, self.channels_last,
                    self.out_dtype)
                yield images, (labels_a, labels_b, lam_b)
            return
        for b in range(len(self)):
            yield batch_augment(ds.images_u8, ds.labels,
                                indices[b * bs:(b + 1) * bs], aug, self.lut,
                                self.pad, self.channels_last, self.out_dtype)


def amp_input_dtype(amp: str) -> torch.dtype:
    """The dtype autocast would cast the first conv's input to."""
    if amp in ("bf16", "bf16_o2"):
        return torch.bfloat16
    if amp == "fp16":
        return torch.float16
    return torch.float32


def build_device_datasets(cfg: TrainConfig, device) -> Tuple[DeviceCIFAR,
                                                             DeviceCIFAR]:
    if not cfg.synthetic and _real_cifar_available(cfg.data_root):
        return (DeviceCIFAR.from_pickle(cfg.data_root, True, device),
                DeviceCIFAR.from_pickle(cfg.data_root, False, device))
    return (DeviceCIFAR.synthetic(SYNTHETIC_TRAIN_N, cfg.num_classes,
                                  cfg.image_size, True, cfg.seed, device),
            DeviceCIFAR.synthetic(SYNTHETIC_TEST_N, cfg.num_classes,
                                  cfg.image_size, False, cfg.seed, device))


def build_device_loaders(cfg: TrainConfig, world_size: int, rank: int,
                         device=None,
                         ) -> Tuple[DeviceLoader, DeviceLoader, DeviceLoader]:
    """(train, test, train): the third slot is what ``fit`` calls
    ``set_epoch`` on, so it is the train loader at every world size. Sampler
    arguments are those of ``build_loaders``' DataLoader path."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) \
            if torch.cuda.is_available() else torch.device("cpu")
    train_ds, test_ds = build_device_datasets(cfg, device)
    per_rank = cfg.per_rank_batch(world_size)
    common = dict(world_size=world_size, rank=rank, seed=cfg.seed,
                  channels_last=cfg.channels_last,
                  out_dtype=amp_input_dtype(cfg.amp))
    train_loader = DeviceLoader(train_ds, per_rank, shuffle=True,
                                drop_last=True, augment=True,
                                hflip=cfg.hflip,
                                cutmix_alpha=cfg.cutmix_alpha,
                                cutmix_prob=cfg.cutmix_prob, **common)
    test_loader = DeviceLoader(test_ds, per_rank, shuffle=False,
                               drop_last=False, augment=False, **common)
    return train_loader, test_loader, train_loader
