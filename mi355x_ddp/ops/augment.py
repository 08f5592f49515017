"""Fused padded-crop / flip / normalize / cast of a device-resident uint8
dataset (csrc/data_aug.hip): the whole train transform of the reference
(RandomCrop(32, padding=4) + Normalize, reference utils/dataset.py:3-14) as
one launch per batch, emitting the layout and dtype the first conv consumes.

Definition, for output pixel (n, c, h, w) of dataset image ``i = idx[n]`` with
``top, left, flip`` unpacked from ``aug[i]``:

    source row    = h + top - pad
    source column = (W-1-w if flip else w) + left - pad
    byte          = images_u8[i, row, column, c], or 0 outside the image
    value         = lut[c][byte], rounded to ``out_dtype`` (nearest even)

The zero is a zero BYTE, i.e. padding happens before normalization exactly as
in ``random_crop_padded`` + ``normalize``: a border pixel is ``lut[c][0]``.
``aug=None`` is evaluation (top = left = pad, no flip). Normalization is a
table lookup, so the HIP kernel and the torch implementation below agree bit
for bit; the torch one is the CPU path and the oracle of the GPU tests.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _backend

_OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def build_norm_lut() -> torch.Tensor:
    """[3, 256] fp32: entry [c][v] is the normalized value of byte v in
    channel c — ``normalize`` applied to ``arange(256).float() / 255``, which
    reproduces ``normalize(u8.float().div(255))`` bit for bit."""
    from ..data.cifar import normalize  # data imports ops; resolve lazily
    ramp = torch.arange(256).float() / 255
    return normalize(ramp.view(1, 1, 256).expand(3, 1, 256)) \
        .reshape(3, 256).contiguous()


def draw_aug_params(n: int, pad: int, hflip: bool, seed: int,
                    epoch: int) -> torch.Tensor:
    """int32[n] of ``top | left << 8 | flip << 16``, one word per DATASET
    index, from one Generator seeded by (seed, epoch). Indexing by dataset
    index makes a sample's augmentation independent of world size, rank and
    batch size; the epoch in the seed makes it differ from epoch to epoch.
    The flip draw is made (and dropped) with hflip off too, so top/left do
    not depend on the flag."""
    if not 0 <= pad <= 127:
        raise ValueError(f"pad must be in [0, 127], got {pad}")
    gen = torch.Generator().manual_seed(int(seed) * 1_000_003 + int(epoch))
    top = torch.randint(0, 2 * pad + 1, (n,), generator=gen)
    left = torch.randint(0, 2 * pad + 1, (n,), generator=gen)
    flip = torch.randint(0, 2, (n,), generator=gen)
    if not hflip:
        flip = torch.zeros_like(flip)
    return (top | (left << 8) | (flip << 16)).to(torch.int32)


def _batch_augment_torch(images_u8, labels_i64, idx_i32, aug_i32, lut_f32,
                         pad, channels_last, out_dtype):
    M, H, W, _ = images_u8.shape
    dev = images_u8.device
    idx = idx_i32.long()
    if aug_i32 is None:
        top = left = torch.full_like(idx, pad)
        flip = torch.zeros_like(idx, dtype=torch.bool)
    else:
        a = aug_i32[idx].long()
        top, left, flip = a & 0xff, (a >> 8) & 0xff, ((a >> 16) & 1).bool()
    hh = torch.arange(H, device=dev)[None, :] + (top[:, None] - pad)  # [N,H]
    ww = torch.arange(W, device=dev)[None, :].expand(idx.numel(), W)
    ww = torch.where(flip[:, None], W - 1 - ww, ww) + (left[:, None] - pad)
    inside = (((hh >= 0) & (hh < H))[:, :, None]
              & ((ww >= 0) & (ww < W))[:, None, :])                   # [N,H,W]
    src = images_u8[idx[:, None, None],
                    hh.clamp(0, H - 1)[:, :, None],
                    ww.clamp(0, W - 1)[:, None, :]]                   # [N,H,W,3]
    src = src * inside[..., None].to(torch.uint8)
    out = lut_f32[torch.arange(3, device=dev), src.long()].to(out_dtype)
    out = out.permute(0, 3, 1, 2)          # NHWC memory viewed as [N,3,H,W]
    out = out.contiguous(memory_format=torch.channels_last if channels_last
                         else torch.contiguous_format)
    return out, labels_i64[idx]


def batch_augment(images_u8: torch.Tensor, labels_i64: torch.Tensor,
                  idx_i32: torch.Tensor, aug_i32: Optional[torch.Tensor],
                  lut_f32: torch.Tensor, pad: int = 4,
                  channels_last: bool = False,
                  out_dtype: torch.dtype = torch.float32,
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(images [N,3,H,W] in ``out_dtype``, labels [N]) for the dataset indices
    ``idx_i32``; see the module docstring for the definition."""
    if images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError("images_u8 must be [M, H, W, 3] (NHWC, 3 channels), "
                         f"got {tuple(images_u8.shape)}")
    if images_u8.dtype != torch.uint8 or not images_u8.is_contiguous():
        raise ValueError("images_u8 must be a contiguous uint8 tensor")
    if idx_i32.dtype != torch.int32 or idx_i32.dim() != 1:
        raise ValueError("idx_i32 must be a 1-D int32 tensor")
    if not 0 <= pad <= 127:
        raise ValueError(f"pad must be in [0, 127], got {pad}")
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"out_dtype must be one of {_OUT_DTYPES}")
    if _backend.native_enabled(images_u8):
        return _backend.C().batch_augment(images_u8, labels_i64, idx_i32,
                                          aug_i32, lut_f32, pad,
                                          channels_last, out_dtype)
    return _batch_augment_torch(images_u8, labels_i64, idx_i32, aug_i32,
                                lut_f32, pad, channels_last, out_dtype)
