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

CutMix (``batch_augment_cutmix``, tables from ``draw_cutmix_params``): with
``p = mix[i, 0]`` and the box of ``mix[i]``, output pixel (n, c, h, w) is
``augmented(p)[c, h, w]`` when ``p`` is in [0, M) and (h, w) is in the box,
else ``augmented(i)[c, h, w]``, where ``augmented(k)`` is the definition above
for dataset index ``k`` with ``aug[k]``: the partner gets its own crop and
flip. ``labels_b`` is the partner's label and ``lam`` the sample's share of
the area; an unmixed row has ``labels_b == labels_a`` and ``lam == 1``. Still a
table lookup per element, so kernel and torch definition agree bit for bit.
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


# salt of the CutMix generator: keeps its stream apart from draw_aug_params
# (seed * 1_000_003 + epoch) for every (seed, epoch)
_CUTMIX_SALT = 0x43754D78


def draw_cutmix_params(n: int, H: int, W: int, alpha: float, prob: float,
                       seed: int, epoch: int,
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mix int32 [n, 3], lam float32 [n]), one row per DATASET index, from a
    numpy Generator of its own seeded by (seed, epoch, salt), so
    ``draw_aug_params`` draws what it always drew.

    ``mix[i] = (partner, y0 | y1 << 16, x0 | x1 << 16)``: ``partner`` is a
    dataset index in [0, n), or -1 for "not mixed" (a row is mixed with
    probability ``prob``). The box is the usual CutMix box in output
    coordinates with exclusive ends: ``l0 ~ Beta(alpha, alpha)``, sides
    ``floor((H, W) * sqrt(1 - l0))``, centre uniform over the image, clipped
    to it. ``lam[i] = 1 - area / (H * W)`` from the clipped box, in float64
    rounded once to fp32; 1 for unmixed rows. An empty box and ``partner ==
    i`` are legal. Every draw is made for every row whether it is mixed or
    not, so a row's box does not depend on ``prob``."""
    import numpy as np
    if not alpha > 0:
        raise ValueError(f"alpha must be > 0, got {alpha}")
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"prob must be in [0, 1], got {prob}")
    if not (1 <= H < 1 << 16 and 1 <= W < 1 << 16):
        raise ValueError(f"H and W must be in [1, 65535], got {H}x{W}")
    rng = np.random.default_rng([int(seed), int(epoch), _CUTMIX_SALT])
    mixed = rng.random(n) < prob
    partner = rng.integers(0, n, size=n)
    l0 = rng.beta(alpha, alpha, size=n)
    cy = rng.integers(0, H, size=n)
    cx = rng.integers(0, W, size=n)
    ratio = np.sqrt(1.0 - l0)
    cut_h = np.floor(H * ratio).astype(np.int64)
    cut_w = np.floor(W * ratio).astype(np.int64)
    y0 = np.clip(cy - cut_h // 2, 0, H)
    y1 = np.clip(cy + cut_h // 2, 0, H)
    x0 = np.clip(cx - cut_w // 2, 0, W)
    x1 = np.clip(cx + cut_w // 2, 0, W)
    area = (y1 - y0) * (x1 - x0)
    lam = np.where(mixed, 1.0 - area.astype(np.float64) / float(H * W), 1.0)
    mix = np.stack([np.where(mixed, partner, -1), y0 | (y1 << 16),
                    x0 | (x1 << 16)], axis=1)
    return (torch.from_numpy(mix.astype(np.int32)),
            torch.from_numpy(lam.astype(np.float32)))


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


def _check_batch_args(images_u8, idx_i32, pad, out_dtype):
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


def batch_augment(images_u8: torch.Tensor, labels_i64: torch.Tensor,
                  idx_i32: torch.Tensor, aug_i32: Optional[torch.Tensor],
                  lut_f32: torch.Tensor, pad: int = 4,
                  channels_last: bool = False,
                  out_dtype: torch.dtype = torch.float32,
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(images [N,3,H,W] in ``out_dtype``, labels [N]) for the dataset indices
    ``idx_i32``; see the module docstring for the definition."""
    _check_batch_args(images_u8, idx_i32, pad, out_dtype)
    if _backend.native_enabled(images_u8):
        return _backend.C().batch_augment(images_u8, labels_i64, idx_i32,
                                          aug_i32, lut_f32, pad,
                                          channels_last, out_dtype)
    return _batch_augment_torch(images_u8, labels_i64, idx_i32, aug_i32,
                                lut_f32, pad, channels_last, out_dtype)


def _batch_augment_cutmix_torch(images_u8, labels_i64, idx_i32, aug_i32,
                                mix_i32, lam_f32, lut_f32, pad, channels_last,
                                out_dtype):
    """The CutMix definition: the sample and its partner each augmented by
    ``_batch_augment_torch`` with their own ``aug`` word, the partner's pixels
    inside the box. Returns (images, labels_a, labels_b, lam)."""
    M, H, W, _ = images_u8.shape
    dev = images_u8.device
    idx = idx_i32.long()
    m = mix_i32[idx].long()                                          # [N,3]
    partner = m[:, 0]
    mixed = (partner >= 0) & (partner < M)
    partner = torch.where(mixed, partner, idx)
    out_a, labels_a = _batch_augment_torch(
        images_u8, labels_i64, idx_i32, aug_i32, lut_f32, pad, channels_last,
        out_dtype)
    out_b, labels_b = _batch_augment_torch(
        images_u8, labels_i64, partner.to(torch.int32), aug_i32, lut_f32, pad,
        channels_last, out_dtype)
    y0, y1 = m[:, 1] & 0xffff, (m[:, 1] >> 16) & 0xffff
    x0, x1 = m[:, 2] & 0xffff, (m[:, 2] >> 16) & 0xffff
    hh = torch.arange(H, device=dev)[None, :]
    ww = torch.arange(W, device=dev)[None, :]
    box = (((hh >= y0[:, None]) & (hh < y1[:, None]))[:, :, None]
           & ((ww >= x0[:, None]) & (ww < x1[:, None]))[:, None, :])  # [N,H,W]
    box = box & mixed[:, None, None]
    out = torch.where(box[:, None], out_b, out_a)
    out = out.contiguous(memory_format=torch.channels_last if channels_last
                         else torch.contiguous_format)
    lam = torch.where(mixed, lam_f32[idx], torch.ones_like(lam_f32[idx]))
    return out, labels_a, labels_b, lam


def batch_augment_cutmix(images_u8: torch.Tensor, labels_i64: torch.Tensor,
                         idx_i32: torch.Tensor,
                         aug_i32: Optional[torch.Tensor],
                         mix_i32: torch.Tensor, lam_f32: torch.Tensor,
                         lut_f32: torch.Tensor, pad: int = 4,
                         channels_last: bool = False,
                         out_dtype: torch.dtype = torch.float32,
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                    torch.Tensor]:
    """``batch_augment`` with a CutMix box per sample (tables from
    ``draw_cutmix_params``): (images, labels_a, labels_b [N] int64, lam [N]
    fp32). ``labels_b`` is the partner's label and ``lam`` the sample's share
    of the image; an unmixed row has ``labels_b == labels_a`` and ``lam ==
    1``."""
    _check_batch_args(images_u8, idx_i32, pad, out_dtype)
    M = images_u8.shape[0]
    if mix_i32.dtype != torch.int32 or tuple(mix_i32.shape) != (M, 3):
        raise ValueError("mix_i32 must be an int32 [M, 3] tensor, got "
                         f"{mix_i32.dtype} {tuple(mix_i32.shape)}")
    if lam_f32.dtype != torch.float32 or tuple(lam_f32.shape) != (M,):
        raise ValueError("lam_f32 must be a float32 [M] tensor, got "
                         f"{lam_f32.dtype} {tuple(lam_f32.shape)}")
    if _backend.native_enabled(images_u8):
        return _backend.C().batch_augment_cutmix(
            images_u8, labels_i64, idx_i32, aug_i32, mix_i32, lam_f32,
            lut_f32, pad, channels_last, out_dtype)
    return _batch_augment_cutmix_torch(images_u8, labels_i64, idx_i32,
                                       aug_i32, mix_i32, lam_f32, lut_f32,
                                       pad, channels_last, out_dtype)
