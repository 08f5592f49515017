"""Group Normalization (Wu & He 2018) joined with the residual add and ReLU:

    y = act(group_norm(x, G, gamma, beta) (+ residual))

`gn_relu` and `gn_add_relu` are ONE autograd Function with the native path
(csrc/group_norm.hip: one forward launch, one backward launch and a small
reduce) and the torch definition in one implementation, like ops/se.py. The
statistics are per sample: there is no collective, no running statistic, and
training and evaluation are the same function. Everything between the 16-bit
operands and the 16-bit result is fp32 on both paths.

The native path runs when `_backend.native_enabled(x)`, `x` (and `residual`)
are bf16 or fp16 channels_last, `C % 8 == 0`, the channels per group are 2, 4,
8, 16, 32 or 64 and gamma and beta are fp32; `MI355X_NATIVE_GN=0` is the A/B
switch. Everything else (the CPU, `MI355X_FORCE_FALLBACK=1`, 16-bit parameters
under `--amp bf16_o2`, fp32 or NCHW activations, other group widths) runs the
torch definition. `MI355X_GN_RESIDENT=0` makes the native kernels stream from
global memory instead of keeping a block's slice in LDS; the results are
bit-identical. `gn_calls` counts the native forward and backward calls.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from . import _backend
from .conv import _Calls

_NATIVE_DTYPES = (torch.bfloat16, torch.float16)
_GROUP_WIDTHS = (2, 4, 8, 16, 32, 64)   # check_groups of csrc/group_norm.hip


class _GNCalls(_Calls):
    def reset(self) -> None:
        self.fwd = self.bwd = 0


gn_calls = _GNCalls()


def native_gn_wanted() -> bool:
    return os.environ.get("MI355X_NATIVE_GN", "1") != "0"


def _native_ok(x, residual, gamma, beta, groups: int) -> bool:
    if not native_gn_wanted() or not _backend.native_enabled(x):
        return False
    if x.dtype not in _NATIVE_DTYPES or x.dim() != 4 or x.shape[1] % 8 != 0:
        return False
    if x.shape[1] % groups or x.shape[1] // groups not in _GROUP_WIDTHS:
        return False
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    if residual is not None and (residual.dtype != x.dtype or
                                 residual.shape != x.shape):
        return False
    return all(p is not None and p.dtype == torch.float32 and p.is_cuda
               for p in (gamma, beta))


def _xhat(x, mean, rstd, groups: int):
    N = x.shape[0]
    xg = x.to(mean.dtype).reshape(N, groups, -1)
    return ((xg - mean[:, :, None]) * rstd[:, :, None]).reshape(x.shape)


class _GroupNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, groups, eps, relu):
        ctx.native = _native_ok(x, residual, gamma, beta, groups)
        ctx.groups, ctx.relu = groups, relu
        ctx.residual_dtype = None if residual is None else residual.dtype
        if ctx.native:
            cl = torch.channels_last
            if residual is not None:
                residual = residual.contiguous(memory_format=cl)
            gamma = gamma.contiguous()
            y, mean, rstd = _backend.C().gn_fwd(
                x, gamma, beta.contiguous(), residual, groups, eps, relu)
            gn_calls.fwd += 1
            ctx.save_for_backward(x, y, mean, rstd, gamma)
            return y
        # the torch definition; 16-bit activations are normalized in fp32
        ct = torch.float32 if x.dtype in _NATIVE_DTYPES else x.dtype
        with torch.autocast(x.device.type, enabled=False):
            N, C = x.shape[:2]
            y, mean, rstd = torch.native_group_norm(
                x.to(ct).contiguous(), gamma.to(ct), beta.to(ct), N, C,
                x.numel() // (N * C), groups, eps)
            if residual is not None:
                y = y + residual.to(ct)
            if relu:
                y = torch.relu(y)
            y = y.to(x.dtype)
            if x.dim() == 4 and x.is_contiguous(
                    memory_format=torch.channels_last):
                y = y.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x, y, mean, rstd, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd, gamma = ctx.saved_tensors
        has_res = ctx.residual_dtype is not None
        if ctx.native:
            dy = dy.contiguous(memory_format=torch.channels_last)
            dx, dres, dgamma, dbeta = _backend.C().gn_bwd(
                dy, y, x, mean, rstd, gamma, ctx.groups, ctx.relu, has_res)
            gn_calls.bwd += 1
            return dx, dres, dgamma, dbeta, None, None, None
        ct = mean.dtype
        with torch.autocast(x.device.type, enabled=False):
            N, G = x.shape[0], ctx.groups
            g = dy.to(ct)
            if ctx.relu:
                g = g * (y > 0)
            xhat = _xhat(x, mean, rstd, G)
            dgamma = (g * xhat).sum(dim=(0, 2, 3))
            dbeta = g.sum(dim=(0, 2, 3))
            dxhat = g * gamma.to(ct)[None, :, None, None]
            s1 = dxhat.reshape(N, G, -1).mean(-1)[:, :, None]
            s2 = (dxhat * xhat).reshape(N, G, -1).mean(-1)[:, :, None]
            dx = (dxhat.reshape(N, G, -1) - s1
                  - xhat.reshape(N, G, -1) * s2) * rstd[:, :, None]
            dx = dx.reshape(x.shape).to(x.dtype)
            if x.is_contiguous(memory_format=torch.channels_last):
                dx = dx.contiguous(memory_format=torch.channels_last)
            return (dx, g.to(ctx.residual_dtype) if has_res else None,
                    dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None, None,
                    None)


def _apply(x, residual: Optional[torch.Tensor], gn: nn.GroupNorm, relu: bool):
    if gn.weight is None:
        raise ValueError("gn_relu needs an affine nn.GroupNorm")
    return _GroupNormAct.apply(x, residual, gn.weight, gn.bias, gn.num_groups,
                               gn.eps, relu)


def gn_relu(x: torch.Tensor, gn: nn.GroupNorm,
            relu: bool = True) -> torch.Tensor:
    """relu(gn(x)), or gn(x) alone with `relu=False`."""
    return _apply(x, None, gn, relu)


def gn_add_relu(x: torch.Tensor, residual: torch.Tensor,
                gn: nn.GroupNorm) -> torch.Tensor:
    """relu(gn(x) + residual)."""
    return _apply(x, residual, gn, True)


def convert_group_norm(module: nn.Module, groups: int = 32) -> nn.Module:
    """Replace every `nn.BatchNorm2d` under `module` (those inside a
    `downsample` too) with `nn.GroupNorm(min(groups, C // 2), C)` on the same
    device and dtype. `min(groups, C // 2)` keeps at least two channels per
    group, so a 32-channel layer gets 16 groups at `groups=32`. Raises
    `ValueError` when that group count does not divide C."""
    if isinstance(module, nn.BatchNorm2d):
        C = module.num_features
        G = min(groups, C // 2)
        if G < 1 or C % G:
            raise ValueError(f"gn_groups={groups}: {G} groups do not divide "
                             f"the {C} channels of a norm layer")
        ref = module.weight if module.weight is not None \
            else module.running_mean
        kw = {} if ref is None else {"device": ref.device, "dtype": ref.dtype}
        return nn.GroupNorm(G, C, eps=module.eps, affine=module.affine, **kw)
    for name, child in module.named_children():
        new = convert_group_norm(child, groups)
        if new is not child:
            setattr(module, name, new)
    return module
