"""Evaluation forward: conv + BatchNorm (+ add) (+ ReLU) as one kernel.

In eval mode BatchNorm is a per-channel affine map of the conv output, so it
can be applied to the conv's fp32 accumulator before that is rounded:

    out = round(relu(acc * scale[k] + shift[k] + residual))

`fold_bn` builds the two tables once per evaluation with plain torch ops;
`conv_bn_act` runs the conv with them. On a GPU, where `MI355Conv2d.forward`
would run the forward igemm kernel, it runs that kernel's BN-epilogue sibling
(`conv_fwd_bn_igemm`, csrc/conv_igemm.hip): one launch and one write of the
activation where the unfused chain takes five launches and three passes. A
layer the igemm kernels do not take today (fp32, NCHW, ``MI355X_NATIVE_CONV=0``)
runs the ops it runs today. On CPU tensors `conv_bn_act` is its torch
definition, so the whole feature is testable without a GPU.

Inference only: nothing here records an autograd graph.

Autotune. The choice is cached per ``("fwd_bn", dtype, x.shape, w.shape,
stride, pad, has_residual)``: the fused kernel at tiles 64, 128 and 128x128,
the split-K forms `splitk_candidates` offers for the plain forward, and one
`UNFUSED` candidate, today's conv (with its own tuned choice, MIOpen included)
followed by `bn_fwd_apply` on the folded tables, so that a layer is never
slower than it is without this module. With the tuner off the fused kernel
runs at the heuristic tile.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend
from .batchnorm import _run_fused
from .conv import (MI355Conv2d, TILE_128X128, UNFUSED, _cu_count, _tune_key,
                   _tuned_choice, splitk_candidates)

FOLDED_ATTR = "_mi355x_folded"   # where core/inference.py hangs the tables


class CallCounter:
    """How `conv_bn_act` ran its calls since the last `reset()`: `fused` on
    the BN-epilogue kernel, `unfused` on the tuner's UNFUSED candidate,
    `fallback` on the ops of a layer the igemm kernels do not take (GPU) or on
    the torch definition (CPU). Measuring runs of the tuner are not counted."""

    __slots__ = ("fused", "unfused", "fallback")

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self.fused = self.unfused = self.fallback = 0


calls = CallCounter()


@torch.no_grad()
def fold_bn(bn: nn.Module) -> torch.Tensor:
    """fp32 ``[4][C]`` = {mean, invstd, scale, shift} of a BatchNorm in eval
    mode, the layout `bn_fwd_apply` reads (rows 2 and 3):

        scale = gamma * rsqrt(running_var + eps)
        shift = beta - running_mean * scale

    Every input is widened to fp32 first (`bf16_o2` keeps bf16 affine
    parameters). `MI355SyncBatchNorm` folds the same way: in eval mode it
    does not communicate."""
    if not isinstance(bn, nn.modules.batchnorm._BatchNorm):
        raise TypeError(f"fold_bn expects a BatchNorm module, got {type(bn)}")
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError("fold_bn needs running statistics: a BatchNorm "
                         "without them normalizes by the batch in eval mode "
                         "too")
    if bn.training:
        raise ValueError("fold_bn expects a BatchNorm in eval mode: in "
                         "training it normalizes by the batch statistics")
    mean = bn.running_mean.float()
    invstd = torch.rsqrt(bn.running_var.float() + bn.eps)
    scale = invstd if bn.weight is None else bn.weight.float() * invstd
    shift = -mean * scale
    if bn.bias is not None:
        shift = bn.bias.float() + shift
    return torch.stack([mean, invstd, scale, shift]).contiguous()


def _torch_definition(x, conv, folded, relu, residual):
    shape = (1, -1, 1, 1)
    y = F.conv2d(x.float(), conv.weight.float(), None, conv.stride,
                 conv.padding, conv.dilation, conv.groups)
    y = y * folded[2].view(shape) + folded[3].view(shape)
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


@torch.no_grad()
def conv_bn_act(x: torch.Tensor, conv: nn.Conv2d, folded: torch.Tensor,
                relu: bool, residual: Optional[torch.Tensor] = None,
                bn: Optional[nn.Module] = None) -> torch.Tensor:
    """``relu(conv(x) * scale + shift + residual)`` with `folded` from
    `fold_bn` (relu and residual optional). `bn`, the module `folded` came
    from, is used only by a GPU layer that falls back to today's ops, which
    then are exactly `bn_relu` / `bn_add_relu` on it."""
    if conv.bias is not None:
        raise ValueError("conv_bn_act expects a bias-free conv")
    if not x.is_cuda:
        calls.fallback += 1
        return _torch_definition(x, conv, folded, relu, residual)
    ops = conv.native_operands(x) if isinstance(conv, MI355Conv2d) else None
    if ops is None:
        calls.fallback += 1
        y = conv(x)
        if bn is not None:
            return _run_fused(y, residual, bn, relu)
        shape = (1, -1, 1, 1)
        out = y.float() * folded[2].view(shape) + folded[3].view(shape)
        if residual is not None:
            out = out + residual.float()
        return (torch.relu(out) if relu else out).to(y.dtype)

    xx, w16 = ops
    C = _backend.C()
    stride, pad = conv.stride[0], conv.padding[0]
    if residual is not None:
        residual = residual.contiguous(memory_format=torch.channels_last)

    def run(t):
        if t == UNFUSED:
            return C.bn_fwd_apply(conv(x), folded, relu, residual)
        tile, nz = t if isinstance(t, tuple) else (t, 1)
        return C.conv_fwd_bn_igemm(xx, w16, folded, residual, relu, stride,
                                   pad, tile, nz)

    key = _tune_key("fwd_bn", xx.dtype, xx.shape, w16.shape, stride, pad,
                    residual is not None)

    def cands():
        # bn_fwd_apply is the vectorised kernel: 8 channels per thread
        unfused = (UNFUSED,) if w16.shape[0] % 8 == 0 else ()
        return (64, 128, TILE_128X128) + splitk_candidates(
            "fwd", xx.shape, w16.shape, stride, pad, _cu_count(xx)) + unfused

    choice = _tuned_choice(key, cands, run, default=0)
    if choice == UNFUSED:
        calls.unfused += 1
    else:
        calls.fused += 1
    return run(choice)
