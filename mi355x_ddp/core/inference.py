"""Fused evaluation forward (`--fused_eval`).

    model.eval()
    with fused_inference(model):
        logits = model(images)     # conv + BN (+ add) (+ ReLU): one kernel

On entry every (conv, BatchNorm) pair of the ResNet gets its eval-mode BN
folded into two per-channel tables (`ops.fused_eval.fold_bn`), hung on the
BatchNorm module; `models.resnet.conv_bn` then runs the pair as one
`conv_bn_act`. On exit, also by an exception, the tables are removed, and the
model is what it was: no parameter or buffer is written, and the mode of no
module is changed. The tables are built from the weights and running
statistics the model holds at entry, so enter it inside `WeightEMA.swapped()`
to evaluate the averages.

A BatchNorm that is training (or keeps no running statistics) is not folded
and runs as it always does. Nested use is one fold. Under `nn.DataParallel`
the context does nothing, with one warning: the replicas would share the
tables of device 0.
"""
from __future__ import annotations

import contextlib
import warnings

import torch.nn as nn

from ..models.resnet import conv_bn_pairs
from ..ops.fused_eval import FOLDED_ATTR, fold_bn

_DEPTH_ATTR = "_mi355x_fused_depth"
_warned_dp = False


def _unwrap(model: nn.Module):
    """The bare module under FlatDDP / torch DDP wrappers; None under
    nn.DataParallel."""
    while True:
        if isinstance(model, nn.DataParallel):
            return None
        inner = getattr(model, "module", None)
        if not isinstance(inner, nn.Module):
            return model
        model = inner


def folded_modules(model: nn.Module):
    """The BatchNorm modules of `model` that carry folded tables now."""
    return [m for m in model.modules() if hasattr(m, FOLDED_ATTR)]


def _unfold(module: nn.Module) -> None:
    for m in folded_modules(module):
        delattr(m, FOLDED_ATTR)


@contextlib.contextmanager
def fused_inference(model: nn.Module):
    global _warned_dp
    module = _unwrap(model)
    if module is None:
        if not _warned_dp:
            warnings.warn("fused_inference does nothing under nn.DataParallel: "
                          "its replicas would share the folded tables of "
                          "device 0; the evaluation forward runs unfused")
            _warned_dp = True
        yield model
        return
    depth = getattr(module, _DEPTH_ATTR, 0)
    try:
        if depth == 0:
            for _, bn in conv_bn_pairs(module):
                if not bn.training and bn.running_mean is not None:
                    # a tensor set on a module that is no Parameter and no
                    # registered buffer is a plain attribute: state_dict(),
                    # .to() and the EMA's buffer list do not see it
                    object.__setattr__(bn, FOLDED_ATTR, fold_bn(bn))
        object.__setattr__(module, _DEPTH_ATTR, depth + 1)
        yield model
    finally:
        if depth == 0:
            _unfold(module)
            if hasattr(module, _DEPTH_ATTR):
                delattr(module, _DEPTH_ATTR)
        else:
            object.__setattr__(module, _DEPTH_ATTR, depth)
