"""Fused multi-tensor SGD with momentum + weight decay.

MI355X-native replacement for the per-parameter ATen SGD step the reference
runs (optimizer at distributed.py:63; SURVEY.md §2.2 N9 calls this the
BASELINE north-star): ONE HIP kernel launch updates every parameter of the
model — ResNet18 has ~62 tensors, so the eager step's ~180 kernel launches
collapse to 1. Math matches torch.optim.SGD exactly:

    m <- mu*m + g + wd*p      (momentum buffer, damping 0)
    p <- p - lr*m

bf16 parameters (the apex-O2-equivalent ``amp="bf16_o2"`` mode, where the
MODEL lives in bf16 and no per-step autocast weight casts exist) get an
fp32 MASTER copy in the optimizer state: the update runs in fp32 against
the master and the bf16 parameter is its rounded copy —

    m <- mu*m + g + wd*master ; master <- master - lr*m ; p <- bf16(master)

Mixed models (some fp32, some bf16 tensors) split into the two paths.

Conv weight shadows (ops/conv.py): an fp32 conv weight used under 16-bit
autocast carries persistent copies in the autocast dtype, bf16 or fp16:
`w16` and the rotated `wT`. The native kernels here write parameters through
raw pointers, which the tensor's version counter does not see, so for every
parameter it updates that carries a shadow the step either rewrites the
shadow itself — the SGD kernel stores p_new rounded to the shadow's dtype
into `w16` next to `p` (per tensor: one step may carry bf16 and fp16
shadows), and one batched `multi_tensor_build_wT` launch rotates every `w16`
into its `wT` — or marks it stale. Never neither.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _backend
from .conv import WeightShadow, shadow_of, weight_shadows_wanted


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            p32, g32, m32, s32 = [], [], [], []
            p16, g16, w16, m16 = [], [], [], []
            momentum = group["momentum"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if p.dtype == torch.bfloat16:
                    if "master" not in state:
                        state["master"] = p.detach().float()
                    if momentum != 0 and "momentum_buffer" not in state:
                        state["momentum_buffer"] = torch.zeros_like(
                            state["master"])
                    p16.append(p)
                    g16.append(p.grad)
                    w16.append(state["master"])
                    if momentum != 0:
                        m16.append(state["momentum_buffer"])
                else:
                    if momentum != 0 and "momentum_buffer" not in state:
                        state["momentum_buffer"] = torch.zeros_like(p)
                    p32.append(p)
                    g32.append(p.grad)
                    s32.append(shadow_of(p))
                    if momentum != 0:
                        m32.append(state["momentum_buffer"])
            if p32:
                fused_sgd_step(p32, g32, m32 if momentum != 0 else None,
                               lr=group["lr"], momentum=momentum,
                               weight_decay=group["weight_decay"],
                               shadows=s32)
            if p16:
                fused_sgd_o2_step(p16, g16, w16,
                                  m16 if momentum != 0 else None,
                                  lr=group["lr"], momentum=momentum,
                                  weight_decay=group["weight_decay"])
        return loss


def fused_sgd_step(params: List[torch.Tensor], grads: List[torch.Tensor],
                   momentum_bufs: Optional[List[torch.Tensor]],
                   lr: float, momentum: float, weight_decay: float,
                   shadows: Optional[List[Optional[WeightShadow]]] = None
                   ) -> None:
    """`shadows[i]` is params[i]'s WeightShadow or None. Each one is either
    rewritten with the new weight here (native path) or invalidated."""
    live = []
    for p, sh in zip(params, shadows or ()):
        if sh is None:
            continue
        if weight_shadows_wanted() and sh.matches(p):
            live.append((p, sh))
        else:
            sh.invalidate()
    if params and _backend.native_enabled(params[0]):
        w16s = []
        if live:
            keep = {id(sh) for _, sh in live}
            w16s = [sh.w16 if sh is not None and id(sh) in keep else None
                    for sh in shadows]
        _backend.C().multi_tensor_sgd(params, grads,
                                      momentum_bufs if momentum_bufs is not None else [],
                                      lr, momentum, weight_decay, w16s)
        if live:
            _backend.C().multi_tensor_build_wT([sh.w16 for _, sh in live],
                                               [sh.wT for _, sh in live])
            for p, sh in live:
                sh.mark_fresh(p)
        return
    for _, sh in live:
        sh.invalidate()
    # torch fallback, same math (used on CPU and for parity tests)
    for i, (p, g) in enumerate(zip(params, grads)):
        if weight_decay != 0:
            g = g.add(p, alpha=weight_decay)
        if momentum_bufs is not None:
            buf = momentum_bufs[i]
            buf.mul_(momentum).add_(g)
            g = buf
        p.add_(g, alpha=-lr)


def fused_sgd_o2_step(params: List[torch.Tensor], grads: List[torch.Tensor],
                      masters: List[torch.Tensor],
                      momentum_bufs: Optional[List[torch.Tensor]],
                      lr: float, momentum: float, weight_decay: float) -> None:
    """bf16 params/grads, fp32 master + momentum (apex-O2 update)."""
    if params and _backend.native_enabled(params[0]):
        _backend.C().multi_tensor_sgd_o2(
            params, grads, masters,
            momentum_bufs if momentum_bufs is not None else [],
            lr, momentum, weight_decay)
        return
    for i, (p, g, w) in enumerate(zip(params, grads, masters)):
        gf = g.float()
        if weight_decay != 0:
            gf = gf.add(w, alpha=weight_decay)
        if momentum_bufs is not None:
            buf = momentum_bufs[i]
            buf.mul_(momentum).add_(gf)
            gf = buf
        w.add_(gf, alpha=-lr)
        p.copy_(w)
