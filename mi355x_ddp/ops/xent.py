"""Fused softmax + cross-entropy (reference: nn.CrossEntropyLoss at distributed.py:61).

One HIP kernel computes the row max, log-sum-exp and NLL in a single pass
(ATen launches softmax + nll separately); backward is one kernel producing
softmax(x) - onehot scaled by 1/N. CPU fallback is the same math in torch.

Beyond the reference: a two-label, label-smoothed form for CutMix targets
(``xent_mix_fwd`` / ``xent_mix_bwd``). For row r with classes a, b, weight l,
smoothing eps and C classes

    q_r     = (1-eps) * (l*x[r,a] + (1-l)*x[r,b]) + (eps/C) * sum_j x[r,j]
    loss    = mean_r (lse_r - q_r)
    dx[r,j] = (softmax(x_r)[j] - (1-eps)*(l*[j==a] + (1-l)*[j==b]) - eps/C)
              * dloss / N

which is l*CE(x,a) + (1-l)*CE(x,b) with torch's ``label_smoothing=eps``. With
l = 1 and eps = 0 it is the plain loss bit for bit (1*xa + 0*xb + 0*sum == xa).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _backend


class _SoftmaxXentFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        logits = logits.contiguous()
        if _backend.native_enabled(logits):
            loss, lse = _backend.C().xent_fwd(logits, target)
        else:
            lf = logits.float()
            lse = torch.logsumexp(lf, dim=1)
            loss = (lse - lf.gather(1, target.view(-1, 1)).squeeze(1)).mean()
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target, lse = ctx.saved_tensors
        if _backend.native_enabled(logits):
            dx = _backend.C().xent_bwd(logits, target, lse, dloss)
        else:
            lf = logits.float()
            p = torch.exp(lf - lse.unsqueeze(1))
            p.scatter_add_(1, target.view(-1, 1),
                           torch.full_like(target.view(-1, 1), -1.0, dtype=p.dtype))
            dx = (p * (dloss.float() / logits.shape[0])).to(logits.dtype)
        return dx, None


class _SoftmaxXentMixFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target_a, target_b, lam, eps):
        logits = logits.contiguous()
        if _backend.native_enabled(logits):
            loss, lse = _backend.C().xent_mix_fwd(logits, target_a, target_b,
                                                  lam, eps)
        else:
            lf = logits.float()
            lse = torch.logsumexp(lf, dim=1)
            xa = lf.gather(1, target_a.view(-1, 1)).squeeze(1)
            xb = lf.gather(1, target_b.view(-1, 1)).squeeze(1)
            q = (1.0 - eps) * (lam * xa + (1.0 - lam) * xb) \
                + (eps / lf.shape[1]) * lf.sum(dim=1)
            loss = (lse - q).mean()
        ctx.save_for_backward(logits, target_a, target_b, lam, lse)
        ctx.eps = eps
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target_a, target_b, lam, lse = ctx.saved_tensors
        eps = ctx.eps
        if _backend.native_enabled(logits):
            dx = _backend.C().xent_mix_bwd(logits, target_a, target_b, lam,
                                           lse, dloss, eps)
        else:
            lf = logits.float()
            p = torch.exp(lf - lse.unsqueeze(1))
            # a == b: both one-hots add
            p.scatter_add_(1, target_a.view(-1, 1),
                           (-(1.0 - eps) * lam).view(-1, 1))
            p.scatter_add_(1, target_b.view(-1, 1),
                           (-(1.0 - eps) * (1.0 - lam)).view(-1, 1))
            p -= eps / lf.shape[1]
            dx = (p * (dloss.float() / logits.shape[0])).to(logits.dtype)
        return dx, None, None, None, None


def softmax_cross_entropy(logits: torch.Tensor, target: torch.Tensor,
                          target_b: Optional[torch.Tensor] = None,
                          lam: Optional[torch.Tensor] = None,
                          label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean-reduced cross entropy over a (N, classes) logits tensor.

    With ``target_b`` and ``lam`` (fp32 [N]) the per-row loss is
    ``lam*CE(x, target) + (1-lam)*CE(x, target_b)``; ``label_smoothing`` has
    torch's meaning. With neither, the plain one-label kernels run."""
    label_smoothing = float(label_smoothing)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError("label_smoothing must be in [0, 1), got "
                         f"{label_smoothing}")
    if (target_b is None) != (lam is None):
        raise ValueError("target_b and lam go together: pass both or neither")
    if target_b is None and label_smoothing == 0.0:
        return _SoftmaxXentFunction.apply(logits, target)
    if target_b is None:
        target_b = target
        lam = torch.ones(target.shape[0], dtype=torch.float32,
                         device=logits.device)
    if lam.dtype != torch.float32:
        raise ValueError(f"lam must be float32, got {lam.dtype}")
    if not (target.shape == target_b.shape == lam.shape
            == (logits.shape[0],)):
        raise ValueError("target, target_b and lam must be [N] for [N, C] "
                         "logits")
    return _SoftmaxXentMixFunction.apply(
        logits, target.contiguous(), target_b.contiguous(), lam.contiguous(),
        label_smoothing)


class SoftmaxCrossEntropy(torch.nn.Module):
    """Drop-in for nn.CrossEntropyLoss(reduction='mean') on 2D logits.

    ``target`` is a class-index tensor or a CutMix ``(labels_a, labels_b,
    lam)`` tuple. As with nn.CrossEntropyLoss, ``label_smoothing`` applies
    whenever the module is called, validation included."""

    def __init__(self, label_smoothing: float = 0.0):
        super().__init__()
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError("label_smoothing must be in [0, 1), got "
                             f"{label_smoothing}")
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits, target):
        if isinstance(target, (tuple, list)):
            labels_a, labels_b, lam = target
            return softmax_cross_entropy(logits, labels_a, labels_b, lam,
                                         self.label_smoothing)
        return softmax_cross_entropy(logits, target,
                                     label_smoothing=self.label_smoothing)
