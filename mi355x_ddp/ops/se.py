"""Squeeze-and-Excitation (Hu et al. 2018) joined with the residual add:

    s = mean_hw(u)                                  [N, C]
    g = sigmoid(fc2(relu(fc1(s))))                  [N, C]
    out = relu(u * g[:, :, None, None] + identity)

`se_add_relu` is ONE autograd Function with the native path (the seven kernels
of csrc/se_block.hip: three forward, four backward) and the torch definition
in one implementation, like ops/batchnorm.py. The gate path is fp32 on both:
`s`, `h`, `g`, their gradients and the parameter gradients never pass through
a 16-bit value, and the native kernels read the fp32 parameters as they are.

The native path runs when `_backend.native_enabled(u)`, `u` and `identity`
are bf16 or fp16 channels_last of one shape, `C % 8 == 0`, the reduced width
is at most 512 and the four parameters are fp32; `MI355X_NATIVE_SE=0` is the
A/B switch. Everything else (the CPU, `MI355X_FORCE_FALLBACK=1`, 16-bit
parameters under `--amp bf16_o2`, fp32 or NCHW activations) runs the torch
definition. `se_calls` counts the native forward and backward calls.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _backend
from .conv import _Calls

_NATIVE_DTYPES = (torch.bfloat16, torch.float16)
_MAX_REDUCED = 512   # MAX_CR of csrc/se_block.hip


class _SECalls(_Calls):
    def reset(self) -> None:
        self.fwd = self.bwd = 0


se_calls = _SECalls()


def native_se_wanted() -> bool:
    return os.environ.get("MI355X_NATIVE_SE", "1") == "1"


def _native_ok(u, identity, w1, b1, w2, b2) -> bool:
    if not native_se_wanted() or not _backend.native_enabled(u):
        return False
    if u.dtype not in _NATIVE_DTYPES or u.dim() != 4 or u.shape[1] % 8 != 0:
        return False
    if identity.dtype != u.dtype or identity.shape != u.shape:
        return False
    if not u.is_contiguous(memory_format=torch.channels_last):
        return False
    if w1.shape[0] > _MAX_REDUCED:
        return False
    return all(p.dtype == torch.float32 and p.is_cuda
               for p in (w1, b1, w2, b2))


class _SEAddReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, identity, w1, b1, w2, b2):
        ctx.native = _native_ok(u, identity, w1, b1, w2, b2)
        ctx.identity_dtype = identity.dtype
        if ctx.native:
            C_ = _backend.C()
            cl = torch.channels_last
            u = u.contiguous(memory_format=cl)
            identity = identity.contiguous(memory_format=cl)
            w1, b1, w2, b2 = (p.contiguous() for p in (w1, b1, w2, b2))
            s = C_.se_squeeze(u)
            h, g = C_.se_excite_fwd(s, w1, b1, w2, b2)
            out = C_.se_scale_add_relu(u, identity, g)
            se_calls.fwd += 1
            ctx.save_for_backward(u, out, s, h, g, w1, w2)
            return out
        # the torch definition; 16-bit activations take the gate path in fp32
        ct = torch.float32 if u.dtype in _NATIVE_DTYPES else u.dtype
        with torch.autocast(u.device.type, enabled=False):
            uf = u.to(ct)
            s = uf.mean(dim=(2, 3))
            h = torch.relu(s @ w1.to(ct).t() + b1.to(ct))
            g = torch.sigmoid(h @ w2.to(ct).t() + b2.to(ct))
            out = torch.relu(uf * g[:, :, None, None] + identity.to(ct))
            out = out.to(u.dtype)
        ctx.save_for_backward(u, out, s, h, g, w1, w2)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, out, s, h, g, w1, w2 = ctx.saved_tensors
        if ctx.native:
            C_ = _backend.C()
            dout = dout.contiguous(memory_format=torch.channels_last)
            dg = C_.se_join_bwd_reduce(dout, out, u)
            dz2, dz1, ds = C_.se_excite_bwd(dg, g, h, w1, w2)
            dw1, db1, dw2, db2 = C_.se_excite_wgrad(dz2, h, dz1, s)
            du, did = C_.se_join_bwd_apply(dout, out, g, ds)
            se_calls.bwd += 1
            return du, did, dw1, db1, dw2, db2
        ct = s.dtype
        with torch.autocast(u.device.type, enabled=False):
            d = dout.to(ct) * (out > 0)
            dg = (d * u.to(ct)).sum(dim=(2, 3))
            dz2 = dg * g * (1 - g)
            dz1 = (dz2 @ w2.to(ct)) * (h > 0)
            ds = dz1 @ w1.to(ct)
            hw = u.shape[2] * u.shape[3]
            du = d * g[:, :, None, None] + ds[:, :, None, None] / hw
            return (du.to(u.dtype), d.to(ctx.identity_dtype),
                    (dz1.t() @ s).to(w1.dtype), dz1.sum(0).to(w1.dtype),
                    (dz2.t() @ h).to(w2.dtype), dz2.sum(0).to(w2.dtype))


class SqueezeExcite(nn.Module):
    """The gate's parameters: `fc1 = Linear(C, Cr)`, `fc2 = Linear(Cr, C)`,
    `Cr = max(C // reduction, 1)`. Plain Linear modules, so checkpoints get
    plain keys and the optimizers, EMA and FlatDDP see ordinary 2-D and 1-D
    parameters. `forward(u)` is the gate alone, in torch; the models run
    `se_add_relu`, which reads the parameters."""

    def __init__(self, channels: int, reduction: int = 16):
        super().__init__()
        reduced = max(channels // reduction, 1)
        self.fc1 = nn.Linear(channels, reduced)
        self.fc2 = nn.Linear(reduced, channels)

    def forward(self, u):
        s = u.float().mean(dim=(2, 3))
        g = torch.sigmoid(self.fc2(torch.relu(self.fc1(s))))
        return (u * g[:, :, None, None]).to(u.dtype)


def se_add_relu(u: torch.Tensor, identity: torch.Tensor,
                se: SqueezeExcite) -> torch.Tensor:
    """relu(u * gate(u) + identity) with the gate of `se`."""
    return _SEAddReLU.apply(u, identity, se.fc1.weight, se.fc1.bias,
                            se.fc2.weight, se.fc2.bias)
