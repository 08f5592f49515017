"""GroupNorm on the kernels of csrc/group_norm.hip: `gn_relu` / `gn_add_relu`
against an fp64 CPU reference, the streaming variant against the LDS-resident
one, bit-reproducibility, host refusals and a GroupNorm ResNet-50 step.
profiles/group_norm.md has the measured errors of every case.
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mi355x_ddp.ops import gn_add_relu, gn_relu
from mi355x_ddp.ops.conv import MI355Conv2d
from mi355x_ddp.ops.groupnorm import gn_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}   # test_conv_grouped_gpu.py
DTYPES = [torch.bfloat16, torch.float16]
EPS = 1e-5

# (N, C, G, H, W)
CASES = [
    (3, 64, 32, 1, 1),     # Cg = 2, one pixel, four groups per lane
    (2, 72, 9, 7, 7),      # ragged last chunk, HW no multiple of the slots
    (1, 128, 8, 8, 8),     # Cg = 16 across two lanes, CAP = 64 exactly, N = 1
    (9, 64, 16, 5, 13),    # 65 px: past a capacity; 9 images: ragged reduce
    (2, 96, 3, 24, 24),    # Cg = 32, 576 px: last resident backward at CW 64
    (2, 64, 1, 32, 32),    # Cg = 64: forward resident, backward streaming
    (2, 64, 32, 32, 32),   # backward resident at CW = 32
    (2, 64, 8, 34, 34),    # streaming both ways
]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else None


def _formula(x, gamma, beta, G, idn):
    xg = x.reshape(x.shape[0], G, -1)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    xhat = ((xg - mean) / (var + EPS).sqrt()).reshape(x.shape)
    pre = xhat * gamma[None, :, None, None] + beta[None, :, None, None]
    return pre if idn is None else pre + idn


class _Case:
    """16-bit-rounded x, identity, dout and fp32 gamma, beta, and the fp64 CPU
    results of the plain formula on them. Built once, never written to.
    mode: "linear" gn(x); "relu" relu(gn(x)); "add_relu" relu(gn(x) + idn)."""

    def __init__(self, shape, dt, mode):
        N, C, G, H, W = shape
        # 19: the first seed base at which every "relu" case is off the kink
        gen = torch.Generator().manual_seed(19 + sum(shape))
        rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        self.gn = nn.GroupNorm(G, C, eps=EPS)
        with torch.no_grad():
            self.gn.weight.copy_(rnd(C))
            self.gn.bias.copy_(rnd(C))
        params = [p.detach().double().requires_grad_(True)
                  for p in self.gn.parameters()]
        # a mean of 3: a one-pass variance would show
        x = (rnd(N, C, H, W) + 3).to(dt).double().requires_grad_(True)
        dout = rnd(N, C, H, W).to(dt).double()
        idn = None
        if mode == "add_relu":
            # keep every pre-activation away from the ReLU's kink: the mask is
            # then never in question and no element is left out
            idn = rnd(N, C, H, W)
            pre = _formula(x, *params, G, idn).detach()
            idn += torch.where(pre.abs() < 0.05,
                               torch.where(pre < 0, -0.25, 0.25), 0.0)
            idn = idn.to(dt).double().requires_grad_(True)
        pre = _formula(x, *params, G, idn)
        if mode == "add_relu":
            assert pre.abs().min() > 0.03
        elif mode == "relu":   # nothing to nudge: the seed keeps it off
            assert pre.abs().min() > 1e-4
        out = pre if mode == "linear" else torch.relu(pre)
        wrt = {"dx": x, "dgamma": params[0], "dbeta": params[1]}
        if idn is not None:
            wrt["d_identity"] = idn
        grads = torch.autograd.grad(out, list(wrt.values()), dout)
        self.ref = dict(zip(wrt, grads), out=out.detach())
        self.dt, self.mode = dt, mode
        self.x, self.dout = (t.detach().to(DEV, dt).contiguous(
            memory_format=CL) for t in (x, dout))
        self.idn = None if idn is None else \
            idn.detach().to(DEV, dt).contiguous(memory_format=CL)
        self.floor = (N * H * W) ** 0.5 * 2.0 ** -24

    def run(self):
        """The results of the public op on the GPU operands, by name."""
        gn = copy.deepcopy(self.gn).to(DEV)
        x = self.x.clone().requires_grad_(True)
        got = {}
        if self.mode == "add_relu":
            idn = self.idn.clone().requires_grad_(True)
            out = gn_add_relu(x, idn, gn)
        else:
            out = gn_relu(x, gn, relu=self.mode == "relu")
        out.backward(self.dout)
        if self.mode == "add_relu":
            got["d_identity"] = idn.grad
        got.update(out=out.detach(), dx=x.grad, dgamma=gn.weight.grad,
                   dbeta=gn.bias.grad)
        return got


@functools.lru_cache(maxsize=None)
def _case(shape, dt, mode):
    return _Case(shape, dt, mode)


def _rel_err(got, ref):
    got = got.detach().double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def _check(monkeypatch, c, shape):
    gn_calls.reset()
    got = c.run()
    assert (gn_calls.fwd, gn_calls.bwd) == (1, 1)
    monkeypatch.setenv("MI355X_NATIVE_GN", "0")
    gn_calls.reset()
    torch_def = c.run()
    assert (gn_calls.fwd, gn_calls.bwd) == (0, 0)
    e = {k: _rel_err(v, c.ref[k]) for k, v in got.items()}
    e_torch = {k: _rel_err(v, c.ref[k]) for k, v in torch_def.items()}
    print("gn", _ids(shape), _ids(c.dt), c.mode, "native",
          " ".join(f"{k} {v:.2e}" for k, v in e.items()), "| torch",
          " ".join(f"{k} {v:.2e}" for k, v in e_torch.items()))
    for k, v in got.items():
        if k in ("dgamma", "dbeta"):
            assert v.dtype == torch.float32
            assert e[k] <= max(4 * e_torch[k], c.floor), (k, e, e_torch)
        else:
            assert v.dtype == c.dt and v.is_contiguous(memory_format=CL)
            assert e[k] < TOL[c.dt], (k, e)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", ["linear", "add_relu"])
@pytest.mark.parametrize("shape", CASES, ids=_ids)
def test_against_fp64(monkeypatch, shape, mode, dt):
    _check(monkeypatch, _case(shape, dt, mode), shape)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", CASES[:3], ids=_ids)
def test_relu_without_residual(monkeypatch, shape, dt):
    _check(monkeypatch, _case(shape, dt, "relu"), shape)


@pytest.mark.parametrize("shape", [CASES[2], CASES[4], CASES[6]], ids=_ids)
def test_streaming_equals_resident(monkeypatch, shape):
    c = _case(shape, torch.bfloat16, "add_relu")
    resident = c.run()
    monkeypatch.setenv("MI355X_GN_RESIDENT", "0")
    streaming = c.run()
    assert len(resident) == 5
    for k in resident:
        assert torch.equal(resident[k], streaming[k]), k


def test_bit_reproducible():
    c = _case(CASES[3], torch.bfloat16, "add_relu")
    first, second = c.run(), c.run()
    for k in first:
        assert torch.equal(first[k], second[k]), k


def _t(shape, dt=torch.bfloat16, cl=True):
    t = torch.zeros(shape, device=DEV, dtype=dt)
    return t.contiguous(memory_format=CL) if cl and t.dim() == 4 else t


def _f(*shape):
    return _t(shape, torch.float32)


@pytest.mark.parametrize("call,message", [
    (lambda C: C.gn_fwd(_t((2, 8, 3, 3), torch.float32), _f(8), _f(8), None,
                        2), "x must be a bf16 or fp16 HIP tensor"),
    (lambda C: C.gn_fwd(_t((2, 8, 3, 3), cl=False), _f(8), _f(8), None, 2),
     "x must be 4-D channels_last"),
    (lambda C: C.gn_fwd(_t((2, 12, 3, 3)), _f(12), _f(12), None, 3),
     "C must be a multiple of 8"),
    (lambda C: C.gn_fwd(_t((2, 8, 3, 3)), _f(8), _f(8), None, 8),
     "channels per group must be 2, 4, 8, 16, 32 or 64, got 1"),
    (lambda C: C.gn_fwd(_t((2, 48, 3, 3)), _f(48), _f(48), None, 2),
     "channels per group must be .* got 24"),
    (lambda C: C.gn_fwd(_t((2, 8, 3, 3)), _t((8,)), _f(8), None, 2),
     "gamma must be a contiguous fp32"),
    (lambda C: C.gn_fwd(_t((2, 8, 3, 3)), _f(8), _f(8),
                        _t((2, 8, 3, 3), torch.float16), 2),
     "residual must have the dtype and shape of x"),
    (lambda C: C.gn_bwd(_t((2, 8, 3, 3)), _t((2, 8, 3, 3)), _t((2, 8, 3, 3)),
                        _f(2, 4), _f(2, 2), _f(8), 2),
     r"mean must be \[2, 2\]"),
])
def test_host_refusals(call, message):
    from mi355x_ddp import _C
    with pytest.raises(RuntimeError, match=message):
        call(_C)


@pytest.mark.parametrize("native", [True, False])
def test_resnet50_gn_step(monkeypatch, native):
    from mi355x_ddp.models import build_model
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setenv("MI355X_NATIVE_GN", "1" if native else "0")
    torch.manual_seed(0)
    model = MI355Conv2d.convert(
        build_model("resnet50", 100, norm="gn").to(DEV)).to(
            memory_format=CL).train()
    x = torch.randn(4, 3, 16, 16, device=DEV).contiguous(memory_format=CL)
    labels = torch.randint(0, 100, (4,), device=DEV)
    gn_calls.reset()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x).float(), labels)
    loss.backward()
    assert (gn_calls.fwd, gn_calls.bwd) == ((53, 53) if native else (0, 0))
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
