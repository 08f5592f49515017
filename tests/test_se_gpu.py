"""Squeeze-and-Excitation on the kernels of csrc/se_block.hip: `se_add_relu`
against an fp64 CPU reference, bit-reproducibility, host refusals and the
routing of the SE models. profiles/se_block.md has the measured errors of
every case.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops import SqueezeExcite, se_add_relu
from mi355x_ddp.ops.conv import MI355Conv2d
from mi355x_ddp.ops.se import se_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}   # test_conv_grouped_gpu.py
DTYPES = [torch.bfloat16, torch.float16]
NAMES = ["out", "du", "d_identity", "dW1", "db1", "dW2", "db2"]

# (N, C, Cr, H, W)
CASES = [
    (3, 64, 4, 1, 1),      # one pixel, Cr < 16, ragged image tile
    (17, 72, 24, 7, 7),    # second image tile of one row, ragged chunk and Cr
    (2, 128, 16, 8, 9),    # more pixels than slots
    (16, 256, 16, 2, 2),   # several images per squeeze block, exact tiles
    (33, 64, 8, 4, 4),     # wgrad over the batch with a ragged last K step
]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else None


def _formula(u, idn, w1, b1, w2, b2):
    s = u.mean(dim=(2, 3))
    g = torch.sigmoid(torch.relu(s @ w1.t() + b1) @ w2.t() + b2)
    return u * g[:, :, None, None] + idn


class _Case:
    """16-bit-rounded u, identity, dout and fp32 parameters, and the fp64 CPU
    results of the plain formula on them. Built once, never written to."""

    def __init__(self, shape, dt):
        N, C, Cr, H, W = shape
        gen = torch.Generator().manual_seed(7 + sum(shape))
        rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        self.se = SqueezeExcite(C, C // Cr)
        assert self.se.fc1.weight.shape == (Cr, C)
        with torch.no_grad():
            for p in self.se.parameters():
                p.copy_(rnd(*p.shape) * (0.5 if p.dim() == 1 else
                                         p.shape[1] ** -0.5))
        params = [p.detach().double().requires_grad_(True)
                  for p in self.se.parameters()]
        u = rnd(N, C, H, W).to(dt).double()
        idn = rnd(N, C, H, W)
        # keep every pre-activation away from the ReLU's kink: the mask is
        # then never in question and no element is left out of a comparison
        pre = _formula(u, idn, *params).detach()
        idn += torch.where(pre.abs() < 0.05,
                           torch.where(pre < 0, -0.25, 0.25), 0.0)
        idn = idn.to(dt).double()
        dout = rnd(N, C, H, W).to(dt).double()
        u.requires_grad_(True)
        idn.requires_grad_(True)
        pre = _formula(u, idn, *params)
        assert pre.abs().min() > 0.03
        out = torch.relu(pre)
        grads = torch.autograd.grad(out, [u, idn] + params, dout)
        self.ref = [out.detach()] + list(grads)
        self.dt = dt
        self.u, self.idn, self.dout = (
            t.detach().to(DEV, dt).contiguous(memory_format=CL)
            for t in (u, idn, dout))
        self.longest = max(N, C, H * W)

    def run(self):
        """The seven results of the public op on the GPU operands."""
        se = copy.deepcopy(self.se).to(DEV)
        u = self.u.clone().requires_grad_(True)
        idn = self.idn.clone().requires_grad_(True)
        out = se_add_relu(u, idn, se)
        out.backward(self.dout)
        return [out.detach(), u.grad, idn.grad] + \
            [p.grad for p in se.parameters()]


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    return _Case(shape, dt)


def _rel_err(got, ref):
    got = got.detach().double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", CASES, ids=_ids)
def test_against_fp64(monkeypatch, shape, dt):
    c = _case(shape, dt)
    se_calls.reset()
    got = c.run()
    assert (se_calls.fwd, se_calls.bwd) == (1, 1)
    monkeypatch.setenv("MI355X_NATIVE_SE", "0")
    torch_def = c.run()
    assert (se_calls.fwd, se_calls.bwd) == (1, 1)
    e = [_rel_err(g, r) for g, r in zip(got, c.ref)]
    e_torch = [_rel_err(g, r) for g, r in zip(torch_def, c.ref)]
    print("se", _ids(shape), _ids(dt), "native",
          " ".join(f"{n} {v:.2e}" for n, v in zip(NAMES, e)), "| torch",
          " ".join(f"{n} {v:.2e}" for n, v in zip(NAMES, e_torch)))
    for g in got[:3]:
        assert g.dtype == dt and g.is_contiguous(memory_format=CL)
    for g in got[3:]:
        assert g.dtype == torch.float32
    assert max(e[:3]) < TOL[dt], e
    floor = c.longest ** 0.5 * 2.0 ** -24
    for name, en, et in zip(NAMES[3:], e[3:], e_torch[3:]):
        assert en <= max(4 * et, floor), (name, en, et, floor)


def test_bit_reproducible():
    c = _case(CASES[4], torch.bfloat16)
    first, second = c.run(), c.run()
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), name


def _t(shape, dt=torch.bfloat16, cl=True):
    t = torch.zeros(shape, device=DEV, dtype=dt)
    return t.contiguous(memory_format=CL) if cl and t.dim() == 4 else t


def _f(*shape):
    return _t(shape, torch.float32)


@pytest.mark.parametrize("call,message", [
    (lambda C: C.se_squeeze(_t((2, 8, 3, 3), torch.float32)),
     "u must be a bf16 or fp16 HIP tensor"),
    (lambda C: C.se_squeeze(_t((2, 8, 3, 3), cl=False)),
     "u must be 4-D channels_last"),
    (lambda C: C.se_squeeze(_t((2, 12, 3, 3))), "C must be a multiple of 8"),
    (lambda C: C.se_excite_fwd(_f(2, 16), _t((4, 16)), _f(4), _f(16, 4),
                               _f(16)),
     "fc1.weight must be a contiguous fp32"),
    (lambda C: C.se_excite_fwd(_f(2, 16), _f(4, 16), _f(4), _f(4, 16).t(),
                               _f(16)),
     "fc2.weight must be a contiguous fp32"),
    (lambda C: C.se_excite_fwd(_f(2, 16), _f(4, 16), _f(5), _f(16, 4),
                               _f(16)), r"fc1.bias must be \[4\]"),
    (lambda C: C.se_excite_fwd(_f(2, 8192), _f(520, 8192), _f(520),
                               _f(8192, 520), _f(8192)),
     r"reduced width must be in 1\.\.512"),
    (lambda C: C.se_scale_add_relu(_t((2, 8, 3, 3)),
                                   _t((2, 8, 3, 3), torch.float16), _f(2, 8)),
     "identity must have the dtype and shape of u"),
    (lambda C: C.se_join_bwd_reduce(_t((2, 8, 3, 3)), _t((2, 8, 3, 4)),
                                    _t((2, 8, 3, 3))),
     "out must have the dtype and shape of u"),
    (lambda C: C.se_excite_bwd(_f(2, 16), _f(2, 16), _f(2, 5), _f(4, 16),
                               _f(16, 4)), r"h must be \[2, 4\]"),
    (lambda C: C.se_excite_wgrad(_f(2, 16), _f(2, 4), _f(2, 4), _f(3, 16)),
     r"s must be \[2, 16\]"),
    (lambda C: C.se_join_bwd_apply(_t((2, 8, 3, 3)), _t((2, 8, 3, 3)),
                                   _f(2, 8), _f(2, 16)),
     r"ds must be \[2, 8\]"),
])
def test_host_refusals(call, message):
    from mi355x_ddp import _C
    with pytest.raises(RuntimeError, match=message):
        call(_C)


def _gpu(model):
    return MI355Conv2d.convert(copy.deepcopy(model).to(DEV)).to(
        memory_format=CL)


@pytest.mark.parametrize("native", [True, False])
def test_se_resnet50_step(monkeypatch, native):
    from mi355x_ddp.models import se_resnet50
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setenv("MI355X_NATIVE_SE", "1" if native else "0")
    torch.manual_seed(0)
    model = _gpu(se_resnet50()).train()
    x = torch.randn(4, 3, 16, 16, device=DEV).contiguous(memory_format=CL)
    labels = torch.randint(0, 100, (4,), device=DEV)
    se_calls.reset()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x).float(), labels)
    loss.backward()
    assert (se_calls.fwd, se_calls.bwd) == ((16, 16) if native else (0, 0))
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


def test_se_resnet18_fused_eval(monkeypatch):
    """The fused evaluation forward needs no SE code of its own: the last conv
    of a block folds without ReLU or residual and the three forward kernels
    follow. Its logits are at most 2x as far from the fp32 CPU model as those
    of the unfused evaluation forward (the rule of test_mobilenet_v1_step)."""
    from mi355x_ddp.core.inference import fused_inference
    from mi355x_ddp.models import se_resnet18
    from mi355x_ddp.ops import fused_eval
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    torch.manual_seed(0)
    cpu_model = se_resnet18().eval()
    x = torch.randn(4, 3, 32, 32)
    model = _gpu(cpu_model).eval()
    xd = x.to(DEV).contiguous(memory_format=CL)
    with torch.no_grad():
        ref = cpu_model(x).double()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            unfused = model(xd)
            se_calls.reset()
            fused_eval.calls.reset()
            with fused_inference(model):
                fused = model(xd)
    assert se_calls.fwd == 8
    assert fused_eval.calls.fused == 20 and fused_eval.calls.fallback == 0
    e_f, e_u = _rel_err(fused, ref), _rel_err(unfused, ref)
    print(f"se_resnet18 eval logits rel err: fused {e_f:.3e}, "
          f"unfused {e_u:.3e}")
    assert e_f <= 2 * e_u, (e_f, e_u)
