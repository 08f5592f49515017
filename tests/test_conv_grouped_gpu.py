"""Grouped 3x3 convolution on the packed MFMA kernels (csrc/conv_grouped.hip)
and its routing through MI355Conv2d and the ResNeXt models.

Reference and tolerances are those of tests/test_conv_fp16_gpu.py: torch's
fp32 conv ON THE CPU with `groups`, fed the same 16-bit-rounded operands;
relative Frobenius error; 5e-4 for fp16 and 4e-3 for bf16, about 2.4x the
reference's own rounding to the output format (2.04-2.12e-4 and 1.60-1.70e-3
on all three passes of these shapes). Weights are randn / sqrt(9 * Cg).

A norm over the whole tensor cannot see a few wrong elements. The elementwise
check is tests/test_conv_grouped_exact_gpu.py: integer operands, `torch.equal`
against the same CPU reference, on shapes that reach every kernel variant on
more than one tile.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import MI355Conv2d, grouped_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}
DTYPES = [torch.bfloat16, torch.float16]

# (N, C, H, W, groups, stride)
SHAPES = [
    (2, 32, 8, 8, 8, 1),      # Cg 4, eight groups in the single pack, one tile
    (3, 64, 10, 10, 8, 2),    # Cg 8, two packs, stride 2, ragged 5x5 output
    (2, 64, 9, 7, 4, 1),      # Cg 16, H != W and both odd: edge masks
    (2, 64, 8, 8, 2, 2),      # Cg 32, block = whole pack, stride 2, even
    (1, 128, 6, 6, 2, 1),     # Cg 64, P = 64: two K steps, four fragments
    (2, 32, 7, 9, 8, 2),      # stride 2 on odd extents: zero-inserted dgrad
    (2, 32, 20, 36, 8, 1),    # 3 x 3 tiles, interior halos; wgrad splits
]
TILED = SHAPES[-1]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


class _Case:
    """Rounded operands on the GPU and the fp32 CPU reference of all three
    passes. Built once per (shape, dtype) and never written to."""

    def __init__(self, shape, dt):
        N, C, H, W, groups, stride = shape
        Cg = C // groups
        g = torch.Generator().manual_seed(4321 + sum(shape))
        x = torch.randn(N, C, H, W, generator=g).to(dt)
        w = (torch.randn(C, Cg, 3, 3, generator=g) / (9 * Cg) ** 0.5).to(dt)
        xr = x.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        y = F.conv2d(xr, wr, None, stride, 1, 1, groups)
        dy = torch.randn(y.shape, generator=g).to(dt)
        dx, dw = torch.autograd.grad(y, (xr, wr), dy.float())
        self.y, self.dx, self.dw = y.detach(), dx, dw
        self.x = x.to(DEV).contiguous(memory_format=CL)
        self.w = w.to(DEV).contiguous(memory_format=CL)
        self.dy = dy.to(DEV).contiguous(memory_format=CL)
        self.H, self.W, self.groups, self.stride = H, W, groups, stride


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    return _Case(shape, dt)


def _rel_err(got, ref):
    got = got.float().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _C():
    from mi355x_ddp import _C
    return _C


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_three_passes_parity(shape, dt):
    c = _case(shape, dt)
    wp, wpT = _C().conv_grouped_prep(c.w, c.groups)
    y = _C().conv_grouped_fwd(c.x, wp, c.stride)
    dx = _C().conv_grouped_dgrad(c.dy, wpT, c.H, c.W, c.stride)
    dw = _C().conv_grouped_wgrad(c.dy, c.x, c.groups, c.stride, 0)
    for name, got, ref in (("y", y, c.y), ("dx", dx, c.dx), ("dw", dw, c.dw)):
        err = _rel_err(got, ref)
        print(f"{name} {shape} {dt}: rel err {err:.3e}")
        assert got.dtype == dt and got.shape == ref.shape, name
        assert got.is_contiguous(memory_format=CL), name
        assert err < TOL[dt], (name, err)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("splits", [1, 3, 0])
def test_wgrad_splits(splits, dt):
    c = _case(TILED, dt)
    got = _C().conv_grouped_wgrad(c.dy, c.x, c.groups, c.stride, splits)
    err = _rel_err(got, c.dw)
    print(f"wgrad splits={splits} {dt}: rel err {err:.3e}")
    assert err < TOL[dt], err
    again = _C().conv_grouped_wgrad(c.dy, c.x, c.groups, c.stride, splits)
    assert torch.equal(got, again)


def _module_run(monkeypatch, native):
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setenv("MI355X_NATIVE_GROUPED", "1" if native else "0")
    torch.manual_seed(3)
    ref = torch.nn.Conv2d(64, 64, 3, padding=1, groups=8, bias=False)
    conv = MI355Conv2d(64, 64, 3, padding=1, groups=8, bias=False)
    conv.load_state_dict(ref.state_dict())
    conv = conv.to(DEV).to(memory_format=CL)
    x = torch.randn(2, 64, 12, 12)
    dy = torch.randn(2, 64, 12, 12)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    grouped_calls.reset()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv(xd)
    # the forward's input-grad operand, kept on ctx; backward must use it as
    # it is and not pack the weight again
    kept = getattr(y.grad_fn, "wpT", None)
    y.backward(dy.to(DEV).bfloat16().contiguous(memory_format=CL))
    assert getattr(y.grad_fn, "wpT", None) is kept
    assert (kept is not None) == native
    return ref, conv, x, dy, xd, y


def test_module_under_bf16_autocast(monkeypatch):
    ref, conv, x, dy, xd, y = _module_run(monkeypatch, native=True)
    assert (grouped_calls.fwd, grouped_calls.dgrad, grouped_calls.wgrad) == \
        (1, 1, 1)
    assert y.dtype == torch.bfloat16
    assert conv.weight.grad.dtype == torch.float32
    assert conv.weight.grad.shape == conv.weight.shape
    assert convmod.shadow_of(conv.weight) is None
    # the fp32 CPU module on the same rounded operands
    bf = torch.bfloat16
    with torch.no_grad():
        ref.weight.copy_(ref.weight.to(bf).float())
    xr = x.to(bf).float().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.to(bf).float())
    errs = (_rel_err(y, yr.detach()), _rel_err(xd.grad, xr.grad),
            _rel_err(conv.weight.grad, ref.weight.grad))
    print("module bf16: y/dx/dw rel err", ["%.3e" % e for e in errs])
    assert max(errs) < TOL[bf], errs


def test_switch_off_leaves_counters_at_zero(monkeypatch):
    _, conv, _, _, xd, y = _module_run(monkeypatch, native=False)
    assert (grouped_calls.fwd, grouped_calls.dgrad, grouped_calls.wgrad) == \
        (0, 0, 0)
    assert torch.isfinite(y).all() and conv.weight.grad is not None


def _resnext_logits(monkeypatch, native, model, x, labels):
    monkeypatch.setenv("MI355X_NATIVE_GROUPED", "1" if native else "0")
    model.zero_grad(set_to_none=True)
    grouped_calls.reset()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(x)
        loss = F.cross_entropy(logits.float(), labels)
    loss.backward()
    assert torch.isfinite(loss)
    return logits.detach().float().cpu(), grouped_calls.fwd


def test_resnext50_step(monkeypatch):
    """Logits against the same model in fp32 on the CPU: the native grouped
    run may be at most 2x as far off as the run with grouped convs on torch's
    conv; both are 16-bit pipelines of equal depth that differ only in
    accumulation order."""
    import copy
    from mi355x_ddp.models import resnext50_32x4d
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    torch.manual_seed(0)
    cpu_model = resnext50_32x4d().train()
    x = torch.randn(4, 3, 16, 16)
    labels = torch.randint(0, 100, (4,))
    model = MI355Conv2d.convert(copy.deepcopy(cpu_model).to(DEV))
    model = model.to(memory_format=CL).train()
    with torch.no_grad():
        ref = cpu_model(x)
    xd = x.to(DEV).contiguous(memory_format=CL)
    ld = labels.to(DEV)
    got, nfwd = _resnext_logits(monkeypatch, True, model, xd, ld)
    base, nbase = _resnext_logits(monkeypatch, False, model, xd, ld)
    err, err_base = _rel_err(got, ref), _rel_err(base, ref)
    print(f"resnext50_32x4d logits rel err: native grouped {err:.3e}, "
          f"torch grouped {err_base:.3e}")
    assert (nfwd, nbase) == (16, 0)
    assert err <= 2 * err_base, (err, err_base)
