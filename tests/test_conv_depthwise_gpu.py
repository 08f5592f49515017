"""Depthwise 3x3 convolution on the kernels of csrc/conv_depthwise.hip, its
routing through MI355Conv2d and the MobileNet-v1 model.

The kernel tests are exact. x and dy are integers in [-3, 3] and w integers in
[-2, 2], so every partial sum is an integer far below 2^24 (the largest, a
weight grad over 3 x 18 x 35 pixels, stays below 2e4) and each pass must equal
torch's fp32 conv ON THE CPU with groups = C, rounded once to the 16-bit
format, under `torch.equal`.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops.conv import MI355Conv2d, depthwise_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}   # test_conv_grouped_gpu.py
DTYPES = [torch.bfloat16, torch.float16]

# (N, C, H, W, stride)
SHAPES = [
    (2, 8, 17, 34, 1),     # one lane group; 3 x 3 wide tiles, ragged both ways
    (3, 72, 18, 35, 1),    # ragged second chunk; the largest weight grad
    (2, 72, 18, 35, 2),    # stride 2: 9 x 18 outputs, gather dgrad on 18 x 35
    (1, 136, 17, 34, 2),   # ragged third chunk, odd H at stride 2
    (2, 8, 9, 17, 2),      # odd extents at stride 2
    (2, 8, 1, 1, 1), (2, 8, 1, 1, 2), (2, 8, 2, 2, 1), (2, 8, 2, 2, 2),
    (1, 8, 1, 40, 1), (1, 8, 1, 40, 2), (1, 8, 40, 1, 1), (1, 8, 40, 1, 2),
    (5, 16, 4, 4, 1),      # 8 images per block, N = 5
    (5, 16, 2, 2, 1),
    (5, 16, 4, 4, 2),
    (5, 16, 7, 7, 2),      # 4 images per block forward, 2 per block dgrad
    (3, 72, 7, 8, 1),      # 2 images per block, N = 3
]
SPLIT_SHAPES = [SHAPES[1], SHAPES[16]]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


class _Case:
    """Integer operands on the GPU and the exact CPU reference of the three
    passes, rounded once. Built once per (shape, dtype), never written to."""

    def __init__(self, shape, dt):
        N, C, H, W, stride = shape
        g = torch.Generator().manual_seed(99 + sum(shape))
        x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
        w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).float()
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, None, stride, 1, 1, C)
        dy = torch.randint(-3, 4, y.shape, generator=g).float()
        dx, dw = torch.autograd.grad(y, (xr, wr), dy)
        self.y, self.dx, self.dw = y.detach().to(dt), dx.to(dt), dw.to(dt)
        self.x = x.to(DEV, dt).contiguous(memory_format=CL)
        self.w = w.to(DEV, dt)
        self.dy = dy.to(DEV, dt).contiguous(memory_format=CL)
        self.H, self.W, self.stride = H, W, stride


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    return _Case(shape, dt)


def _C():
    from mi355x_ddp import _C
    return _C


def _same(got, ref):
    return got.dtype == ref.dtype and torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_three_passes_exact(shape, dt):
    c = _case(shape, dt)
    y = _C().conv_dw_fwd(c.x, c.w, c.stride)
    dx = _C().conv_dw_dgrad(c.dy, c.w, c.H, c.W, c.stride)
    dw = _C().conv_dw_wgrad(c.dy, c.x, c.stride, 0)
    assert y.is_contiguous(memory_format=CL)
    assert dx.is_contiguous(memory_format=CL)
    assert _same(y, c.y), "fwd"
    assert _same(dx, c.dx), "dgrad"
    assert _same(dw, c.dw), "wgrad"


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("splits", [0, 1, 2, 5, 1000])
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=_ids)
def test_wgrad_splits_exact(shape, splits, dt):
    c = _case(shape, dt)
    assert _same(_C().conv_dw_wgrad(c.dy, c.x, c.stride, splits), c.dw)


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_filter_view_is_read_through_its_strides(dt):
    c = _case(SHAPES[2], dt)
    wide = torch.full((c.w.shape[0], 2, 3, 6), 7.0, device=DEV, dtype=dt)
    view = wide[:, 1:, :, ::2]
    view.copy_(c.w)
    assert not view.is_contiguous()
    assert _same(_C().conv_dw_fwd(c.x, view, c.stride), c.y)
    assert _same(_C().conv_dw_dgrad(c.dy, view, c.H, c.W, c.stride), c.dx)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[16]], ids=_ids)
def test_stride2_dgrad_writes_all_of_dx(shape):
    """dx comes from torch.empty: poison the allocator's free blocks first."""
    c = _case(shape, torch.bfloat16)
    for _ in range(2):
        poison = torch.ones(c.dx.numel(), device=DEV, dtype=torch.bfloat16)
        del poison
        assert _same(_C().conv_dw_dgrad(c.dy, c.w, c.H, c.W, 2), c.dx)


def _t(shape, dt=torch.bfloat16, cl=True):
    t = torch.zeros(shape, device=DEV, dtype=dt)
    return t.contiguous(memory_format=CL) if cl and t.dim() == 4 else t


@pytest.mark.parametrize("call,message", [
    (lambda C: C.conv_dw_fwd(_t((2, 8, 6, 6), torch.float32), _t((8, 1, 3, 3)),
                             1), "x must be a bf16 or fp16 HIP tensor"),
    (lambda C: C.conv_dw_fwd(_t((2, 8, 6, 6)),
                             _t((8, 1, 3, 3), torch.float16), 1),
     "must share one dtype"),
    (lambda C: C.conv_dw_wgrad(_t((2, 8, 6, 6), torch.float16),
                               _t((2, 8, 6, 6)), 1, 0),
     "must share one dtype"),
    (lambda C: C.conv_dw_fwd(_t((2, 8, 6, 6), cl=False), _t((8, 1, 3, 3)), 1),
     "x must be 4-D channels_last"),
    (lambda C: C.conv_dw_dgrad(_t((2, 8, 6, 6), cl=False), _t((8, 1, 3, 3)),
                               6, 6, 1), "dy must be 4-D channels_last"),
    (lambda C: C.conv_dw_fwd(_t((2, 8, 6, 6)), _t((8, 1, 5, 5)), 1),
     r"filter must be \(C, 1, 3, 3\)"),
    (lambda C: C.conv_dw_fwd(_t((2, 8, 6, 6)), _t((8, 2, 3, 3)), 1),
     r"filter must be \(C, 1, 3, 3\)"),
    (lambda C: C.conv_dw_dgrad(_t((2, 8, 6, 6)), _t((16, 1, 3, 3)), 6, 6, 1),
     r"filter must be \(C, 1, 3, 3\)"),
    (lambda C: C.conv_dw_fwd(_t((2, 12, 6, 6)), _t((12, 1, 3, 3)), 1),
     "C must be a multiple of 8"),
    (lambda C: C.conv_dw_fwd(_t((2, 8, 6, 6)), _t((8, 1, 3, 3)), 3),
     "stride must be 1 or 2"),
    (lambda C: C.conv_dw_wgrad(_t((2, 8, 6, 6)), _t((2, 8, 6, 6)), 0, 0),
     "stride must be 1 or 2"),
    (lambda C: C.conv_dw_dgrad(_t((2, 8, 6, 6)), _t((8, 1, 3, 3)), 6, 6, 2),
     "dy's extents do not belong"),
    (lambda C: C.conv_dw_dgrad(_t((2, 8, 3, 3)), _t((8, 1, 3, 3)), 6, 7, 2),
     "dy's extents do not belong"),
    (lambda C: C.conv_dw_wgrad(_t((2, 8, 6, 6)), _t((2, 8, 6, 6)), 2, 0),
     "dy's extents do not belong"),
])
def test_host_refusals(call, message):
    with pytest.raises(RuntimeError, match=message):
        call(_C())


def _rel_err(got, ref):
    got = got.float().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _module_run(monkeypatch, dt, stride, native):
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setenv("MI355X_NATIVE_DEPTHWISE", "1" if native else "0")
    torch.manual_seed(5)
    ref = torch.nn.Conv2d(72, 72, 3, stride, 1, groups=72, bias=False)
    conv = MI355Conv2d(72, 72, 3, stride, 1, groups=72, bias=False)
    conv.load_state_dict(ref.state_dict())
    conv = conv.to(DEV).to(memory_format=CL)
    x = torch.randn(3, 72, 11, 13)
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    depthwise_calls.reset()
    with torch.autocast("cuda", dtype=dt):
        y = conv(xd)
    dy = torch.randn(y.shape)
    y.backward(dy.to(DEV, dt).contiguous(memory_format=CL))
    return ref, conv, x, dy, xd, y


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_module_under_autocast(monkeypatch, dt, stride):
    ref, conv, x, dy, xd, y = _module_run(monkeypatch, dt, stride, True)
    assert (depthwise_calls.fwd, depthwise_calls.dgrad,
            depthwise_calls.wgrad) == (1, 1, 1)
    assert y.dtype == dt
    assert conv.weight.grad.dtype == torch.float32
    assert conv.weight.grad.shape == conv.weight.shape
    assert conv.weight.grad.stride() == conv.weight.stride()   # FusedSGD's rule
    # the fp32 CPU module on the same rounded operands
    with torch.no_grad():
        ref.weight.copy_(ref.weight.to(dt).float())
    xr = x.to(dt).float().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.to(dt).float())
    errs = (_rel_err(y, yr.detach()), _rel_err(xd.grad, xr.grad),
            _rel_err(conv.weight.grad, ref.weight.grad))
    print(f"module {dt} stride {stride}: y/dx/dw rel err",
          ["%.3e" % e for e in errs])
    assert max(errs) < TOL[dt], errs


def test_switch_off_leaves_counters_at_zero(monkeypatch):
    _, conv, _, _, xd, y = _module_run(monkeypatch, torch.bfloat16, 1, False)
    assert (depthwise_calls.fwd, depthwise_calls.dgrad,
            depthwise_calls.wgrad) == (0, 0, 0)
    assert torch.isfinite(y).all() and conv.weight.grad is not None


def _mobilenet_logits(monkeypatch, native, model, x, labels):
    monkeypatch.setenv("MI355X_NATIVE_DEPTHWISE", "1" if native else "0")
    model.zero_grad(set_to_none=True)
    depthwise_calls.reset()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(x)
        loss = F.cross_entropy(logits.float(), labels)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is not None for p in model.parameters())
    return logits.detach().float().cpu(), depthwise_calls.fwd


def test_mobilenet_v1_step(monkeypatch):
    """A routing check, not a precision check: all 13 depthwise layers run
    native, and the logits are at most 2x as far from the fp32 CPU model as
    those of the same model with depthwise convs on torch's conv (two 16-bit
    pipelines of equal depth that differ in accumulation order)."""
    import copy
    from mi355x_ddp.models import mobilenet_v1
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    torch.manual_seed(0)
    cpu_model = mobilenet_v1().train()
    x = torch.randn(4, 3, 16, 16)
    labels = torch.randint(0, 100, (4,))
    model = MI355Conv2d.convert(copy.deepcopy(cpu_model).to(DEV))
    model = model.to(memory_format=CL).train()
    with torch.no_grad():
        ref = cpu_model(x)
    xd = x.to(DEV).contiguous(memory_format=CL)
    ld = labels.to(DEV)
    got, nfwd = _mobilenet_logits(monkeypatch, True, model, xd, ld)
    base, nbase = _mobilenet_logits(monkeypatch, False, model, xd, ld)
    err, err_base = _rel_err(got, ref), _rel_err(base, ref)
    print(f"mobilenet_v1 logits rel err: native depthwise {err:.3e}, "
          f"torch depthwise {err_base:.3e}")
    assert (nfwd, nbase) == (13, 0)
    assert err <= 2 * err_base, (err, err_base)
