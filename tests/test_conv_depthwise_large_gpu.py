"""Depthwise 5x5 / 7x7 / 9x9 convolution (csrc/conv_depthwise_large.hip), its
routing through MI355Conv2d and ConvMixer. The kernel tests are exact: x and dy
are integers in [-3, 3], w in [-2, 2], so every partial sum is an integer far
below 2^24 (at most 17 010, a weight grad over 3 x 18 x 35 pixels) and each
pass must `torch.equal` torch's fp32 CPU conv, rounded once to the dtype."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops.conv import MI355Conv2d, depthwise_calls, dwk_calls

pytestmark = pytest.mark.gpu

DEV, CL, BF = "cuda", torch.channels_last, torch.bfloat16
DTYPES = [torch.bfloat16, torch.float16]
KS = [5, 7, 9]

# (N, C, H, W); the tile is 8 x 16
SHAPES = [
    (2, 8, 17, 34),     # 3 x 3 tiles, ragged both ways
    (3, 72, 18, 35),    # ragged second chunk; the largest weight grad
    (1, 136, 9, 17),    # ragged third chunk
    (2, 8, 1, 1), (2, 8, 2, 3),   # extents below the halo
    (1, 8, 1, 40),      # one-pixel rows and columns
    (1, 8, 40, 1),
    (5, 16, 4, 4),
]


class _Case:
    """Integer operands on the GPU, the exact CPU reference rounded once."""

    def __init__(self, shape, K, dt):
        C = shape[1]
        g = torch.Generator().manual_seed(7 * K + sum(shape))
        x = torch.randint(-3, 4, shape, generator=g).float()
        w = torch.randint(-2, 3, (C, 1, K, K), generator=g).float()
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, None, 1, K // 2, 1, C)
        dy = torch.randint(-3, 4, y.shape, generator=g).float()
        dx, dw = torch.autograd.grad(y, (xr, wr), dy)
        self.y, self.dx, self.dw = y.detach().to(dt), dx.to(dt), dw.to(dt)
        self.x = x.to(DEV, dt).contiguous(memory_format=CL)
        self.w = w.to(DEV, dt)
        self.dy = dy.to(DEV, dt).contiguous(memory_format=CL)


@functools.lru_cache(maxsize=None)
def _case(shape, K, dt):
    return _Case(shape, K, dt)


def _C():
    from mi355x_ddp import _C
    return _C


def _counts(c):
    return (c.fwd, c.dgrad, c.wgrad)


def _same(got, ref):
    return got.dtype == ref.dtype and torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_three_passes_exact(shape, K, dt):
    c = _case(shape, K, dt)
    y = _C().conv_dwk_fwd(c.x, c.w)
    dx = _C().conv_dwk_dgrad(c.dy, c.w)
    dw = _C().conv_dwk_wgrad(c.dy, c.x, K, 0)
    assert y.is_contiguous(memory_format=CL) and \
        dx.is_contiguous(memory_format=CL)
    assert _same(y, c.y), "fwd"
    assert _same(dx, c.dx), "dgrad"
    assert _same(dw, c.dw), "wgrad"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("splits", [0, 1, 2, 5, 1000])
def test_wgrad_splits_exact(splits, dt):
    c = _case(SHAPES[1], 7, dt)
    assert _same(_C().conv_dwk_wgrad(c.dy, c.x, 7, splits), c.dw)


@pytest.mark.parametrize("dt", DTYPES)
def test_filter_view_is_read_through_its_strides(dt):
    c = _case(SHAPES[1], 7, dt)
    wide = torch.full((c.w.shape[0], 2, 7, 14), 7.0, device=DEV, dtype=dt)
    view = wide[:, 1:, :, ::2]
    view.copy_(c.w)
    assert _same(_C().conv_dwk_fwd(c.x, view), c.y)
    assert _same(_C().conv_dwk_dgrad(c.dy, view), c.dx)


def _t(shape, dt=BF, cl=True):
    t = torch.zeros(shape, device=DEV, dtype=dt)
    return t.contiguous(memory_format=CL) if cl and t.dim() == 4 else t


_X, _W = (2, 8, 6, 6), (8, 1, 5, 5)
_K, _F = "K must be 5, 7 or 9", r"filter must be \(C, 1, K, K\)"


def _call(name):
    return lambda *args: getattr(_C(), "conv_dwk_" + name)(*args)


fwd, dgrad, wgrad = _call("fwd"), _call("dgrad"), _call("wgrad")


@pytest.mark.parametrize("call,message", [
    (lambda: fwd(_t(_X), _t((8, 1, 3, 3))), _K),
    (lambda: fwd(_t(_X), _t((8, 1, 11, 11))), _K),
    (lambda: wgrad(_t(_X), _t(_X), 3, 0), _K),
    (lambda: fwd(_t(_X), _t((8, 1, 5, 7))), _F),
    (lambda: fwd(_t(_X), _t((16, 1, 5, 5))), _F),     # a channel multiplier
    (lambda: fwd(_t(_X), _t((8, 2, 5, 5))), _F),
    (lambda: fwd(_t(_X, torch.float32), _t(_W)), "x must be a bf16 or fp16"),
    (lambda: dgrad(_t(_X, cl=False), _t(_W)), "dy must be 4-D channels_last"),
    (lambda: fwd(_t(_X), _t(_W, torch.float16)), "must share one dtype"),
    (lambda: wgrad(_t(_X, torch.float16), _t(_X), 5, 0), "share one dtype"),
    (lambda: fwd(_t((2, 12, 6, 6)), _t((12, 1, 5, 5))), "a multiple of 8"),
    (lambda: wgrad(_t(_X), _t(_X), 5, -1), "splits must be in"),
    (lambda: wgrad(_t(_X), _t(_X), 5, 65536), "splits must be in"),
    (lambda: wgrad(_t(_X), _t((2, 8, 6, 7)), 5, 0), "the same extents"),
])
def test_host_refusals(call, message):
    with pytest.raises(RuntimeError, match=message):
        call()


def _module_run(monkeypatch, K, native="1"):
    """One MI355Conv2d step under bf16 autocast on a case's integer data."""
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setenv("MI355X_NATIVE_DEPTHWISE", native)
    c = _case((3, 72, 11, 13), K, BF)
    conv = MI355Conv2d(72, 72, K, padding=K // 2, groups=72, bias=False)
    conv = conv.to(DEV).to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(c.w)
    xd = c.x.float().requires_grad_(True)
    dwk_calls.reset()
    depthwise_calls.reset()
    with torch.autocast("cuda", dtype=BF):
        y = conv(xd)
    y.backward(c.dy)
    return (y.detach(), xd.grad, conv.weight.grad), (c.y, c.dx, c.dw), conv


@pytest.mark.parametrize("K", KS)
def test_module_routes_to_the_large_kernels(monkeypatch, K):
    got, ref, conv = _module_run(monkeypatch, K)
    assert _counts(dwk_calls) == (1, 1, 1)
    assert _counts(depthwise_calls) == (0, 0, 0)
    assert got[0].dtype == BF and got[2].dtype == torch.float32
    assert got[2].stride() == conv.weight.stride()   # FusedSGD's rule
    for name, a, b in zip(("y", "dx", "dw"), got, ref):
        assert torch.equal(a.float().cpu(), b.float()), name


def test_switch_off_and_3x3_leave_the_counters_alone(monkeypatch):
    got, _, _ = _module_run(monkeypatch, 7, native="0")
    assert _counts(dwk_calls) == (0, 0, 0)
    assert torch.isfinite(got[0]).all() and got[2] is not None
    _module_run(monkeypatch, 3)
    assert _counts(dwk_calls) == (0, 0, 0)
    assert _counts(depthwise_calls) == (1, 1, 1)


def _rel_err(got, ref):
    return ((got.float().cpu() - ref).norm() / ref.norm()).item()


def test_convmixer_step(monkeypatch):
    """Logits and every parameter grad are at most 2x as far from the fp32
    CPU model as with the depthwise convs on torch's conv: two bf16 pipelines
    that differ in the order of an at most 49-term fp32 sum."""
    from mi355x_ddp.models import ConvMixer
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    torch.manual_seed(0)
    cpu_model = ConvMixer(64, 2, 7, 2, 10).train()
    x = torch.randn(4, 3, 32, 32)
    labels = torch.randint(0, 10, (4,))
    model = MI355Conv2d.convert(copy.deepcopy(cpu_model).to(DEV))
    model = model.to(memory_format=CL).train()
    logits = cpu_model(x)
    F.cross_entropy(logits, labels).backward()
    ref = [logits.detach()] + [p.grad for p in cpu_model.parameters()]
    xd, ld = x.to(DEV).contiguous(memory_format=CL), labels.to(DEV)
    runs = []
    for native in ("1", "0"):
        monkeypatch.setenv("MI355X_NATIVE_DEPTHWISE", native)
        model.zero_grad(set_to_none=True)
        dwk_calls.reset()
        with torch.autocast("cuda", dtype=BF):
            out = model(xd)
            F.cross_entropy(out.float(), ld).backward()
        runs.append([out.detach()] + [p.grad for p in model.parameters()])
        assert _counts(dwk_calls) == ((2, 2, 2) if native == "1" else (0,) * 3)
    got, base = runs
    names = ["logits"] + [k for k, _ in model.named_parameters()]
    errs = [(_rel_err(a, r), _rel_err(b, r))
            for a, b, r in zip(got, base, ref)]
    for name, (e, eb) in zip(names, errs):
        print(f"convmixer {name}: rel err native {e:.3e}, torch {eb:.3e}")
    assert all(e <= 2 * eb for e, eb in errs), list(zip(names, errs))
