"""fp16 implicit-GEMM convolutions on the GPU (MI355X): the f16 MFMA
instantiations of the conv kernels, fp16 weight shadows and their refresh in
the SGD step, and the routing of fp16 autocast onto the native kernels.

Reference and tolerances. Every parity check compares against torch's fp32
conv ON THE CPU, fed the same 16-bit-rounded operands (`x.to(dt).float()`):
the input quantisation cancels and what is left is the rounding of the output
to the 16-bit format plus the accumulation order. The reference's own
rounding to the output format is a relative Frobenius error of 2.1e-4 for
fp16 and 1.66e-3 for bf16 on all three passes of these shapes; the bounds are
5e-4 for fp16 and 4e-3 for bf16, about 2.4x the floor each. The fp16 bound
sits 3x under the bf16 floor: an fp16 kernel that rounds through bf16 anywhere
fails. The bf16 rows are the control that tells a format bug from a shape bug.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.core.amp import DynamicLossScaler
from mi355x_ddp.ops.conv import (MI355Conv2d, WeightShadow, rotate_wT,
                                 shadow_of)
from mi355x_ddp.ops.sgd import FusedSGD
from mi355x_ddp.ops.xent import softmax_cross_entropy

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}
DTYPES = [torch.bfloat16, torch.float16]

# (N, C, H, W, K, R, stride, pad): the smallest shapes that reach every path
SHAPES = [
    (2, 64, 8, 8, 64, 3, 1, 1),      # FAST, M = 128 exactly
    (3, 64, 10, 10, 128, 3, 2, 1),   # stride-2 parity dgrad, ragged M = 75
    (2, 64, 8, 8, 128, 1, 2, 0),     # 1x1 s2: memset plus one parity class
    (2, 3, 10, 10, 64, 3, 1, 1),     # PADC stem, ragged
    (2, 3, 16, 16, 64, 7, 2, 3),     # 7x7 stem, K 196 -> 256
    (2, 128, 8, 8, 256, 1, 1, 0),    # BNT=128 and 256x64 wgrad targets
    (2, 256, 4, 4, 512, 3, 1, 1),    # reduction length 2304 on a tiny image
]
S64 = SHAPES[0]
S1X1 = SHAPES[5]
STEM = SHAPES[3]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


class _Case:
    """Rounded operands on the GPU and the fp32 CPU reference of all three
    passes. Built once per (shape, dtype, dy scale) and never written to."""

    def __init__(self, shape, dt, dy_scale):
        N, C, H, W, K, R, stride, pad = shape
        P = (H + 2 * pad - R) // stride + 1
        Q = (W + 2 * pad - R) // stride + 1
        g = torch.Generator().manual_seed(1234 + sum(shape))
        x = torch.randn(N, C, H, W, generator=g).to(dt)
        w = (torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5).to(dt)
        dy = (torch.randn(N, K, P, Q, generator=g) * dy_scale).to(dt)
        xr = x.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        y = F.conv2d(xr, wr, None, stride, pad)
        dx, dw = torch.autograd.grad(y, (xr, wr), dy.float())
        self.y, self.dx, self.dw = y.detach(), dx, dw
        self.x = x.to(DEV).contiguous(memory_format=CL)
        self.w = w.to(DEV).contiguous(memory_format=CL)
        self.dy = dy.to(DEV).contiguous(memory_format=CL)
        self.wT = rotate_wT(self.w)
        self.R, self.stride, self.pad, self.H, self.W = R, stride, pad, H, W


@functools.lru_cache(maxsize=None)
def _case(shape, dt, dy_scale=1.0):
    return _Case(shape, dt, dy_scale)


def _rel_err(got, ref):
    got = got.float().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _C():
    from mi355x_ddp import _C
    return _C


def _fwd(c, tile=0):
    return _C().conv_fwd_igemm(c.x, c.w, c.stride, c.pad, tile)


def _dgrad(c, tile=0):
    return _C().conv_dgrad_igemm(c.dy, c.wT, c.H, c.W, c.stride, c.pad, tile)


def _wgrad(c, splits=0, wtile=0, out_fp32=False):
    return _C().conv_wgrad_igemm(c.dy, c.x, c.R, c.R, c.stride, c.pad,
                                 splits, wtile, out_fp32)


# --------------------------------------------------------------------------
# parity
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fwd_parity(shape, dt):
    c = _case(shape, dt)
    got = _fwd(c)
    err = _rel_err(got, c.y)
    print(f"fwd {shape} {dt}: rel err {err:.3e}")
    assert got.dtype == dt and got.shape == c.y.shape
    assert got.is_contiguous(memory_format=CL)
    assert err < TOL[dt], err


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dgrad_parity(shape, dt):
    c = _case(shape, dt)
    got = _dgrad(c)
    err = _rel_err(got, c.dx)
    print(f"dgrad {shape} {dt}: rel err {err:.3e}")
    assert got.dtype == dt and got.shape == c.dx.shape
    assert got.is_contiguous(memory_format=CL)
    assert err < TOL[dt], err


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_wgrad_parity(shape, dt):
    c = _case(shape, dt)
    got = _wgrad(c)
    err = _rel_err(got, c.dw)
    print(f"wgrad {shape} {dt}: rel err {err:.3e}")
    N, C, H, W, K, R, _, _ = shape
    assert got.dtype == dt and got.shape == (K, C, R, R)
    assert got.is_contiguous(memory_format=CL)
    assert err < TOL[dt], err


# --------------------------------------------------------------------------
# launch variants agree (fp16)
# --------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fwd_dgrad_tiles_bit_equal(shape):
    """Every output element is one chain of MFMAs over the reduction chunks
    in increasing order, whatever the tile shape, so all tiles give the same
    bits: 128 vs 228 on the FAST wide-N shapes and 64 vs 128 on the stem are
    what the bf16 suite asserts; the other pairs follow from the same
    argument."""
    c = _case(shape, torch.float16)
    y0, dx0 = _fwd(c), _dgrad(c)
    for tile in (64, 128, 228):
        assert torch.equal(_fwd(c, tile), y0), ("fwd", tile)
        assert torch.equal(_dgrad(c, tile), dx0), ("dgrad", tile)


WGRAD_VARIANTS = [(t, 0) for t in (1, 2, 3, 4, 5, 6, 8, 9)] + \
                 [(0, s) for s in (-1, 1, 2, 32)]


@pytest.mark.parametrize("variant", WGRAD_VARIANTS, ids=_ids)
@pytest.mark.parametrize("shape", [S64, S1X1, STEM], ids=_ids)
def test_wgrad_variants_agree(shape, variant):
    """Two correct results differ by an fp16 ulp on a few elements at most
    (the split-K summation order differs); a non-atomic variant repeats its
    own bits exactly."""
    wtile, splits = variant
    c = _case(shape, torch.float16)
    ref = _wgrad(c, 1, 1)
    got = _wgrad(c, splits, wtile)
    err = _rel_err(got, ref.float().cpu())
    print(f"wgrad {shape} wtile={wtile} splits={splits}: {err:.3e}")
    assert got.dtype == torch.float16
    assert err < 5e-4, err
    assert _rel_err(got, c.dw) < TOL[torch.float16]
    if wtile != 4:
        assert torch.equal(_wgrad(c, splits, wtile), got)


@pytest.mark.parametrize("variant", [(0, 0), (1, 1), (0, 2), (4, 0)], ids=_ids)
@pytest.mark.parametrize("shape", [S64, S1X1, STEM], ids=_ids)
def test_wgrad_fp32_is_widened_fp16(shape, variant):
    wtile, splits = variant
    c = _case(shape, torch.float16)
    d = _wgrad(c, splits, wtile, True)
    assert d.dtype == torch.float32
    assert d.is_contiguous(memory_format=CL)
    assert torch.equal(d, d.half().float())
    if wtile != 4:   # the atomic slab's summation order is not repeatable
        assert torch.equal(d, _wgrad(c, splits, wtile, False).float())


# --------------------------------------------------------------------------
# fp16 range: overflow and subnormals
# --------------------------------------------------------------------------

def test_overflow_is_inf_not_saturated():
    """256 * 256 * 64 is far beyond 65504: every element of every pass is
    +inf (plain round-to-nearest-even, no saturation, no NaN), and the fp32
    weight gradient carries the inf to the loss scaler's check."""
    N, C, H, W, K = 2, 64, 8, 8, 64
    x = torch.full((N, C, H, W), 256.0, device=DEV,
                   dtype=torch.float16).contiguous(memory_format=CL)
    w = torch.full((K, C, 1, 1), 256.0, device=DEV,
                   dtype=torch.float16).contiguous(memory_format=CL)
    dy = torch.full((N, K, H, W), 256.0, device=DEV,
                    dtype=torch.float16).contiguous(memory_format=CL)
    C_ = _C()
    y = C_.conv_fwd_igemm(x, w, 1, 0)
    dx = C_.conv_dgrad_igemm(dy, rotate_wT(w), H, W, 1, 0)
    dw = C_.conv_wgrad_igemm(dy, x, 1, 1, 1, 0)
    dw32 = C_.conv_wgrad_igemm(dy, x, 1, 1, 1, 0, 0, 0, True)
    for name, t in (("y", y), ("dx", dx), ("dw", dw), ("dw32", dw32)):
        assert torch.isposinf(t).all(), name


# The 64 -> 64 3x3 layer at the size where the weight gradient of a dy scaled
# by 2^-18 is fp16-NORMAL (rms 3.4e-4): 8192 output pixels. On S64 (128
# pixels) the result itself is fp16-subnormal (rms 4e-5) and its own rounding
# is already 4.4e-4 of the 5e-4 bound, which would test the output format,
# not the operands.
SUBNORMAL_SHAPE = (8, 64, 32, 32, 64, 3, 1, 1)


def test_subnormal_operands_are_not_flushed():
    """dy * 2^-18 is subnormal in fp16 (|dy| ~ 4e-6 < 6.1e-5); the f16 MFMA
    must take such A/B operands unflushed. A flushed operand gives a zero
    weight gradient."""
    c = _case(SUBNORMAL_SHAPE, torch.float16, 2.0 ** -18)
    assert (c.dy.float().abs() < 2.0 ** -14).all()      # all subnormal
    assert (c.dy != 0).float().mean() > 0.9
    assert c.dw.pow(2).mean().sqrt() > 2.0 ** -14 * 4     # result is normal
    got = _wgrad(c)
    err = _rel_err(got, c.dw)
    print(f"subnormal dy wgrad: rel err {err:.3e}, "
          f"rms got {got.float().pow(2).mean().sqrt().item():.3e}")
    assert err < TOL[torch.float16], err


# --------------------------------------------------------------------------
# dtype checks
# --------------------------------------------------------------------------

def test_mixed_16bit_dtypes_raise():
    c = _case(S64, torch.float16)
    C_ = _C()
    with pytest.raises(RuntimeError, match="Half.*BFloat16|BFloat16.*Half"):
        C_.conv_fwd_igemm(c.x, c.w.bfloat16(), 1, 1)
    with pytest.raises(RuntimeError, match="Half.*BFloat16|BFloat16.*Half"):
        C_.conv_dgrad_igemm(c.dy, c.wT.bfloat16(), c.H, c.W, 1, 1)
    with pytest.raises(RuntimeError, match="Half.*BFloat16|BFloat16.*Half"):
        C_.conv_wgrad_igemm(c.dy.bfloat16(), c.x, 3, 3, 1, 1)
    w32 = c.w.float()
    with pytest.raises(RuntimeError, match="Half.*BFloat16|BFloat16.*Half"):
        C_.conv_prep_weight(w32, torch.empty_like(c.w),
                            torch.empty_like(c.wT, dtype=torch.bfloat16))


def test_prep_weight_rounds_to_the_shadow_dtype():
    C_ = _C()
    for shape in (S64, STEM):
        w32 = _case(shape, torch.float16).w.float() * 1.2345
        for dt in DTYPES:
            w16 = torch.empty_like(w32, dtype=dt)
            K, C, R, S = w32.shape
            wT = torch.empty((C, R, S, K), dtype=dt, device=DEV)
            C_.conv_prep_weight(w32, w16, wT)
            assert torch.equal(w16, w32.to(dt)), (shape, dt)
            assert torch.equal(wT, rotate_wT(w32.to(dt))), (shape, dt)
            assert torch.equal(C_.conv_build_wT(w16), wT), (shape, dt)


# --------------------------------------------------------------------------
# autograd and shadows under fp16 autocast
# --------------------------------------------------------------------------

@pytest.fixture
def no_autotune(monkeypatch):
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    return monkeypatch


def test_module_under_fp16_autocast(no_autotune):
    no_autotune.setenv("MI355X_CHECK_SHADOWS", "1")
    shape = (4, 64, 16, 16, 128, 3, 2, 1)
    N, C, H, W, K, R, stride, pad = shape
    conv = MI355Conv2d(C, K, R, stride=stride, padding=pad, bias=False)
    conv = conv.to(DEV).to(memory_format=CL)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=g)
    P = (H + 2 * pad - R) // stride + 1
    dy = torch.randn(N, K, P, P, generator=g)
    for dt in (torch.float16, torch.bfloat16):   # the second replaces the shadow
        xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        conv.weight.grad = None
        with torch.autocast("cuda", dtype=dt):
            y = conv(xd)
        assert y.dtype == dt and y.is_contiguous(memory_format=CL)
        y.backward(dy.to(DEV).to(dt).contiguous(memory_format=CL))
        sh = shadow_of(conv.weight)
        assert sh is not None and sh.dtype == dt and sh.w16.dtype == dt
        assert sh.wT.dtype == dt
        sh.check(conv.weight)
        assert conv.weight.grad.dtype == torch.float32
        assert xd.grad.dtype == torch.float32

        xr = x.to(dt).float().requires_grad_(True)
        wr = conv.weight.detach().cpu().to(dt).float().requires_grad_(True)
        yr = F.conv2d(xr, wr, None, stride, pad)
        dxr, dwr = torch.autograd.grad(yr, (xr, wr), dy.to(dt).float())
        errs = (_rel_err(y, yr.detach()), _rel_err(xd.grad, dxr),
                _rel_err(conv.weight.grad, dwr))
        print(f"module {dt}: y/dx/dw rel err", ["%.3e" % e for e in errs])
        assert max(errs) < TOL[dt], errs


# --------------------------------------------------------------------------
# SGD refresh of fp16 shadows
# --------------------------------------------------------------------------

SGD_SHAPES = [(64, 3, 3, 3), (5, 3, 3, 3), (64, 64, 3, 3), (128, 64, 1, 1)]


def _sgd_setup(dtypes):
    g = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(
        torch.randn(s, generator=g).to(DEV).contiguous(memory_format=CL))
        for s in SGD_SHAPES]
    grads = [[torch.randn(s, generator=g).to(DEV).contiguous(memory_format=CL)
              for s in SGD_SHAPES] for _ in range(2)]
    shadows = []
    for p, dt in zip(params, dtypes):
        if dt is None:
            shadows.append(None)
            continue
        sh = WeightShadow(p, dt)
        sh.refresh(p)
        p._mi355x_shadow = sh
        shadows.append(sh)
    opt = FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4)
    return params, grads, shadows, opt


def _sgd_run(params, grads, opt, steps):
    for i in range(steps):
        for p, g in zip(params, grads[i]):
            p.grad = g.clone()
        opt.step()


@pytest.mark.parametrize("dtypes", [
    (torch.float16,) * 4,
    (torch.float16, torch.bfloat16, torch.bfloat16, torch.float16),
], ids=["fp16", "mixed"])
def test_sgd_refreshes_fp16_shadows(monkeypatch, dtypes):
    monkeypatch.setenv("MI355X_WEIGHT_SHADOWS", "1")
    params, grads, shadows, opt = _sgd_setup(dtypes)
    _sgd_run(params, grads, opt, 2)
    monkeypatch.setenv("MI355X_WEIGHT_SHADOWS", "0")
    twin, tgrads, _, topt = _sgd_setup((None,) * 4)
    _sgd_run(twin, tgrads, topt, 2)
    for p, q, sh, dt in zip(params, twin, shadows, dtypes):
        what = (tuple(p.shape), dt)
        assert torch.equal(p, q), what
        assert torch.equal(opt.state[p]["momentum_buffer"],
                           topt.state[q]["momentum_buffer"]), what
        assert sh.w16.dtype == dt
        assert torch.equal(sh.w16, p.detach().to(dt)), what
        assert torch.equal(sh.wT, rotate_wT(p.detach().to(dt))), what
        assert sh.fresh(p), what
        assert sh.refreshes == 1, what      # the one in _sgd_setup


def test_skipped_step_leaves_weights_and_shadows(monkeypatch):
    monkeypatch.setenv("MI355X_WEIGHT_SHADOWS", "1")
    params, grads, shadows, opt = _sgd_setup((torch.float16,) * 4)
    before = [p.detach().clone() for p in params]
    scaler = DynamicLossScaler(init_scale=2.0 ** 16)
    for p, g in zip(params, grads[0]):
        p.grad = g.clone()
    params[2].grad[3, 5, 1, 2] = float("inf")
    assert scaler.unscale_([p.grad for p in params]) is True
    assert scaler.step(opt) is False
    assert scaler.scale == 2.0 ** 15
    for p, b, sh in zip(params, before, shadows):
        assert torch.equal(p, b)
        assert sh.fresh(p) and sh.refreshes == 1
        sh.check(p)


# --------------------------------------------------------------------------
# the switch is real
# --------------------------------------------------------------------------

def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA]


def _resnet_fp16_step():
    from mi355x_ddp.models import resnet18
    torch.manual_seed(0)
    model = MI355Conv2d.convert(resnet18().to(DEV)).to(memory_format=CL)
    x = torch.randn(16, 3, 32, 32, device=DEV).to(memory_format=CL)
    labels = torch.randint(0, 100, (16,), device=DEV)

    def step():
        # the fused loss takes fp16 logits as they are: F.cross_entropy would
        # add an fp32 cast whose backward is one more float -> half copy
        with torch.autocast("cuda", dtype=torch.float16):
            loss = softmax_cross_entropy(model(x), labels)
        loss.backward()
        return loss

    step()                    # first use: shadows are created and filled
    model.zero_grad(set_to_none=True)
    out = {}
    names = _kernel_names(lambda: out.setdefault("loss", step()))
    assert torch.isfinite(out["loss"])
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    nconv = sum(isinstance(m, MI355Conv2d) for m in model.modules())
    return names, nconv


def test_fp16_autocast_runs_the_native_kernels(no_autotune):
    mp = no_autotune
    mp.setenv("MI355X_NATIVE_CONV_FP16", "1")
    names, nconv = _resnet_fp16_step()
    assert names, "profiler recorded no GPU kernels"
    assert any("conv_igemm_kernel" in n for n in names), names
    assert any("conv_wgrad" in n for n in names), names
    # float -> half: the image, the fc weight and the fc bias; no conv weight
    f2h = sum("float16_copy_kernel_cuda" in n for n in names)
    print(f"float -> half copies, native: {f2h}")
    assert f2h <= 3, (f2h, names)

    mp.setenv("MI355X_NATIVE_CONV_FP16", "0")
    names_off, _ = _resnet_fp16_step()
    assert names_off, "profiler recorded no GPU kernels"
    assert not any("conv_igemm_kernel" in n for n in names_off), names_off
    assert not any("conv_wgrad" in n for n in names_off), names_off
    # and every conv weight is cast again
    f2h_off = sum("float16_copy_kernel_cuda" in n for n in names_off)
    print(f"float -> half copies, MIOpen routing: {f2h_off} ({nconv} convs)")
    assert f2h_off >= f2h + nconv, (f2h_off, f2h, nconv)
