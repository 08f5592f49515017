"""The one-launch BatchNorm tails against the chain of ops they replace.

Reference: the exported ops `bn_stats_packed -> bn_finalize -> bn_fwd` and
`bn_bwd_reduce_packed -> bn_bwd`, which stay as they were. The tail kernels
reduce the partials in bn_reduce_partials_kernel's order and use the same
expressions, so everything observable is compared with torch.equal: mean,
invstd, running stats, y, the backward sums (= dbeta, dgamma), dx, dres.

The coefficient rows (scale, shift, A, B, D) are internal to bn_fwd / bn_bwd
in the old chain. They are checked here (a) through y / dx / dres, which are
computed from them and must be bit-equal, and (b) directly: scale and A are a
single fp32 product and must equal torch's; shift, B and D (2-4 roundings,
one possibly fused) must be within a few fp32 ulps of an fp64 evaluation.
"""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
EPS32 = 2.0 ** -24  # fp32 unit roundoff

# (N, C, H, W) bf16 channels_last -> expected split (rows of the partial)
V2_SHAPES = {
    (2, 8, 3, 3): 1,        # C=8: tpr=1, one partial row
    (2, 512, 5, 5): 13,     # rpb=4: fewer partial rows than threads
    (8, 512, 16, 16): 512,  # two loads per thread in the tail's j loop
    (3, 2048, 2, 2): 12,    # tpr=256, rpb=1
    (4, 64, 8, 8): 8,       # mid case
}
# relu, residual, momentum, running stats given
VARIANTS = [
    (True, False, 0.1, True),
    (False, False, 1.0, True),
    (True, True, 0.1, False),
]


@pytest.fixture(autouse=True)
def _native_required():
    from mi355x_ddp.ops import _backend
    assert _backend.extension_available(), "HIP extension must be built"
    yield


def _C():
    from mi355x_ddp.ops import _backend
    return _backend.C()


def _inputs(shape, seed=0, fmt=torch.channels_last, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    N, C, H, W = shape

    def t():
        return (torch.randn(shape, device=DEV, generator=g) * 1.5 + 0.25) \
            .to(dtype).contiguous(memory_format=fmt)
    x, res, dy = t(), t(), t()
    w = torch.rand(C, device=DEV, generator=g) + 0.5
    b = torch.randn(C, device=DEV, generator=g)
    return x, res, dy, w, b


def _running(C, given):
    if not given:
        return None, None
    return (torch.linspace(-1, 1, C, device=DEV),
            torch.linspace(0.5, 2, C, device=DEV))


def _empty(x):
    return torch.empty(0, device=x.device, dtype=x.dtype)


def _old_fwd(x, res, w, b, rm, rv, momentum, eps, relu):
    cnt = float(x.numel() // x.shape[1])
    packed = _C().bn_stats_packed(x)
    mean, invstd = _C().bn_finalize(packed, cnt, momentum, eps, rm, rv)
    y = _C().bn_fwd(x, w, b, mean, invstd, relu,
                    res if res is not None else _empty(x))
    return mean, invstd, y


def _old_bwd(dy, x, w, mean, invstd, y, relu, training, need_dres):
    C = x.shape[1]
    cnt = float(x.numel() // C)
    packed = _C().bn_bwd_reduce_packed(dy, x, mean, invstd, y, relu)
    dx, dres = _C().bn_bwd(dy, x, w, mean, invstd, packed[:C], packed[C:],
                           cnt, y, relu, training, need_dres)
    return packed, dx, dres


def _check_fwd_coeffs(stats, w, b):
    mean, invstd, scale, shift = stats
    assert torch.equal(scale, w * invstd)
    ref = b.double() - mean.double() * scale.double()
    bound = 4 * EPS32 * (b.abs() + (mean * scale).abs()).double()
    assert bool(((shift.double() - ref).abs() <= bound).all())


def _check_bwd_coeffs(coeffs, w, mean, invstd, sums, inv_count, training):
    A, B, D = coeffs
    assert torch.equal(A, w * invstd)
    if not training:
        assert not B.any() and not D.any()
        return
    ic = float(torch.tensor(inv_count, dtype=torch.float32))
    a, s_dy, s_dyx = A.double(), sums[0].double(), sums[1].double()
    refB = -a * invstd.double() * s_dyx * ic
    assert bool(((B.double() - refB).abs() <= 8 * EPS32 * refB.abs()).all())
    t1, t2 = -a * s_dy * ic, B.double() * mean.double()
    assert bool(((D.double() - (t1 - t2)).abs()
                 <= 8 * EPS32 * (t1.abs() + t2.abs())).all())


@pytest.mark.parametrize("relu,residual,momentum,running", VARIANTS)
@pytest.mark.parametrize("shape", list(V2_SHAPES))
def test_tail_chain_bit_equal_to_old_chain(shape, relu, residual, momentum,
                                           running):
    N, C, H, W = shape
    cnt = float(N * H * W)
    x, res, dy, w, b = _inputs(shape)
    res = res if residual else None
    assert _C().bn_v2_ok(x)

    rm0, rv0 = _running(C, running)
    mean0, invstd0, y0 = _old_fwd(x, res, w, b, rm0, rv0, momentum, 1e-5, relu)
    packed0, dx0, dres0 = _old_bwd(dy, x, w, mean0, invstd0, y0, relu, True,
                                   residual)

    rm1, rv1 = _running(C, running)
    part = _C().bn_stats_partial(x)
    assert tuple(part.shape) == (V2_SHAPES[shape], 2 * C)
    stats, mean1, invstd1 = _C().bn_fwd_tail(part, w, b, cnt, momentum, 1e-5,
                                             rm1, rv1)
    y1 = _C().bn_fwd_apply(x, stats, relu, res)
    assert tuple(stats.shape) == (4, C) and stats.dtype == torch.float32
    assert torch.equal(mean1, mean0) and torch.equal(stats[0], mean0)
    assert torch.equal(invstd1, invstd0) and torch.equal(stats[1], invstd0)
    if running:
        assert torch.equal(rm1, rm0) and torch.equal(rv1, rv0)
    _check_fwd_coeffs(stats, w, b)
    assert torch.equal(y1, y0)
    assert y1.is_contiguous(memory_format=torch.channels_last)

    bpart = _C().bn_bwd_reduce_partial(dy, x, mean1, invstd1, y1, relu)
    assert tuple(bpart.shape) == (V2_SHAPES[shape], 2 * C)
    dbeta, dgamma, coeffs = _C().bn_bwd_tail(bpart, w, mean1, invstd1,
                                             1.0 / cnt, True)
    dx1, dres1 = _C().bn_bwd_apply(dy, x, y1, coeffs, relu, True, residual)
    assert torch.equal(dbeta, packed0[:C])
    assert torch.equal(dgamma, packed0[C:])
    _check_bwd_coeffs(coeffs, w, mean1, invstd1, (dbeta, dgamma), 1.0 / cnt,
                      True)
    assert torch.equal(dx1, dx0)
    if residual:
        assert torch.equal(dres1, dres0)
    else:
        assert dres1.numel() == 0

    # the SyncBN form of the tail: the same sums twice, in separate storage
    lb, lg, packed1 = _C().bn_bwd_tail_dup(bpart)
    assert torch.equal(lb, packed0[:C]) and torch.equal(lg, packed0[C:])
    assert torch.equal(packed1, packed0)
    packed1.zero_()
    assert torch.equal(lb, packed0[:C]) and torch.equal(lg, packed0[C:])


@pytest.mark.parametrize("as_2d", [True, False])
def test_fwd_tail_on_packed_row_equals_finalize(as_2d):
    # split == 1: what the tail sees after the SyncBN all_reduce
    shape = (4, 64, 8, 8)
    N, C, H, W = shape
    cnt = 2.0 * N * H * W  # as if two ranks had contributed
    x, _, _, w, b = _inputs(shape, seed=1)
    packed = _C().bn_stats_packed(x) * 2
    rm0, rv0 = _running(C, True)
    rm1, rv1 = _running(C, True)
    mean0, invstd0 = _C().bn_finalize(packed, cnt, 0.1, 1e-5, rm0, rv0)
    stats, mean1, invstd1 = _C().bn_fwd_tail(
        packed.view(1, 2 * C) if as_2d else packed, w, b, cnt, 0.1, 1e-5,
        rm1, rv1)
    assert torch.equal(mean1, mean0) and torch.equal(invstd1, invstd0)
    assert torch.equal(rm1, rm0) and torch.equal(rv1, rv0)
    _check_fwd_coeffs(stats, w, b)
    y0 = _C().bn_fwd(x, w, b, mean0, invstd0, True, _empty(x))
    assert torch.equal(_C().bn_fwd_apply(x, stats, True, None), y0)


def test_bwd_tail_eval_coeffs():
    shape = (4, 64, 8, 8)
    N, C, H, W = shape
    x, _, dy, w, b = _inputs(shape, seed=2)
    mean = torch.randn(C, device=DEV)
    invstd = torch.rand(C, device=DEV) + 0.5
    y = _C().bn_fwd(x, w, b, mean, invstd, True, _empty(x))
    packed0, dx0, _ = _old_bwd(dy, x, w, mean, invstd, y, True, False, False)
    part = _C().bn_bwd_reduce_partial(dy, x, mean, invstd, y, True)
    dbeta, dgamma, coeffs = _C().bn_bwd_tail(part, w, mean, invstd,
                                             1.0 / (N * H * W), False)
    assert torch.equal(dbeta, packed0[:C]) and torch.equal(dgamma, packed0[C:])
    _check_bwd_coeffs(coeffs, w, mean, invstd, (dbeta, dgamma), 0.0, False)
    dx1, _ = _C().bn_bwd_apply(dy, x, y, coeffs, True, False, False)
    assert torch.equal(dx1, dx0)


def _module_step(bn, x, res, dy, relu):
    from mi355x_ddp.ops import bn_add_relu, bn_relu
    x = x.clone().requires_grad_(True)
    if res is not None:
        res = res.clone().requires_grad_(True)
        y = bn_add_relu(x, res, bn)
    else:
        y = bn_relu(x, bn, relu=relu)
    y.backward(dy)
    return y.detach(), x.grad, (res.grad if res is not None else None)


def _bn_module(C, w, b, dtype=torch.float32):
    bn = nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
        bn.running_mean.copy_(torch.linspace(-1, 1, C))
        bn.running_var.copy_(torch.linspace(0.5, 2, C))
    return bn


@pytest.mark.parametrize("relu,residual", [(True, False), (False, False),
                                           (True, True)])
@pytest.mark.parametrize("shape", [(2, 512, 5, 5), (8, 512, 16, 16),
                                   (4, 64, 8, 8)])
def test_module_api_matches_old_chain_and_grads_do_not_alias(shape, relu,
                                                             residual):
    N, C, H, W = shape
    x, res, dy, w, b = _inputs(shape, seed=3)
    res = res if residual else None
    bn = _bn_module(C, w, b)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    mean0, invstd0, y0 = _old_fwd(x, res, w, b, rm0, rv0, 0.1, bn.eps, relu)
    packed0, dx0, dres0 = _old_bwd(dy, x, w, mean0, invstd0, y0, relu, True,
                                   residual)

    y1, dx1, dres1 = _module_step(bn, x, res, dy, relu)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    if residual:
        assert torch.equal(dres1, dres0)
    assert torch.equal(bn.running_mean, rm0)
    assert torch.equal(bn.running_var, rv0)
    gw, gb = bn.weight.grad, bn.bias.grad
    assert gw.dtype == torch.float32 and gw.is_contiguous()
    assert torch.equal(gb, packed0[:C]) and torch.equal(gw, packed0[C:])

    # a second step on other data must not write into the first step's grads
    bn.weight.grad = None
    bn.bias.grad = None
    x2, res2, dy2, _, _ = _inputs(shape, seed=4)
    _module_step(bn, x2, res2 if residual else None, dy2, relu)
    assert torch.equal(gb, packed0[:C]) and torch.equal(gw, packed0[C:])
    assert not torch.equal(bn.weight.grad, gw)
    # and accumulating into an existing grad adds, as for any parameter
    before = bn.weight.grad.clone()
    _module_step(bn, x, res, dy, relu)
    assert torch.allclose(bn.weight.grad, before + gw, rtol=1e-6, atol=1e-6)


def test_module_api_eval_mode():
    shape = (4, 64, 8, 8)
    N, C, H, W = shape
    x, _, dy, w, b = _inputs(shape, seed=5)
    bn = _bn_module(C, w, b).eval()
    mean = bn.running_mean.clone()
    invstd = torch.rsqrt(bn.running_var + bn.eps)
    y0 = _C().bn_fwd(x, w, b, mean, invstd, True, _empty(x))
    packed0, dx0, _ = _old_bwd(dy, x, w, mean, invstd, y0, True, False, False)
    y1, dx1, _ = _module_step(bn, x, None, dy, True)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    assert torch.equal(bn.running_mean, mean)
    assert torch.equal(bn.bias.grad, packed0[:C])
    assert torch.equal(bn.weight.grad, packed0[C:])


# Inputs that do not take the tail: bn_relu must still give the old chain's
# results. The first two reduce with a single block per channel (one atomic
# add onto zero), so they are bit-reproducible; the NHWC width 24 sums 32
# per-pixel atomics per channel in scheduling order, so its stats carry a
# reordering error of at most 32 fp32 roundings and y / dx may differ by one
# bf16 rounding (2^-8 relative).
@pytest.mark.parametrize("shape,fmt,dtype,exact", [
    ((2, 16, 8, 8), torch.contiguous_format, BF16, True),
    ((2, 16, 4, 4), torch.contiguous_format, torch.float32, True),
    ((2, 24, 4, 4), torch.channels_last, BF16, False),
])
def test_fallback_paths_unchanged(shape, fmt, dtype, exact):
    N, C, H, W = shape
    x, _, dy, w, b = _inputs(shape, seed=6, fmt=fmt, dtype=dtype)
    assert not _C().bn_v2_ok(x)
    bn = _bn_module(C, w, b)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    mean0, invstd0, y0 = _old_fwd(x, None, w, b, rm0, rv0, 0.1, bn.eps, True)
    packed0, dx0, _ = _old_bwd(dy, x, w, mean0, invstd0, y0, True, True, False)
    y1, dx1, _ = _module_step(bn, x, None, dy, True)
    if exact:
        def same(a, ref):
            return torch.equal(a, ref)
    else:
        def same(a, ref):
            return torch.allclose(a.float(), ref.float(), rtol=2.0 ** -7,
                                  atol=2.0 ** -7)
    assert same(y1, y0) and same(dx1, dx0)
    assert same(bn.running_mean, rm0) and same(bn.running_var, rv0)
    assert same(bn.bias.grad, packed0[:C])
    assert same(bn.weight.grad, packed0[C:])
