"""Split-K 128x128 tile of the conv forward / input-grad kernels (MI355X).

A split result differs from the unsplit 128x128 tile only in the order of the
fp32 partial sums before the single rounding to 16 bits, so the bounds are the
ones the project already uses for that situation: 5e-3 relative norm between
launch variants (test_conv_wgrad_splits_agree) and 2e-2 against the fp32
reference (test_conv_fwd_parity).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
T228 = 228
SPLITS = (2, 3, 4, 5)
DTYPES = (torch.bfloat16, torch.float16)

# (N, C, H, W, K, R, stride, pad)
L4 = (8, 512, 4, 4, 512, 3, 1, 1)      # one M-tile, 4 N-tiles, 72 K-tiles
L3_RAGGED = (3, 256, 8, 8, 256, 3, 1, 1)   # M = 192: ragged edge tile
L4_S2 = (8, 256, 8, 8, 512, 3, 2, 1)   # stride 2: dgrad is the parity path
N160 = (8, 256, 8, 8, 160, 1, 1, 0)    # N = 160, 4 K-tiles: splits 5 clamps
SHAPES = (L4, L3_RAGGED, L4_S2, N160)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """Seeded operands, the fp32 references and the unsplit 128x128 results
    of one (shape, dtype): computed once, shared, never modified."""
    from mi355x_ddp import _C
    N, C, H, W, K, R, stride, pad = shape
    g = torch.Generator(device=DEV).manual_seed(hash(shape) % (2**31))
    x = torch.randn(N, C, H, W, generator=g, device=DEV) \
        .to(memory_format=torch.channels_last)
    w = torch.randn(K, C, R, R, generator=g, device=DEV) \
        .to(memory_format=torch.channels_last) / (C * R * R) ** 0.5
    x.requires_grad_(True)
    y = F.conv2d(x, w, None, stride, pad)
    dy = torch.randn(y.shape, generator=g, device=DEV) \
        .to(memory_format=torch.channels_last)
    (y * dy).sum().backward()
    c = Case()
    c.H, c.W, c.stride, c.pad = H, W, stride, pad
    c.ref_y, c.ref_dx = y.detach(), x.grad.detach()
    c.x, c.w, c.dy = x.detach().to(dtype), w.to(dtype), dy.to(dtype)
    c.wT = c.w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    c.y228 = _C.conv_fwd_igemm(c.x, c.w, stride, pad, T228)
    c.dx228 = _C.conv_dgrad_igemm(c.dy, c.wT, H, W, stride, pad, T228)
    return c


def _rel(got, ref):
    return ((got.float() - ref.float()).norm() /
            ref.float().norm().clamp_min(1e-12)).item()


def _fwd(c, tile=0, splits=1):
    from mi355x_ddp import _C
    return _C.conv_fwd_igemm(c.x, c.w, c.stride, c.pad, tile, splits)


def _dgrad(c, tile=0, splits=1):
    from mi355x_ddp import _C
    return _C.conv_dgrad_igemm(c.dy, c.wT, c.H, c.W, c.stride, c.pad, tile,
                               splits)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_splitk_fwd_agrees(shape, dtype):
    c = _case(shape, dtype)
    for s in SPLITS:
        got = _fwd(c, T228, s)
        assert got.shape == c.ref_y.shape and got.dtype == dtype
        assert got.is_contiguous(memory_format=torch.channels_last)
        e_var, e_ref = _rel(got, c.y228), _rel(got, c.ref_y)
        print(f"fwd {shape} {dtype} splits={s}: vs 228 {e_var:.2e}, "
              f"vs fp32 {e_ref:.2e}")
        assert e_var < 5e-3, (shape, s, e_var)
        assert e_ref < 2e-2, (shape, s, e_ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
@pytest.mark.parametrize("shape", (L4, L3_RAGGED, N160), ids=str)
def test_splitk_dgrad_agrees(shape, dtype):
    c = _case(shape, dtype)
    for s in SPLITS:
        got = _dgrad(c, T228, s)
        assert got.shape == c.ref_dx.shape and got.dtype == dtype
        e_var, e_ref = _rel(got, c.dx228), _rel(got, c.ref_dx)
        print(f"dgrad {shape} {dtype} splits={s}: vs 228 {e_var:.2e}, "
              f"vs fp32 {e_ref:.2e}")
        assert e_var < 5e-3, (shape, s, e_var)
        assert e_ref < 2e-2, (shape, s, e_ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
def test_splitk_stride2_dgrad_takes_parity_path(dtype):
    c = _case(L4_S2, dtype)
    for s in SPLITS:
        assert torch.equal(_dgrad(c, T228, s), c.dx228), s


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
def test_splitk_clamps_to_the_k_tile_count(dtype):
    """4 K-tiles: a request for 5 slices runs 4, with the bits of 4."""
    c = _case(N160, dtype)
    assert torch.equal(_fwd(c, T228, 5), _fwd(c, T228, 4))
    assert torch.equal(_fwd(c, T228, 1000), _fwd(c, T228, 4))


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
def test_splitk_fallbacks(dtype):
    """Shapes the 128x128 tile does not take ignore `splits`."""
    for shape in ((8, 3, 32, 32, 64, 3, 1, 1),      # C = 3 stem: not FAST
                  (8, 64, 16, 16, 64, 3, 1, 1)):    # N = 64 < 96
        c = _case(shape, dtype)
        for s in (2, 4):
            assert torch.equal(_fwd(c, T228, s), c.y228), (shape, s)
            assert torch.equal(_dgrad(c, T228, s), c.dx228), (shape, s)
    # N160's input-grad gathers 160 channels: not FAST either
    c = _case(N160, dtype)
    assert torch.equal(_dgrad(c, T228, 4), c.dx228)
    # splits without the 128x128 tile is ignored as well
    c = _case(L4, dtype)
    assert torch.equal(_fwd(c, 64, 4), _fwd(c, 64))
    assert torch.equal(_dgrad(c, 128, 4), _dgrad(c, 128))


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
def test_splitk_deterministic_and_default_unchanged(dtype):
    for shape in (L4, L3_RAGGED):
        c = _case(shape, dtype)
        for s in SPLITS:
            assert torch.equal(_fwd(c, T228, s), _fwd(c, T228, s)), (shape, s)
            assert torch.equal(_dgrad(c, T228, s), _dgrad(c, T228, s)), \
                (shape, s)
        # the heuristic (tile=0) never splits: same bits as the plain tiles
        y0, dx0 = _fwd(c), _dgrad(c)
        for t in (64, 128):
            assert torch.equal(y0, _fwd(c, t)), (shape, t)
            assert torch.equal(dx0, _dgrad(c, t)), (shape, t)


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp16"))
def test_splitk_end_to_end_through_the_tuner_cache(dtype):
    """_ConvIGEMM with (228, 4) pinned for fwd and dgrad runs the split
    kernels and its gradients stay within 2e-2 of fp32 autograd."""
    from mi355x_ddp.ops import conv as conv_mod
    c = _case(L4, dtype)
    N, C, H, W, K, R, stride, pad = L4
    x = c.x.clone().requires_grad_(True)
    w = c.w.clone().requires_grad_(True)
    yshape = tuple(c.ref_y.shape)
    keys = {
        conv_mod._tune_key("fwd", dtype, x.shape, w.shape, stride, pad):
            (T228, 4),
        conv_mod._tune_key("dgrad", dtype, yshape, (C, R, R, K), stride, pad):
            (T228, 4),
        # keep the weight-grad on its default launch: no probing in a test
        conv_mod._tune_key("wgrad_tile", dtype, yshape, x.shape, R, stride,
                           pad): (0, 0),
        conv_mod._tune_key("wgrad_splits", dtype, yshape, x.shape, R, stride,
                           pad, 0): (0, 0),
    }
    saved = dict(conv_mod._TUNE_CACHE)
    conv_mod._TUNE_CACHE.update(keys)
    try:
        y = conv_mod.conv2d(x, w, (stride, stride), (pad, pad))
        y.backward(c.dy)
        report = conv_mod.tune_report()
    finally:
        conv_mod._TUNE_CACHE.clear()
        conv_mod._TUNE_CACHE.update(saved)
    assert "split-K x4" in report
    assert torch.equal(y.detach(), _fwd(c, T228, 4))
    assert torch.equal(x.grad, _dgrad(c, T228, 4))
    assert _rel(y, c.ref_y) < 2e-2
    assert _rel(x.grad, c.ref_dx) < 2e-2
    # weight grad against fp32 autograd on the same fp32 operands
    xf = c.x.float()
    wf = c.w.float().requires_grad_(True)
    F.conv2d(xf, wf, None, stride, pad).backward(c.dy.float())
    assert _rel(w.grad, wf.grad) < 2e-2
