"""Split-K wgrad: fragment-order partial slabs and their reduce (MI355X).

Exact-arithmetic agreement with an fp64 reference over every tile variant
and split count, bit-determinism of repeated calls, and a rounding bound on
random data for the heuristic path.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (N, C, H, W, K, R, stride, pad)
SHAPES = [
    (8, 64, 32, 32, 64, 3, 1, 1),     # M=64 < v2 tile, N=576 ragged vs 128, 128 chunks
    (8, 128, 16, 16, 128, 3, 1, 1),   # 32 chunks: splits clamp below 128
    (8, 256, 8, 8, 512, 3, 2, 1),     # 2 chunks; wide-stage tiles get one slice
    (8, 64, 32, 32, 256, 1, 1, 0),    # LIN kernels, 256x64 tile
    (3, 64, 32, 32, 64, 3, 1, 1),     # K=3072: unequal chunk counts per slice
    (4, 24, 9, 9, 40, 3, 1, 1),       # generic non-FAST path, ragged M and N
    (5, 3, 30, 30, 64, 3, 1, 1),      # stem, padded channels, ragged M
]
WTILES = [0, 1, 2, 3, 5, 6, 8, 9]
SPLITS = [0, -1, 1, 2, 3, 7, 32, 128, 1000]   # -1: residency-sized count
MAX_POS = 256   # non-zero (n, p, q) positions of dy -> |dw| <= 256, exact


def _out_hw(shape):
    N, C, H, W, K, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def _ref_dw(x, dy, shape):
    """fp64 weight gradient on the CPU, (K, C, R, R)."""
    N, C, H, W, K, R, stride, pad = shape
    return torch.nn.grad.conv2d_weight(
        x.double().cpu().contiguous(), (K, C, R, R),
        dy.double().cpu().contiguous(), stride=stride, padding=pad)


@functools.lru_cache(maxsize=None)
def _exact_case(shape):
    """x in {-1,0,1}; dy in {-1,0,1}, non-zero at <= MAX_POS (n,p,q) rows with
    every 64-row K-chunk hit at least once. Returns (x, dy, fp64 reference)."""
    N, C, H, W, K, R, stride, pad = shape
    P, Q = _out_hw(shape)
    g = torch.Generator().manual_seed(1234 + sum(shape))
    x = torch.randint(-1, 2, (N, C, H, W), generator=g).float()
    npq = N * P * Q
    nchunks = (npq + 63) // 64
    assert nchunks <= MAX_POS
    rows = []
    for c in range(nchunks):
        lo, hi = c * 64, min(c * 64 + 64, npq)
        rows.append(int(torch.randint(lo, hi, (1,), generator=g)))
    extra = torch.randperm(npq, generator=g)[:MAX_POS - nchunks].tolist()
    rows = sorted(set(rows) | set(extra))[:MAX_POS]
    dy_rows = torch.zeros(npq, K)
    vals = torch.randint(-1, 2, (len(rows), K), generator=g).float()
    vals[:, 0] = 1.0   # no chosen row is all-zero
    dy_rows[rows] = vals
    dy = dy_rows.view(N, P, Q, K).permute(0, 3, 1, 2)   # NKPQ view of NHWC data
    ref = _ref_dw(x, dy, shape)
    assert ref.abs().max() <= MAX_POS
    xb = x.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    dyb = dy.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    return xb, dyb, ref


@functools.lru_cache(maxsize=None)
def _random_case(shape):
    N, C, H, W, K, R, stride, pad = shape
    P, Q = _out_hw(shape)
    g = torch.Generator().manual_seed(4321 + sum(shape))
    x = torch.randn(N, C, H, W, generator=g).bfloat16()
    dy = torch.randn(N, K, P, Q, generator=g).bfloat16()
    ref = _ref_dw(x, dy, shape)
    xb = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dyb = dy.to(DEV).contiguous(memory_format=torch.channels_last)
    return xb, dyb, ref


@pytest.mark.parametrize("wtile", WTILES)
@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_exact_all_tiles_and_splits(shape, wtile):
    """Integer-valued data: every (wtile, splits) must equal the fp64
    reference exactly — catches a dropped or double-counted chunk, a wrong
    un-permute, an edge-tile leak and an unwritten slab."""
    from mi355x_ddp import _C
    R, stride, pad = shape[5], shape[6], shape[7]
    x, dy, ref = _exact_case(shape)
    for splits in SPLITS:
        got = _C.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, wtile)
        assert got.shape == ref.shape
        assert got.is_contiguous(memory_format=torch.channels_last)
        got64 = got.double().cpu()
        assert torch.equal(got64, ref), (
            f"{shape} wtile={wtile} splits={splits}: "
            f"{int((got64 != ref).sum())} of {ref.numel()} differ, "
            f"max abs diff {float((got64 - ref).abs().max())}")


@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad_deterministic(shape):
    """Same inputs, same (wtile, splits): same bits on consecutive calls."""
    from mi355x_ddp import _C
    R, stride, pad = shape[5], shape[6], shape[7]
    x, dy, _ = _random_case(shape)
    for wtile in WTILES:
        for splits in SPLITS:
            a = _C.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, wtile)
            b = _C.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, wtile)
            assert torch.equal(a, b), f"{shape} wtile={wtile} splits={splits}"


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]])
def test_wgrad_heuristic_rounding_bound(shape):
    """bf16 random-normal inputs, heuristic path: the output is one bf16
    round-to-nearest (<= 2^-9 relative per element) of an fp32 accumulation
    of at most 8192 terms; norm-wise relative error must stay below 2^-8."""
    from mi355x_ddp import _C
    R, stride, pad = shape[5], shape[6], shape[7]
    x, dy, ref = _random_case(shape)
    got = _C.conv_wgrad_igemm(dy, x, R, R, stride, pad, 0, 0).double().cpu()
    err = float((got - ref).norm() / ref.norm())
    print(f"{shape}: norm-wise rel err {err:.3e} (bound {2.0 ** -8:.3e})")
    assert err < 2.0 ** -8
