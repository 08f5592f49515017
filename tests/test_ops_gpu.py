"""HIP kernel numerics vs plain PyTorch fp32 references (runs on MI355X).

Every native op is compared against an eager fp32 torch composition on the
same data; bf16/fp16 variants use dtype-appropriate tolerance bands.
"""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [  # every ResNet18/50 CIFAR stage shape
    (8, 64, 32, 32),
    (8, 128, 16, 16),
    (8, 256, 8, 8),
    (8, 512, 4, 4),
]


def tol(dtype):
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else \
        dict(atol=5e-2, rtol=5e-2)


@pytest.fixture(autouse=True)
def _native_required():
    from mi355x_ddp.ops import _backend
    assert _backend.extension_available(), "HIP extension must be built"
    yield


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_stats_kernel(shape, dtype):
    from mi355x_ddp.ops import _backend
    x = torch.randn(*shape, device=DEV, dtype=dtype)
    s, sq = _backend.C().bn_stats(x)
    xf = x.float()
    assert torch.allclose(s, xf.sum((0, 2, 3)), **tol(dtype))
    assert torch.allclose(sq, (xf * xf).sum((0, 2, 3)), **tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("residual", [False, True])
def test_bn_fwd_kernel(dtype, relu, residual):
    from mi355x_ddp.ops import _backend
    N, C, H, W = 4, 32, 8, 8
    x = torch.randn(N, C, H, W, device=DEV, dtype=dtype)
    res = torch.randn_like(x) if residual else torch.empty(0, device=DEV, dtype=dtype)
    w = torch.rand(C, device=DEV) + 0.5
    b = torch.randn(C, device=DEV)
    mean = torch.randn(C, device=DEV)
    invstd = torch.rand(C, device=DEV) + 0.5
    y = _backend.C().bn_fwd(x, w, b, mean, invstd, relu, res)
    sh = (1, -1, 1, 1)
    ref = (x.float() - mean.view(sh)) * invstd.view(sh) * w.view(sh) + b.view(sh)
    if residual:
        ref = ref + res.float()
    if relu:
        ref = F.relu(ref)
    assert torch.allclose(y.float(), ref.to(dtype).float(), **tol(dtype))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_bn_relu_autograd_vs_torch(training, dtype):
    from mi355x_ddp.ops import bn_relu
    torch.manual_seed(0)
    bn = nn.BatchNorm2d(64).to(DEV)
    ref_bn = nn.BatchNorm2d(64).to(DEV)
    ref_bn.load_state_dict(bn.state_dict())
    bn.train(training), ref_bn.train(training)

    x1 = torch.randn(8, 64, 16, 16, device=DEV, dtype=dtype, requires_grad=True)
    x2 = x1.detach().float().requires_grad_(True)

    y = bn_relu(x1, bn)
    y_ref = F.relu(ref_bn(x2))
    assert torch.allclose(y.float(), y_ref, **tol(dtype))

    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype))
    y_ref.backward(g)
    assert torch.allclose(x1.grad.float(), x2.grad, **tol(dtype))
    # dgamma/dbeta are O(sqrt(N*S))-term sums of bf16-quantised products while
    # the reference sums fp32 copies of the same inputs — allow absolute noise
    # proportional to the dtype's input quantisation, not a kernel tolerance.
    gtol = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else \
        dict(atol=2e-1, rtol=2e-2)
    assert torch.allclose(bn.weight.grad, ref_bn.weight.grad, **gtol)
    assert torch.allclose(bn.bias.grad, ref_bn.bias.grad, **gtol)
    if training:
        assert torch.allclose(bn.running_mean, ref_bn.running_mean, atol=1e-3)
        assert torch.allclose(bn.running_var, ref_bn.running_var, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_bn_add_relu_autograd_vs_torch(dtype):
    from mi355x_ddp.ops import bn_add_relu
    torch.manual_seed(1)
    bn = nn.BatchNorm2d(128).to(DEV)
    ref_bn = nn.BatchNorm2d(128).to(DEV)
    ref_bn.load_state_dict(bn.state_dict())

    x1 = torch.randn(4, 128, 8, 8, device=DEV, dtype=dtype, requires_grad=True)
    r1 = torch.randn(4, 128, 8, 8, device=DEV, dtype=dtype, requires_grad=True)
    x2 = x1.detach().float().requires_grad_(True)
    r2 = r1.detach().float().requires_grad_(True)

    y = bn_add_relu(x1, r1, bn)
    y_ref = F.relu(ref_bn(x2) + r2)
    assert torch.allclose(y.float(), y_ref, **tol(dtype))
    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype))
    y_ref.backward(g)
    assert torch.allclose(x1.grad.float(), x2.grad, **tol(dtype))
    assert torch.allclose(r1.grad.float(), r2.grad, **tol(dtype))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_stats_kernel_nhwc(shape, dtype):
    from mi355x_ddp.ops import _backend
    x = torch.randn(*shape, device=DEV, dtype=dtype) \
        .to(memory_format=torch.channels_last)
    s, sq = _backend.C().bn_stats(x)
    xf = x.float()
    assert torch.allclose(s, xf.sum((0, 2, 3)), **tol(dtype))
    assert torch.allclose(sq, (xf * xf).sum((0, 2, 3)), **tol(dtype))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_bn_relu_nhwc_vs_torch(training, dtype):
    """channels_last inputs run the NHWC kernels; reference is fp32 NCHW."""
    from mi355x_ddp.ops import bn_relu
    torch.manual_seed(0)
    bn = nn.BatchNorm2d(64).to(DEV)
    ref_bn = nn.BatchNorm2d(64).to(DEV)
    ref_bn.load_state_dict(bn.state_dict())
    bn.train(training), ref_bn.train(training)

    x1 = torch.randn(8, 64, 16, 16, device=DEV, dtype=dtype) \
        .to(memory_format=torch.channels_last).requires_grad_(True)
    x2 = x1.detach().float().contiguous().requires_grad_(True)

    y = bn_relu(x1, bn)
    assert y.is_contiguous(memory_format=torch.channels_last)
    y_ref = F.relu(ref_bn(x2))
    assert torch.allclose(y.float().contiguous(), y_ref, **tol(dtype))

    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype).to(memory_format=torch.channels_last))
    y_ref.backward(g)
    assert torch.allclose(x1.grad.float().contiguous(), x2.grad, **tol(dtype))
    gtol = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else \
        dict(atol=2e-1, rtol=2e-2)
    assert torch.allclose(bn.weight.grad, ref_bn.weight.grad, **gtol)
    assert torch.allclose(bn.bias.grad, ref_bn.bias.grad, **gtol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_bn_add_relu_nhwc_vs_torch(dtype):
    from mi355x_ddp.ops import bn_add_relu
    torch.manual_seed(1)
    bn = nn.BatchNorm2d(128).to(DEV)
    ref_bn = nn.BatchNorm2d(128).to(DEV)
    ref_bn.load_state_dict(bn.state_dict())
    x1 = torch.randn(4, 128, 8, 8, device=DEV, dtype=dtype) \
        .to(memory_format=torch.channels_last).requires_grad_(True)
    r1 = torch.randn(4, 128, 8, 8, device=DEV, dtype=dtype) \
        .to(memory_format=torch.channels_last).requires_grad_(True)
    x2 = x1.detach().float().contiguous().requires_grad_(True)
    r2 = r1.detach().float().contiguous().requires_grad_(True)

    y = bn_add_relu(x1, r1, bn)
    y_ref = F.relu(ref_bn(x2) + r2)
    assert torch.allclose(y.float().contiguous(), y_ref, **tol(dtype))
    g = torch.randn_like(y_ref)
    y.backward(g.to(dtype).to(memory_format=torch.channels_last))
    y_ref.backward(g)
    assert torch.allclose(x1.grad.float().contiguous(), x2.grad, **tol(dtype))
    assert torch.allclose(r1.grad.float().contiguous(), r2.grad, **tol(dtype))


def test_multi_tensor_sgd_channels_last():
    from mi355x_ddp.ops import _backend
    torch.manual_seed(5)
    p = torch.randn(16, 8, 3, 3, device=DEV).to(memory_format=torch.channels_last)
    g = torch.randn_like(p)  # preserves channels_last
    m = torch.zeros_like(p)
    ref = p.detach().clone()
    _backend.C().multi_tensor_sgd([p], [g], [m], 0.1, 0.9, 1e-4)
    d = g.add(ref, alpha=1e-4)
    assert torch.allclose(p, ref - 0.1 * d, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nc", [(16, 100), (256, 100), (64, 1000)])
def test_xent_kernel_vs_torch(dtype, nc):
    from mi355x_ddp.ops import softmax_cross_entropy
    N, C = nc
    torch.manual_seed(2)
    logits1 = torch.randn(N, C, device=DEV, dtype=dtype, requires_grad=True)
    logits2 = logits1.detach().float().requires_grad_(True)
    target = torch.randint(0, C, (N,), device=DEV)

    loss = softmax_cross_entropy(logits1, target)
    loss_ref = F.cross_entropy(logits2, target)
    assert torch.allclose(loss.float(), loss_ref, atol=1e-2, rtol=1e-3)
    loss.backward()
    loss_ref.backward()
    assert torch.allclose(logits1.grad.float(), logits2.grad, **tol(dtype))


def test_multi_tensor_sgd_vs_torch():
    from mi355x_ddp.ops import _backend
    torch.manual_seed(3)
    # 70 tensors of mixed sizes -> exercises multi-launch chunking (cap 32)
    sizes = [(3,), (64,), (64, 3, 3, 3), (512, 512, 3, 3), (100, 512), (1000000,)] * 12
    params = [torch.randn(*s, device=DEV) for s in sizes[:70]]
    grads = [torch.randn_like(p) for p in params]
    bufs = [torch.randn_like(p) for p in params]
    ref_p = [p.clone() for p in params]
    ref_m = [m.clone() for m in bufs]

    lr, mu, wd = 0.1, 0.9, 1e-4
    _backend.C().multi_tensor_sgd(params, grads, bufs, lr, mu, wd)
    for p, g, m in zip(ref_p, grads, ref_m):
        d = g.add(p, alpha=wd)
        m.mul_(mu).add_(d)
        p.add_(m, alpha=-lr)
    for p, rp in zip(params, ref_p):
        assert torch.allclose(p, rp, atol=1e-6)
    for m, rm in zip(bufs, ref_m):
        assert torch.allclose(m, rm, atol=1e-6)


def test_multi_tensor_unscale_detects_inf_and_nan():
    from mi355x_ddp.ops import _backend
    g1 = torch.full((1 << 18,), 4.0, device=DEV)
    g2 = torch.full((123,), 2.0, device=DEV)
    found = _backend.C().multi_tensor_unscale([g1, g2], 0.5)
    assert found.item() == 0
    assert torch.allclose(g1, torch.full_like(g1, 2.0))
    assert torch.allclose(g2, torch.full_like(g2, 1.0))

    g1[777] = float("inf")
    found = _backend.C().multi_tensor_unscale([g1, g2], 1.0)
    assert found.item() == 1
    g1[777] = 0.0
    g2[5] = float("nan")
    found = _backend.C().multi_tensor_unscale([g1, g2], 1.0)
    assert found.item() == 1

    # 40 tensors: two launches (32 per launch), sizes around the 8192-element
    # chunk. Powers of two times a power of two: every product is exact.
    sizes = [1, 3, 8191, 8192, 8193, 2 * 8192 + 5]
    vals = [2.0 ** (i % 7 - 3) for i in range(40)]
    gs = [torch.full((sizes[i % 6],), vals[i], device=DEV) for i in range(40)]
    found = _backend.C().multi_tensor_unscale(gs, 0.25)
    assert found.item() == 0
    for g, v in zip(gs, vals):
        assert torch.equal(g, torch.full_like(g, v * 0.25))
    assert gs[35].numel() == 2 * 8192 + 5   # in the second launch
    gs[35][-1] = float("inf")
    assert _backend.C().multi_tensor_unscale(gs, 1.0).item() == 1
    gs[35][-1] = 0.0
    assert gs[4].numel() == 8193            # element 8192: its second chunk
    gs[4][8192] = float("nan")
    assert _backend.C().multi_tensor_unscale(gs, 1.0).item() == 1


def test_fused_sgd_optimizer_gpu_matches_torch():
    from mi355x_ddp.ops import FusedSGD
    torch.manual_seed(4)
    m1 = nn.Sequential(nn.Conv2d(3, 8, 3), nn.Flatten(), nn.LazyLinear(10)).to(DEV)
    m1(torch.randn(2, 3, 8, 8, device=DEV))  # materialise lazy
    import copy
    m2 = copy.deepcopy(m1)
    o1 = FusedSGD(m1.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    o2 = torch.optim.SGD(m2.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    x = torch.randn(4, 3, 8, 8, device=DEV)
    for _ in range(3):
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad()
            m(x).pow(2).mean().backward()
            o.step()
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.allclose(p1, p2, atol=1e-5)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("clast", [False, True])
def test_bn_stats_packed_and_finalize(shape, clast):
    from mi355x_ddp.ops import _backend
    x = torch.randn(*shape, device=DEV, dtype=torch.bfloat16)
    if clast:
        x = x.to(memory_format=torch.channels_last)
    N, C, H, W = shape
    packed = _backend.C().bn_stats_packed(x)
    xf = x.float()
    ref_s = xf.sum(dim=(0, 2, 3))
    ref_sq = (xf * xf).sum(dim=(0, 2, 3))
    assert torch.allclose(packed[:C], ref_s, atol=2.0, rtol=1e-2)
    assert torch.allclose(packed[C:], ref_sq, atol=2.0, rtol=1e-2)

    cnt = float(N * H * W)
    rm = torch.zeros(C, device=DEV)
    rv = torch.ones(C, device=DEV)
    mean, invstd = _backend.C().bn_finalize(packed, cnt, 0.1, 1e-5, rm, rv)
    ref_mean = ref_s / cnt
    ref_var = (ref_sq / cnt - ref_mean * ref_mean).clamp_min(0)
    assert torch.allclose(mean, ref_mean, atol=1e-2, rtol=1e-2)
    assert torch.allclose(invstd, torch.rsqrt(ref_var + 1e-5), atol=1e-2, rtol=1e-2)
    unb = ref_var * cnt / (cnt - 1)
    assert torch.allclose(rm, 0.1 * ref_mean, atol=1e-3, rtol=1e-2)
    assert torch.allclose(rv, 0.9 + 0.1 * unb, atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("clast", [False, True])
def test_bn_bwd_reduce_packed(clast):
    from mi355x_ddp.ops import _backend
    N, C, H, W = 8, 128, 16, 16
    fmt = torch.channels_last if clast else torch.contiguous_format
    x = torch.randn(N, C, H, W, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=fmt)
    dy = torch.randn_like(x).contiguous(memory_format=fmt)
    y = torch.randn_like(x).contiguous(memory_format=fmt)
    mean = x.float().mean(dim=(0, 2, 3)).contiguous()
    invstd = torch.rand(C, device=DEV) + 0.5
    packed = _backend.C().bn_bwd_reduce_packed(dy, x, mean, invstd, y, True)
    g = dy.float() * (y.float() > 0)
    xhat = (x.float() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    assert torch.allclose(packed[:C], g.sum(dim=(0, 2, 3)), atol=1.0, rtol=2e-2)
    assert torch.allclose(packed[C:], (g * xhat).sum(dim=(0, 2, 3)), atol=1.0, rtol=2e-2)


@pytest.mark.parametrize("clast", [False, True])
def test_global_avgpool(clast):
    from mi355x_ddp.ops.pool import GlobalAvgPool2d
    x = torch.randn(8, 512, 4, 4, device=DEV, dtype=torch.bfloat16)
    if clast:
        x = x.to(memory_format=torch.channels_last)
    x.requires_grad_(True)
    y = GlobalAvgPool2d()(x)
    assert y.shape == (8, 512, 1, 1)
    ref = x.float().mean(dim=(2, 3), keepdim=True)
    assert torch.allclose(y.float(), ref, atol=1e-2, rtol=1e-2)
    dy = torch.randn_like(y)
    y.backward(dy)
    ref_dx = (dy.float() / 16).expand(8, 512, 4, 4)
    assert torch.allclose(x.grad.float(), ref_dx, atol=1e-2, rtol=1e-2)


def test_class_rank_accuracy():
    from mi355x_ddp.core.metrics import accuracy
    torch.manual_seed(3)
    logits = torch.randn(64, 100, device=DEV)
    target = torch.randint(0, 100, (64,), device=DEV)
    got1, got5 = accuracy(logits, target, (1, 5))
    # reference: topk pipeline on CPU
    maxk = 5
    _, pred = logits.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.view(1, -1))
    ref1 = correct[:1].float().sum() * 100.0 / 64
    ref5 = correct[:5].reshape(-1).float().sum() * 100.0 / 64
    assert torch.allclose(got1.cpu().reshape(()), ref1.cpu(), atol=1e-4)
    assert torch.allclose(got5.cpu().reshape(()), ref5.cpu(), atol=1e-4)


def test_conv_build_wT():
    from mi355x_ddp.ops import _backend
    w = torch.randn(64, 128, 3, 3, device=DEV, dtype=torch.bfloat16) \
        .to(memory_format=torch.channels_last)
    got = _backend.C().conv_build_wT(w)
    ref = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_maxpool_nhwc_parity(dtype):
    """Native NHWC max pool (fwd argmax + gather backward) vs ATen, including
    the overlapping-window 3x3 s2 case of the ImageNet stem."""
    torch.manual_seed(3)
    for (n, c, h, w, k, s, p) in [(4, 64, 112, 112, 3, 2, 1),
                                  (2, 64, 56, 56, 2, 2, 0),
                                  (3, 128, 17, 17, 3, 2, 1)]:
        x = torch.randn(n, c, h, w, device="cuda", dtype=dtype) \
            .to(memory_format=torch.channels_last).requires_grad_(True)
        xr = x.detach().clone().requires_grad_(True)
        from mi355x_ddp.ops.pool import MI355MaxPool2d
        pool = MI355MaxPool2d(k, s, p)
        y = pool(x)
        yr = torch.nn.functional.max_pool2d(xr, k, s, p)
        assert torch.equal(y, yr), (n, c, h, w, k, s, p)
        dy = torch.randn_like(y)
        y.backward(dy)
        yr.backward(dy)
        assert torch.allclose(x.grad.float(), xr.grad.float(),
                              atol=1e-2, rtol=1e-2), (n, c, h, w, k, s, p)


def test_maxpool_in_imagenet_model_step():
    """resnet50_imagenet forward+backward on the native NHWC path."""
    from mi355x_ddp.models import build_model
    from mi355x_ddp.ops import MI355Conv2d
    from mi355x_ddp.ops.pool import MI355MaxPool2d
    torch.manual_seed(0)
    m = build_model("resnet50_imagenet").cuda()
    m = MI355Conv2d.convert(m)
    m = MI355MaxPool2d.convert(m)
    m = m.to(memory_format=torch.channels_last)
    x = torch.randn(4, 3, 96, 96, device="cuda") \
        .to(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = m(x).float().logsumexp(dim=1).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
