"""xent_mix_fwd / xent_mix_bwd (two-label, label-smoothed cross entropy)
against float64, against the one-label kernels they must reproduce bit for
bit at lam = 1, eps = 0, and against themselves from run to run."""
import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops import _backend, softmax_cross_entropy

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 2), (5, 100), (256, 100), (300, 1000)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def tol(dtype):
    # tests/test_ops_gpu.py::test_xent_kernel_vs_torch's gradient tolerances
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else \
        dict(atol=5e-2, rtol=5e-2)


def _case(n, c, dtype, seed):
    """Random lam with rows forced to 0, 1 and 0.5, and a == b in some rows
    (with lam strictly inside (0, 1) in one of them)."""
    gen = torch.Generator().manual_seed(seed)
    x = (4 * torch.randn(n, c, generator=gen)).to(dtype)
    a = torch.randint(0, c, (n,), generator=gen)
    b = torch.randint(0, c, (n,), generator=gen)
    lam = torch.rand(n, generator=gen)
    forced = [0.0, 1.0, 0.5]
    for r in range(min(n, 3)):
        lam[r] = forced[r]
    if n >= 5:
        b[2], b[4] = a[2], a[4]
    if n >= 100:
        b[::7] = a[::7]
    return x, a, b, lam


def _reference(x, a, b, lam, eps):
    """float64 loss and d loss / d x of the same (rounded) logits."""
    x64 = x.double()
    l64 = lam.double()
    ce = lambda t: F.cross_entropy(x64, t, reduction="none",  # noqa: E731
                                   label_smoothing=eps)
    loss = (l64 * ce(a) + (1 - l64) * ce(b)).mean()
    n, c = x.shape
    hot = lambda t: F.one_hot(t, c).double()                   # noqa: E731
    dx = (torch.softmax(x64, dim=1)
          - (1 - eps) * (l64[:, None] * hot(a) + (1 - l64)[:, None] * hot(b))
          - eps / c) / n
    return loss, dx


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("nc", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_and_gradient_against_float64(nc, dtype, eps):
    """Loss: rtol 1e-5 is what test_xent_loss_is_the_same_bits_every_run
    derives for this reduction structure (fast exp/log to a few ulp, ten
    roundings in the sum). atol 1e-6 covers the added row sum: about ten
    roundings (6e-7 relative) of a sum of magnitude up to about 3.2*C, scaled
    by eps/C <= 0.1, i.e. about 2e-7."""
    x, a, b, lam = _case(*nc, dtype, seed=nc[0] + nc[1])
    want, want_dx = _reference(x, a, b, lam, eps)
    xg = x.to(DEV).requires_grad_(True)
    loss = softmax_cross_entropy(xg, a.to(DEV), b.to(DEV), lam.to(DEV), eps)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    print(f"loss {float(loss.detach()):.9g} want {float(want):.9g} "
          f"diff {float(loss.detach().double().cpu() - want):.3g}")
    torch.testing.assert_close(loss.double().cpu(), want, rtol=1e-5,
                               atol=1e-6)
    loss.backward()
    assert xg.grad.dtype == dtype
    got_dx = xg.grad.double().cpu()
    print(f"dx max abs diff {float((got_dx - want_dx).abs().max()):.3g}")
    assert torch.allclose(got_dx, want_dx, **tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("nc", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lam_one_eps_zero_is_the_one_label_kernels_bit_for_bit(nc, dtype):
    x, a, b, _ = _case(*nc, dtype, seed=7)
    x, a, b = x.to(DEV), a.to(DEV), b.to(DEV)
    ones = torch.ones(nc[0], device=DEV)
    dloss = torch.tensor(1.7, device=DEV)
    C = _backend.C()
    loss, lse = C.xent_fwd(x, a)
    dx = C.xent_bwd(x, a, lse, dloss)
    loss_m, lse_m = C.xent_mix_fwd(x, a, b, ones, 0.0)
    dx_m = C.xent_mix_bwd(x, a, b, ones, lse_m, dloss, 0.0)
    assert torch.equal(loss, loss_m)
    assert torch.equal(lse, lse_m)
    assert torch.equal(dx, dx_m)


@pytest.mark.parametrize("n", [5, 256, 300])
def test_loss_is_the_same_bits_every_run(n):
    x, a, b, lam = _case(n, 100, torch.bfloat16, seed=n)
    x, a, b, lam = x.to(DEV), a.to(DEV), b.to(DEV), lam.to(DEV)
    native = _backend.C().xent_mix_fwd
    losses = torch.stack([native(x, a, b, lam, 0.1)[0] for _ in range(6)])
    assert torch.equal(losses, losses[:1].expand(6))


def test_smoothing_alone_and_module_on_gpu():
    from mi355x_ddp.ops.xent import SoftmaxCrossEntropy
    x, a, b, lam = _case(64, 100, torch.bfloat16, seed=3)
    xg, ag = x.to(DEV), a.to(DEV)
    loss = SoftmaxCrossEntropy(0.1)(xg, ag)
    want = F.cross_entropy(x.double(), a, label_smoothing=0.1)
    torch.testing.assert_close(loss.double().cpu(), want, rtol=1e-5,
                               atol=1e-6)
    loss = SoftmaxCrossEntropy(0.1)(xg, (ag, b.to(DEV), lam.to(DEV)))
    want, _ = _reference(x, a, b, lam, 0.1)
    torch.testing.assert_close(loss.double().cpu(), want, rtol=1e-5,
                               atol=1e-6)


def test_kernel_rejects_bad_arguments():
    x, a, b, lam = _case(8, 10, torch.float32, seed=1)
    x, a, b, lam = x.to(DEV), a.to(DEV), b.to(DEV), lam.to(DEV)
    native = _backend.C().xent_mix_fwd
    with pytest.raises(RuntimeError, match="int64"):
        native(x, a.int(), b, lam, 0.0)
    with pytest.raises(RuntimeError, match="float32"):
        native(x, a, b, lam.double(), 0.0)
    with pytest.raises(RuntimeError, match=r"\[N\]"):
        native(x, a, b[:4], lam, 0.0)
    with pytest.raises(RuntimeError, match="device"):
        native(x, a, b, lam.cpu(), 0.0)
    with pytest.raises(RuntimeError, match="smoothing"):
        native(x, a, b, lam, 1.0)
