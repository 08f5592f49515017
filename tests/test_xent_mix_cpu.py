"""Two-label, label-smoothed cross entropy: the torch path of
ops.softmax_cross_entropy against a float64 reference built from
F.cross_entropy(label_smoothing=eps)."""
import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.ops import softmax_cross_entropy
from mi355x_ddp.ops.xent import SoftmaxCrossEntropy


def _reference(x64, a, b, lam, eps):
    ce = lambda t: F.cross_entropy(x64, t, reduction="none",  # noqa: E731
                                   label_smoothing=eps)
    l64 = lam.double()
    return (l64 * ce(a) + (1 - l64) * ce(b)).mean()


def _case(n, c, seed):
    gen = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(n, c, generator=gen)
    a = torch.randint(0, c, (n,), generator=gen)
    b = torch.randint(0, c, (n,), generator=gen)
    lam = torch.rand(n, generator=gen)
    lam[0] = 0.0
    if n > 2:
        lam[1], lam[2] = 1.0, 0.5
        b[2] = a[2]                       # a == b: both one-hots add
    return x, a, b, lam


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("nc", [(1, 2), (5, 100), (33, 10)])
def test_loss_and_gradient_match_float64_reference(nc, eps):
    x, a, b, lam = _case(*nc, seed=11)
    x32 = x.clone().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    loss = softmax_cross_entropy(x32, a, b, lam, label_smoothing=eps)
    want = _reference(x64, a, b, lam, eps)
    # fp32 evaluation of an O(10) quantity: a few ulp of 1e-6 relative
    torch.testing.assert_close(loss.double(), want, rtol=1e-5, atol=1e-6)
    (2.0 * loss).backward()
    (2.0 * want).backward()
    torch.testing.assert_close(x32.grad.double(), x64.grad, rtol=1e-4,
                               atol=1e-6)


def test_smoothing_alone_matches_torch():
    x, a, _, _ = _case(7, 20, seed=3)
    loss = softmax_cross_entropy(x, a, label_smoothing=0.1)
    want = F.cross_entropy(x.double(), a, label_smoothing=0.1)
    torch.testing.assert_close(loss.double(), want, rtol=1e-5, atol=1e-6)


def test_lam_one_eps_zero_is_the_plain_loss_exactly():
    x, a, b, _ = _case(9, 100, seed=5)
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    plain = softmax_cross_entropy(x1, a)
    mixed = softmax_cross_entropy(x2, a, b, torch.ones(9), 0.0)
    assert torch.equal(plain, mixed)
    plain.backward()
    mixed.backward()
    assert torch.equal(x1.grad, x2.grad)


def test_module_takes_tensor_or_tuple_target():
    x, a, b, lam = _case(6, 10, seed=8)
    crit = SoftmaxCrossEntropy(label_smoothing=0.1)
    assert torch.equal(crit(x, (a, b, lam)),
                       softmax_cross_entropy(x, a, b, lam, 0.1))
    assert torch.equal(crit(x, a),
                       softmax_cross_entropy(x, a, label_smoothing=0.1))
    assert torch.equal(SoftmaxCrossEntropy()(x, a),
                       softmax_cross_entropy(x, a))


def test_bad_arguments_raise():
    x, a, b, lam = _case(4, 10, seed=1)
    with pytest.raises(ValueError, match="label_smoothing"):
        softmax_cross_entropy(x, a, label_smoothing=1.0)
    with pytest.raises(ValueError, match="label_smoothing"):
        SoftmaxCrossEntropy(label_smoothing=-0.1)
    with pytest.raises(ValueError, match="together"):
        softmax_cross_entropy(x, a, target_b=b)
    with pytest.raises(ValueError, match="float32"):
        softmax_cross_entropy(x, a, b, lam.double())
