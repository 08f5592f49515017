"""Conv weight shadows on the GPU (MI355X): fp32 wgrad output, the SGD
kernel's bf16 shadow store and vector path, the batched rotate, and the
end-to-end guarantee that a shadowed model trains bit-for-bit like one that
casts and rotates per call.

Every comparison is torch.equal: the feature removes casts and launches, it
must not move a single bit.
"""
import functools

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.ops import _backend
from mi355x_ddp.ops.batchnorm import bn_relu
from mi355x_ddp.ops.conv import (MI355Conv2d, invalidate_weight_shadows,
                                 shadow_of)
from mi355x_ddp.ops.pool import GlobalAvgPool2d
from mi355x_ddp.ops.sgd import FusedSGD
from mi355x_ddp.ops.xent import softmax_cross_entropy

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last


# --------------------------------------------------------------------------
# fp32 dw from the wgrad epilogues
# --------------------------------------------------------------------------

# (N, C, H, W, K, R, stride, pad)
WGRAD_SHAPES = [
    (8, 64, 32, 32, 64, 3, 1, 1),
    (8, 256, 8, 8, 512, 3, 2, 1),
    (8, 64, 32, 32, 256, 1, 1, 0),
    (4, 24, 9, 9, 40, 3, 1, 1),
    (5, 3, 30, 30, 64, 3, 1, 1),
]
WTILES = [0, 1, 2, 3, 4, 5, 6]
SPLITS = [0, -1, 1, 7, 128]


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape):
    N, C, H, W, K, R, stride, pad = shape
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - R) // stride + 1
    g = torch.Generator().manual_seed(77 + sum(shape))
    x = torch.randn(N, C, H, W, generator=g).bfloat16()
    dy = torch.randn(N, K, P, Q, generator=g).bfloat16()
    return (x.to(DEV).contiguous(memory_format=CL),
            dy.to(DEV).contiguous(memory_format=CL))


@functools.lru_cache(maxsize=None)
def _wgrad_int_case(shape):
    """Integers in [-3, 3]: every product and partial sum is an integer below
    2^24, so an fp32 sum is exact in ANY order, while most results exceed 256
    and still have to be rounded to bf16."""
    N, C, H, W, K, R, stride, pad = shape
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - R) // stride + 1
    g = torch.Generator().manual_seed(78 + sum(shape))
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).bfloat16()
    dy = torch.randint(-3, 4, (N, K, P, Q), generator=g).bfloat16()
    return (x.to(DEV).contiguous(memory_format=CL),
            dy.to(DEV).contiguous(memory_format=CL))


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_fp32_equals_widened_bf16(shape):
    """Single-slice epilogues (splits 1), the atomic row-major reduce
    (wtile 4) and the <1,1>, <1,4> and grouped fragment reduces all store
    the bf16-rounded value, widened.

    Random bf16 data, except for wtile 4 with more than one possible slice:
    that tile sums its slices with fp32 atomics in an order that differs
    between launches, so two launches on random data can disagree in the
    last bf16 bit of some elements whatever the output type. There the data is
    integer-valued (exact sums in any order) and the comparison stays
    torch.equal; test_wgrad_fp32_atomic_tile_is_bf16_valued covers random
    data for that tile."""
    N, C, H, W, K, R, stride, pad = shape
    C_ = _backend.C()
    for wtile in WTILES:
        for splits in SPLITS:
            x, dy = _wgrad_int_case(shape) if (wtile == 4 and splits != 1) \
                else _wgrad_case(shape)
            d16 = C_.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, wtile)
            d32 = C_.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, wtile,
                                      True)
            assert d16.dtype == torch.bfloat16
            assert d32.dtype == torch.float32, (wtile, splits)
            assert d32.shape == (K, C, R, R)
            assert d32.is_contiguous(memory_format=CL)
            assert d32.stride() == d16.stride()
            assert torch.equal(d32, d16.float()), (wtile, splits)


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_fp32_atomic_tile_is_bf16_valued(shape):
    """wtile 4 sums with fp32 atomics, whose order varies between launches,
    so two launches need not agree bit for bit. What the fp32 output must
    still be is a bf16 value (round-trip exact), next to the bf16 launch's:
    the two fp32 sums differ by at most the worst-case reordering error
    n * max|x| * max|dy| * 2^-23 (n products per element), and rounding
    each to bf16 adds at most one bf16 spacing, 2^-7 relative."""
    N, C, H, W, K, R, stride, pad = shape
    x, dy = _wgrad_case(shape)
    n_red = N * dy.shape[2] * dy.shape[3]
    atol = n_red * float(x.abs().max()) * float(dy.abs().max()) * 2.0 ** -23
    C_ = _backend.C()
    for splits in SPLITS:
        d16 = C_.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, 4)
        d32 = C_.conv_wgrad_igemm(dy, x, R, R, stride, pad, splits, 4, True)
        assert d32.dtype == torch.float32
        assert d32.is_contiguous(memory_format=CL)
        assert torch.equal(d32, d32.bfloat16().float()), splits
        ref = d16.float()
        assert torch.all((d32 - ref).abs() <= ref.abs() * 2.0 ** -7 + atol), \
            splits


# --------------------------------------------------------------------------
# multi_tensor_sgd with bf16 shadow outputs
# --------------------------------------------------------------------------

def _sgd_tensors():
    """40 (p, g, m, w16) sets: crosses the 32-tensor batch, covers the chunk
    edge (8192 / 8193), a scalar tail (7, 100, 8193), conv layouts, and one
    view that starts one element into its buffer (4 bytes off 16-byte
    alignment -> scalar path) with an aligned twin holding the same data."""
    g = torch.Generator().manual_seed(5)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(DEV)

    shapes = [(7,), (100,), (8192,), (8193,)]
    shapes += [(3 * i + 5,) for i in range(31)]        # odd fillers
    shapes += [(20000,)]                               # several chunks
    sets = []
    for s in shapes:
        sets.append([rnd(*s), rnd(*s), rnd(*s)])
    sets.append([rnd(16, 8, 3, 3).contiguous(memory_format=CL)
                 for _ in range(3)])
    sets.append([rnd(32, 16, 1, 1).contiguous(memory_format=CL)
                 for _ in range(3)])
    n = 9001
    mis_src = [rnd(n) for _ in range(3)]
    mis = []
    for t in mis_src:
        buf = torch.zeros(n + 1, device=DEV)
        buf[1:].copy_(t)
        mis.append(buf[1:])
    assert mis[0].data_ptr() % 16 == 4
    sets.append(mis)                                   # index -2: misaligned
    sets.append([t.clone() for t in mis_src])          # index -1: its twin
    assert len(sets) == 40
    return sets


def _bf16_like(p, misaligned):
    if misaligned:
        return torch.zeros(p.numel() + 1, dtype=torch.bfloat16,
                           device=DEV)[1:]
    return torch.zeros_like(p, dtype=torch.bfloat16)


@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("mu", [0.0, 0.9])
def test_sgd_shadow_outputs(mu, wd):
    sets = _sgd_tensors()
    C_ = _backend.C()
    lr = 0.1

    def clone(t):   # keeps strides; a misaligned view becomes aligned
        return t.clone(memory_format=torch.preserve_format)

    # reference: cloned inputs, no shadow list (the six-argument call)
    rp = [clone(s[0]) for s in sets]
    rg = [clone(s[1]) for s in sets]
    rm = [clone(s[2]) for s in sets]
    C_.multi_tensor_sgd(rp, rg, rm if mu else [], lr, mu, wd)

    p = [s[0] for s in sets]
    gr = [s[1] for s in sets]
    m = [s[2] for s in sets]
    # every 6th tensor carries no shadow (null entry)
    w16 = [None if i % 6 == 1 else _bf16_like(t, i == len(p) - 2)
           for i, t in enumerate(p)]
    assert w16[-2] is not None and w16[-1] is not None
    m_before = [t.clone() for t in m]
    C_.multi_tensor_sgd(p, gr, m if mu else [], lr, mu, wd, w16)
    torch.cuda.synchronize()
    for i in range(len(p)):
        assert torch.equal(p[i], rp[i]), i
        if mu:
            assert torch.equal(m[i], rm[i]), i
        else:
            assert torch.equal(m[i], m_before[i]), i
        if w16[i] is not None:
            assert w16[i].stride() == p[i].stride()
            assert torch.equal(w16[i], p[i].to(torch.bfloat16)), i
    # misaligned (scalar path) == the same data aligned (vector path)
    assert torch.equal(p[-2], p[-1])
    assert torch.equal(m[-2], m[-1])
    assert torch.equal(w16[-2], w16[-1])


# --------------------------------------------------------------------------
# batched rotate and the one-launch cast + rotate
# --------------------------------------------------------------------------

ROT_SHAPES = [(64, 64, 3), (40, 24, 3), (64, 3, 3), (256, 64, 1), (8, 520, 1)]


def _filters(shapes, dtype):
    g = torch.Generator().manual_seed(11)
    return [torch.randn(K, C, R, R, generator=g).to(DEV).to(dtype)
            .contiguous(memory_format=CL) for K, C, R in shapes]


def test_batched_rotate_equals_build_wT():
    C_ = _backend.C()
    w16s = _filters(ROT_SHAPES, torch.bfloat16)
    wTs = [torch.zeros(C, R, R, K, dtype=torch.bfloat16, device=DEV)
           for K, C, R in ROT_SHAPES]
    C_.multi_tensor_build_wT(w16s, wTs)
    for w16, wT in zip(w16s, wTs):
        assert torch.equal(wT, C_.conv_build_wT(w16)), tuple(w16.shape)


def test_batched_rotate_crosses_the_32_tensor_batch():
    C_ = _backend.C()
    shapes = [(8 + i, 5 + 2 * i, 3 if i % 2 else 1) for i in range(35)]
    w16s = _filters(shapes, torch.bfloat16)
    wTs = [torch.zeros(C, R, R, K, dtype=torch.bfloat16, device=DEV)
           for K, C, R in shapes]
    C_.multi_tensor_build_wT(w16s, wTs)
    for w16, wT in zip(w16s, wTs):
        assert torch.equal(wT, C_.conv_build_wT(w16)), tuple(w16.shape)


def test_prep_weight_casts_and_rotates():
    C_ = _backend.C()
    for w32 in _filters(ROT_SHAPES, torch.float32):
        K, C, R, _ = w32.shape
        w16 = torch.zeros_like(w32, dtype=torch.bfloat16)
        wT = torch.zeros(C, R, R, K, dtype=torch.bfloat16, device=DEV)
        C_.conv_prep_weight(w32, w16, wT)
        ref16 = w32.to(torch.bfloat16)
        assert torch.equal(w16, ref16), tuple(w32.shape)
        assert torch.equal(wT, C_.conv_build_wT(ref16)), tuple(w32.shape)


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------

class _Net(nn.Module):
    """stem conv (C=3, no input grad) + a strided 64->64 conv (dgrad through
    wT) + BN + fc."""

    def __init__(self):
        super().__init__()
        self.conv1 = MI355Conv2d(3, 64, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = MI355Conv2d(64, 64, 3, stride=2, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(64)
        self.pool = GlobalAvgPool2d()
        self.fc = nn.Linear(64, 10)

    def forward(self, x):
        out = bn_relu(self.conv1(x), self.bn1)
        out = bn_relu(self.conv2(out), self.bn2)
        return self.fc(torch.flatten(self.pool(out), 1))


def _build(seed=3):
    torch.manual_seed(seed)
    net = _Net().to(DEV).to(memory_format=CL)
    opt = FusedSGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    return net, opt


def _batch(i):
    g = torch.Generator().manual_seed(100 + i)
    x = torch.randn(8, 3, 16, 16, generator=g).to(DEV) \
        .contiguous(memory_format=CL)
    y = torch.randint(0, 10, (8,), generator=g).to(DEV)
    return x, y


def _fwd_bwd(net, i, scale=1.0):
    x, y = _batch(i)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = softmax_cross_entropy(net(x), y) * scale
    loss.backward()
    return loss.detach()


def _train_step(net, opt, i):
    opt.zero_grad(set_to_none=True)
    loss = _fwd_bwd(net, i)
    grads = [p.grad.clone() for p in net.parameters()]
    opt.step()
    return loss, grads


def _state(net):
    return [p.detach().clone() for p in net.parameters()] + \
           [b.detach().clone() for b in net.buffers()]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.stride() == v.stride(), (what, i)
        assert torch.equal(u, v), (what, i)


@pytest.fixture
def no_autotune(monkeypatch):
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    return monkeypatch


def test_three_steps_bit_equal_to_shadows_off(no_autotune):
    mp = no_autotune
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    on, opt_on = _build()
    mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
    off, opt_off = _build()
    for i in range(3):
        mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
        loss_on, g_on = _train_step(on, opt_on, i)
        mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
        loss_off, g_off = _train_step(off, opt_off, i)
        # the loss value itself is summed with atomics over the rows and is
        # not bit-stable run to run; its gradient is
        assert torch.allclose(loss_on, loss_off, rtol=1e-6), i
        _assert_same(g_on, g_off, f"grad step {i}")
        _assert_same(_state(on), _state(off), f"state step {i}")
    for conv in (on.conv1, on.conv2):
        sh = shadow_of(conv.weight)
        # created and filled once, at the first forward; every later update
        # came from the SGD step
        assert sh is not None and sh.refreshes == 1
        assert sh.fresh(conv.weight)
    for conv in (off.conv1, off.conv2):
        assert shadow_of(conv.weight) is None


def test_grad_accumulation_and_eval_with_shadow_check(no_autotune):
    mp = no_autotune
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    mp.setenv("MI355X_CHECK_SHADOWS", "1")
    on, opt_on = _build()
    mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
    off, opt_off = _build()
    for step in range(3):
        outs = []
        for net, opt, flag in ((on, opt_on, "1"), (off, opt_off, "0")):
            mp.setenv("MI355X_WEIGHT_SHADOWS", flag)
            opt.zero_grad(set_to_none=True)
            _fwd_bwd(net, 2 * step, 0.5)
            net.eval()
            with torch.no_grad(), torch.autocast("cuda",
                                                 dtype=torch.bfloat16):
                ev = net(_batch(50 + step)[0])
            net.train()
            _fwd_bwd(net, 2 * step + 1, 0.5)
            grads = [p.grad.clone() for p in net.parameters()]
            opt.step()
            outs.append((ev, grads, _state(net)))
        assert torch.equal(outs[0][0], outs[1][0]), step
        _assert_same(outs[0][1], outs[1][1], f"grad step {step}")
        _assert_same(outs[0][2], outs[1][2], f"state step {step}")
    assert shadow_of(on.conv2.weight).refreshes == 1


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA]


def test_steady_state_launches(no_autotune):
    """A steady-state step with shadows holds no per-conv cast or rotate
    kernel: only the image and the fc layer are still cast."""
    mp = no_autotune
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    on, opt_on = _build()
    for i in range(2):
        _train_step(on, opt_on, i)
    names = _kernel_names(lambda: _train_step(on, opt_on, 2))
    assert names, "profiler recorded no GPU kernels"

    def count(sub):
        return sum(sub in n for n in names)

    assert count("multi_tensor_sgd_kernel") >= 1, names
    assert count("build_wT_kernel") - count("multi_build_wT_kernel") == 0, names
    assert count("multi_build_wT_kernel") == 1, names
    # float -> bf16: image, fc weight, fc bias
    f2b = sum("bfloat16_copy_kernel_cuda" in n for n in names)
    # bf16 -> float: the fc weight and bias gradients
    b2f = sum("bfloat16tofloat32_copy_kernel_cuda" in n for n in names)
    assert f2b <= 3, names
    assert b2f <= 2, names

    # and the same step without shadows does launch them: 2 casts each way
    # (two convs) and one rotate (conv2; the stem has no input gradient)
    mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
    off, opt_off = _build()
    for i in range(2):
        _train_step(off, opt_off, i)
    names_off = _kernel_names(lambda: _train_step(off, opt_off, 2))
    assert sum("build_wT_kernel" in n for n in names_off) == 1, names_off
    assert sum("bfloat16_copy_kernel_cuda" in n for n in names_off) == f2b + 2
    assert sum("bfloat16tofloat32_copy_kernel_cuda" in n
               for n in names_off) == b2f + 2


@pytest.mark.parametrize("how", ["inplace", "load_state_dict", "data_assign"])
def test_staleness(no_autotune, how):
    """Every way of changing a weight other than the optimizer step is seen
    by the next forward."""
    mp = no_autotune
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    on, opt_on = _build()
    mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
    off, opt_off = _build()
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    _train_step(on, opt_on, 0)
    mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
    _train_step(off, opt_off, 0)

    other = _build(seed=9)[0]
    for net in (on, off):
        if how == "inplace":
            with torch.no_grad():
                net.conv1.weight.mul_(0.5)
                net.conv2.weight.mul_(0.5)
        elif how == "load_state_dict":
            net.load_state_dict(other.state_dict())
        else:
            net.conv1.weight.data = other.conv1.weight.detach().clone(
                memory_format=torch.preserve_format)
            net.conv2.weight.data = other.conv2.weight.detach().clone(
                memory_format=torch.preserve_format)

    x = _batch(7)[0]
    outs = []
    for net, flag in ((on, "1"), (off, "0")):
        mp.setenv("MI355X_WEIGHT_SHADOWS", flag)
        net.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            outs.append(net(x))
    assert torch.equal(outs[0], outs[1])
    assert shadow_of(on.conv1.weight).refreshes == 2
    # and a training step from there still agrees (dgrad reads the new wT)
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    on.train()
    _, g_on = _train_step(on, opt_on, 1)
    mp.setenv("MI355X_WEIGHT_SHADOWS", "0")
    off.train()
    _, g_off = _train_step(off, opt_off, 1)
    _assert_same(g_on, g_off, "grad after external write")
    _assert_same(_state(on), _state(off), "state after external write")


def test_unseen_write_needs_invalidate(no_autotune):
    """p.data.<op>_() bypasses the version counter; invalidate_weight_shadows
    is the documented remedy."""
    mp = no_autotune
    mp.setenv("MI355X_WEIGHT_SHADOWS", "1")
    on, opt_on = _build()
    _train_step(on, opt_on, 0)
    on.conv2.weight.data.mul_(0.25)
    invalidate_weight_shadows(on)
    mp.setenv("MI355X_CHECK_SHADOWS", "1")   # raises if a shadow is stale
    _train_step(on, opt_on, 1)
    assert shadow_of(on.conv2.weight).refreshes == 2
