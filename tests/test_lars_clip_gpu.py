"""LARS and gradient-norm clipping on the GPU (MI355X): the multi-tensor norm
kernels, the coefficient kernel, the scaled update kernels, FusedSGD end to
end against a float64 reference, the hipGraph-captured step, and the unchanged
default step.

Inputs are N(0, 0.1^2), so fp32 rounding of an update (a few operations on
values below 1) stays far under the absolute tolerances used here. LARS runs
with eta = 1, which makes the trust ratios O(1): with 1e-3 a wrong ratio would
hide under the tolerance.
"""
import functools
import math

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.ops import _backend
from mi355x_ddp.ops.conv import _shadow_for
from mi355x_ddp.ops.sgd import FusedSGD

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
CHUNK = 8192
# one, a few, under a chunk, around one chunk, over two, 37 chunks (the fold)
SIZES = [1, 3, 255, 8191, 8192, 8193, 2 * 8192 + 5, 300_000]
REPS = 7          # 7 x 10 = 70 tensors: crosses the 32-per-launch cap twice
LR, MU, WD = 0.1, 0.9, 1e-2


def _rnd(gen, *shape):
    return (torch.randn(*shape, generator=gen) * 0.1).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs():
    """(ws fp32, gs fp32, gs bf16), 70 tensors each. Shared and read-only:
    every test that writes works on clones."""
    gen = torch.Generator().manual_seed(1234)
    ws, gs = [], []
    for _ in range(REPS):
        for s in SIZES:
            ws.append(_rnd(gen, s))
            gs.append(_rnd(gen, s))
        ws.append(_rnd(gen, 64, 3, 3, 3).contiguous(memory_format=CL))
        gs.append(_rnd(gen, 64, 3, 3, 3).contiguous(memory_format=CL))
        # views one element into a buffer: pointers not 16-byte aligned
        ws.append(_rnd(gen, CHUNK + 78)[1:])
        gs.append(_rnd(gen, CHUNK + 78)[1:])
    gs16 = [_offset_like(g, g.bfloat16()) for g in gs]
    assert ws[-1].data_ptr() % 16 != 0 and gs16[-1].data_ptr() % 16 != 0
    return ws, gs, gs16


def _offset_like(src, val):
    """`val` with src's alignment: an unaligned src gets an unaligned copy."""
    if src.data_ptr() % 16 == 0:
        return val
    buf = torch.empty(val.numel() + 1, dtype=val.dtype, device=val.device)
    buf[1:].copy_(val)
    return buf[1:]


def _clone(ts):
    """Clones that keep strides and (mis)alignment."""
    return [_offset_like(t, t.clone()) for t in ts]


def _nchunks(ts):
    return sum((t.numel() + CHUNK - 1) // CHUNK for t in ts)


def _sqnorm(ws, gs):
    partials = torch.empty(2, _nchunks(ws), device=DEV)
    sq = torch.empty(2, len(ws), device=DEV)
    _backend.C().multi_tensor_sqnorm(ws, gs, partials, sq)
    return sq


def _sq64(ts):
    return torch.stack([t.double().pow(2).sum() for t in ts])


def test_constants_agree_with_extension():
    """ops/sgd.py keeps its own values for the CPU fallback."""
    from mi355x_ddp.ops import sgd
    C = _backend.C()
    assert C.MT_CHUNK == sgd._MT_CHUNK == CHUNK
    # the kernels hold these as float, and torch rounds the Python values to
    # float where it adds them to fp32 tensors: equal as float
    for name in ("LARS_EPS", "CLIP_EPS"):
        mine = torch.tensor(getattr(sgd, name), dtype=torch.float32).item()
        assert getattr(C, name) == mine, name


# ---- 1. sums of squares -------------------------------------------------------

@pytest.mark.parametrize("gdtype", ["fp32", "bf16"])
def test_sqnorm_vs_float64(gdtype):
    # All terms are >= 0, so a fixed-order fp32 sum whose longest chain is L
    # additions has relative error <= (L + 1) * 2^-24. The kernels' L: 32 in
    # a thread (8192/256 elements), 6 + 6 in the block reduction, then
    # ceil(nchunks/256) = 1 in a fold thread and 6 + 6 again: L = 57,
    # (L + 1) * 2^-24 = 3.5e-6 <= 1e-5.
    ws, gs, gs16 = _inputs()
    g = gs if gdtype == "fp32" else gs16
    sq = _sqnorm(ws, g)
    want = torch.stack([_sq64(ws), _sq64(g)])
    rel = ((sq.double() - want).abs() / want).max()
    assert rel <= 1e-5, float(rel)
    assert torch.equal(_sqnorm(ws, g), sq)


def test_sqnorm_mixed_grad_dtypes_in_one_list():
    """fp32 and bf16 gradients in one list (a model with both kinds of
    parameters): launches are cut at the dtype changes."""
    ws, gs, gs16 = _inputs()
    mixed = [g if (i // 7) % 2 == 0 else h
             for i, (g, h) in enumerate(zip(gs, gs16))]
    sq = _sqnorm(ws, mixed)
    want = torch.stack([_sq64(ws), _sq64(mixed)])
    assert ((sq.double() - want).abs() / want).max() <= 1e-5


# ---- 2. coefficients ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sq_with_zeros():
    """The kernel's own sq for the shared list with one all-zero gradient
    (tensor 3) and one all-zero weight (tensor 4)."""
    ws, gs, _ = _inputs()
    ws, gs = list(ws), list(gs)
    gs[3] = torch.zeros_like(gs[3])
    ws[4] = torch.zeros_like(ws[4])
    sq = _sqnorm(ws, gs)
    assert sq[1, 3] == 0 and sq[0, 4] == 0
    return sq


@pytest.mark.parametrize("max_norm", [0.0, 1.0, 1e4])   # off, clips, does not
@pytest.mark.parametrize("lars", [False, True])
def test_coeffs_vs_float64(max_norm, lars):
    eta = 1.0
    sq = _sq_with_zeros()
    n = sq.shape[1]
    flags = [i % 3 == 2 for i in range(n)]
    excluded = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    gscale = torch.full((1,), -1.0, device=DEV)
    ratio = torch.full((n,), -1.0, device=DEV)
    gnorm = torch.full((), -1.0, device=DEV)
    _backend.C().sgd_coeffs(sq, excluded, gscale, ratio, gnorm, max_norm,
                            lars, eta, WD)
    sq64 = sq.double().cpu()
    norm = math.sqrt(float(sq64[1].sum()))
    c = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    assert (c < 1.0) == (max_norm == 1.0)
    want = []
    for t in range(n):
        wn, gn = math.sqrt(float(sq64[0, t])), math.sqrt(float(sq64[1, t]))
        if lars and not flags[t] and wn > 0 and gn > 0:
            want.append(eta * wn / (c * gn + WD * wn + 1e-8))
        else:
            want.append(1.0)
    assert want[3] == 1.0 and want[4] == 1.0 and want[2] == 1.0
    if lars:
        assert want[0] != 1.0
    # about six fp32 operations at a few ulp each
    assert abs(float(gnorm) - norm) <= 1e-5 * norm
    assert abs(float(gscale) - c) <= 1e-5 * c
    want = torch.tensor(want, dtype=torch.float64)
    assert torch.allclose(ratio.double().cpu(), want, rtol=1e-5, atol=0)
    if max_norm in (0.0, 1e4):
        assert float(gscale) == 1.0
    ones = [t for t in range(n) if want[t] == 1.0]
    assert torch.equal(ratio[ones], torch.ones(len(ones), device=DEV))


def test_coeffs_range_writes_only_its_ratios():
    sq = _sq_with_zeros()
    n = sq.shape[1]
    excluded = torch.zeros(n, dtype=torch.uint8, device=DEV)
    gscale = torch.zeros(1, device=DEV)
    gnorm = torch.zeros((), device=DEV)
    full = torch.full((n,), -1.0, device=DEV)
    part = torch.full((n,), -1.0, device=DEV)
    C = _backend.C()
    C.sgd_coeffs(sq, excluded, gscale, full, gnorm, 1.0, True, 1.0, WD)
    C.sgd_coeffs(sq, excluded, gscale, part, gnorm, 1.0, True, 1.0, WD, 10, 45)
    assert torch.equal(part[10:45], full[10:45])
    assert (part[:10] == -1).all() and (part[45:] == -1).all()


# ---- 3. scaled update kernels -------------------------------------------------

def _ref_update64(w, g, m, r, c, mu):
    d = r * (c * g.double() + WD * w.double())
    m_new = mu * m.double() + d if m is not None else d
    return w.double() - LR * m_new, m_new


@pytest.mark.parametrize("mu", [MU, 0.0])
def test_scaled_update_fp32(mu):
    ws0, gs0, _ = _inputs()
    n = len(ws0)
    gen = torch.Generator().manual_seed(5)
    ms0 = [_offset_like(w, _rnd(gen, *w.shape).contiguous(
        memory_format=CL if w.dim() == 4 else torch.contiguous_format))
        for w in ws0] if mu else None
    ws, gs = _clone(ws0), _clone(gs0)
    ms = _clone(ms0) if mu else []
    w16s = [None if i % 3 == 0 else torch.empty_like(
        w, dtype=torch.bfloat16 if i % 3 == 1 else torch.float16)
        for i, w in enumerate(ws)]
    c = 0.5
    ratio = torch.linspace(0.25, 2.0, n, device=DEV)
    gscale = torch.tensor([c], device=DEV)
    _backend.C().multi_tensor_sgd_scaled(ws, gs, ms, LR, mu, WD, gscale,
                                         ratio, w16s)
    for i in range(n):
        w_ref, m_ref = _ref_update64(ws0[i], gs0[i], ms0[i] if mu else None,
                                     float(ratio[i]), c, mu)
        assert torch.allclose(ws[i].double(), w_ref, atol=1e-6, rtol=0), i
        if mu:
            assert torch.allclose(ms[i].double(), m_ref, atol=1e-6, rtol=0), i
        assert torch.equal(gs[i], gs0[i]), i   # gradients are not modified
        if w16s[i] is not None:
            assert torch.equal(w16s[i], ws[i].to(w16s[i].dtype)), i


def test_scaled_update_o2():
    ws0, _, gs16 = _inputs()
    n = len(ws0)
    gen = torch.Generator().manual_seed(6)
    ms0 = [_rnd(gen, *w.shape).contiguous(
        memory_format=CL if w.dim() == 4 else torch.contiguous_format)
        for w in ws0]
    masters, gs, ms = _clone(ws0), _clone(gs16), _clone(ms0)
    ps = [torch.empty_like(w, dtype=torch.bfloat16) for w in masters]
    c = 0.5
    ratio = torch.linspace(0.25, 2.0, n, device=DEV)
    gscale = torch.tensor([c], device=DEV)
    _backend.C().multi_tensor_sgd_o2_scaled(ps, gs, masters, ms, LR, MU, WD,
                                            gscale, ratio)
    for i in range(n):
        w_ref, m_ref = _ref_update64(ws0[i], gs16[i], ms0[i],
                                     float(ratio[i]), c, MU)
        assert torch.allclose(masters[i].double(), w_ref, atol=1e-6,
                              rtol=0), i
        assert torch.allclose(ms[i].double(), m_ref, atol=1e-6, rtol=0), i
        assert torch.equal(ps[i], masters[i].bfloat16()), i
        # ... and within atol of the reference once that is rounded alike
        assert torch.allclose(ps[i].double(), w_ref, atol=1e-6, rtol=2 ** -8)
        assert torch.equal(gs[i], gs16[i]), i


@pytest.mark.parametrize("mu", [MU, 0.0])
def test_scaled_update_vector_and_scalar_paths_agree(mu):
    gen = torch.Generator().manual_seed(7)
    size = 2 * CHUNK + 5
    w, g, m = (_rnd(gen, size) for _ in range(3))

    def unaligned(t):
        buf = torch.empty(size + 1, device=DEV)
        buf[1:].copy_(t)
        return buf[1:]

    ws = [w.clone(), unaligned(w)]
    gs = [g.clone(), unaligned(g)]
    ms = [m.clone(), unaligned(m)] if mu else []
    w16s = [torch.empty(size, dtype=torch.bfloat16, device=DEV)
            for _ in range(2)]
    assert ws[0].data_ptr() % 16 == 0 and ws[1].data_ptr() % 16 != 0
    ratio = torch.tensor([1.3, 1.3], device=DEV)
    # no power of two: gscale*g rounds, so a path that fuses it into an FMA
    # and one that does not give different bits
    gscale = torch.tensor([0.3], device=DEV)
    _backend.C().multi_tensor_sgd_scaled(ws, gs, ms, LR, mu, WD, gscale,
                                         ratio, w16s)
    assert not torch.equal(ws[0], w)
    assert torch.equal(ws[0], ws[1])
    assert torch.equal(w16s[0], w16s[1])
    if mu:
        assert torch.equal(ms[0], ms[1])


# ---- 4. end to end ------------------------------------------------------------

# 1-D tensors are excluded from LARS; the 2-D and 4-D ones are adapted
E2E_SHAPES = [(1,), (3,), (255,), (8191,), (64, 128), (8193,), (3, 5463),
              (300, 1000), (64, 3, 3, 3), (2, 4135)]
E2E_REPS = 4      # 40 tensors: more than one launch


def _e2e_tensors(gen, unaligned_last):
    out = []
    for _ in range(E2E_REPS):
        for shape in E2E_SHAPES:
            if len(shape) == 4:
                t = _rnd(gen, *shape).contiguous(memory_format=CL)
            elif unaligned_last and shape == E2E_SHAPES[-1]:
                # like a FlatDDP gradient view at an odd offset
                t = _rnd(gen, shape[0] * shape[1] + 1)[1:].view(shape)
            else:
                t = _rnd(gen, *shape)
            out.append(t)
    return out


@pytest.mark.parametrize("shadows", [False, True])
def test_fused_sgd_lars_clip_vs_float64(shadows):
    eta, max_norm = 1.0, 10.0
    gen = torch.Generator().manual_seed(8)
    ps = [nn.Parameter(t) for t in _e2e_tensors(gen, False)]
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, lars=True,
                   lars_eta=eta, clip_grad_norm=max_norm)
    shs = {}
    if shadows:
        four_d = [i for i, p in enumerate(ps) if p.dim() == 4]
        for k, i in enumerate(four_d):
            shs[i] = _shadow_for(
                ps[i], torch.bfloat16 if k % 2 == 0 else torch.float16)
    ws = [p.detach().double().clone() for p in ps]
    ms = [torch.zeros_like(w) for w in ws]
    for step in range(2):
        grads = _e2e_tensors(gen, True)
        assert grads[len(E2E_SHAPES) - 1].data_ptr() % 16 != 0
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
        g64 = [g.double() for g in grads]
        norm = math.sqrt(sum(float(g.pow(2).sum()) for g in g64))
        c = min(1.0, max_norm / (norm + 1e-6))
        assert c < 1.0
        assert abs(float(opt.grad_norm()) - norm) <= 1e-5 * norm
        for i, (p, w, g, m) in enumerate(zip(ps, ws, g64, ms)):
            wn, gn = float(w.norm()), float(g.norm())
            r = 1.0
            if w.dim() > 1:
                r = eta * wn / (c * gn + WD * wn + 1e-8)
                assert abs(r - 1.0) > 0.1
            d = r * (c * g + WD * w)
            m.mul_(MU).add_(d)
            w.sub_(LR * m)
            # 2e-5: 1e-5 on each of the two norms under the ratio
            tol = 2e-5 * float(d.abs().max()) + 1e-6
            buf = opt.state[p]["momentum_buffer"].double()
            err_m = float((buf - m).abs().max())
            err_p = float((p.detach().double() - w).abs().max())
            assert err_m <= tol, (step, i, err_m, tol)
            assert err_p <= LR * tol + 1e-6, (step, i, err_p)
        for i, sh in shs.items():
            assert sh.fresh(ps[i]), (step, i)
            sh.check(ps[i])   # w16 == rounded weight, wT == its rotation
            assert torch.equal(sh.w16, ps[i].detach().to(sh.dtype))


# ---- 5. hipGraph --------------------------------------------------------------

def _make_net():
    torch.manual_seed(11)
    # ReLU-free, like the exact graph test of test_train_gpu.py: borderline
    # ReLU mask flips would make eager and replay drift legitimately
    return nn.Sequential(
        nn.Conv2d(3, 16, 3, padding=1), nn.BatchNorm2d(16), nn.Tanh(),
        nn.Conv2d(16, 32, 3, stride=2, padding=1),
        nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(), nn.Linear(32, 10))


def test_hip_graph_step_with_lars_and_clip_matches_eager():
    from mi355x_ddp.config import TrainConfig
    from mi355x_ddp.core.graphs import GraphedTrainStep
    from mi355x_ddp.core.worker import init_seeds
    from mi355x_ddp.parallel import FlatDDP

    init_seeds(0, deterministic=True)
    gen = torch.Generator().manual_seed(3)
    data = [(torch.randn(16, 3, 16, 16, generator=gen).pin_memory(),
             torch.randint(0, 10, (16,), generator=gen).pin_memory())
            for _ in range(4)]
    device = torch.device("cuda", 0)
    crit = nn.CrossEntropyLoss()
    etas = [0.1, 0.1, 0.3, 0.3]   # changes between replays 2 and 3

    def make_opt(model):
        return FusedSGD(model.parameters(), lr=0.05, momentum=0.9,
                        weight_decay=1e-4, lars=True, lars_eta=etas[0],
                        clip_grad_norm=0.5)

    def eager(etas):
        model = FlatDDP(_make_net().to(device), overlap=True)
        opt = make_opt(model)
        model.train()
        for (img, lbl), eta in zip(data, etas):
            opt.param_groups[0]["lars_eta"] = eta
            model.zero_grad_buffer()
            crit(model(img.to(device)), lbl.to(device)).backward()
            model.finalize_backward()
            opt.step()
        return [p.detach().clone() for p in model.parameters()]

    def graphed():
        cfg = TrainConfig(batch_size=16, amp="fp32", sync_bn=False,
                          hip_graph=True)
        model = FlatDDP(_make_net().to(device), overlap=False,
                        static_grads=True)
        opt = make_opt(model)
        model.train()
        snap = [p.detach().clone() for p in model.parameters()]
        bufs = [b.detach().clone() for b in model.buffers()]
        # the capture succeeding shows that the step has no host sync
        step = GraphedTrainStep(model, crit, opt, cfg, device, batch=16,
                                image_size=16, num_classes=10)
        with torch.no_grad():
            for p, s in zip(model.parameters(), snap):
                p.copy_(s)
            for b, s in zip(model.buffers(), bufs):
                b.copy_(s)
            for st in opt.state.values():
                st["momentum_buffer"].zero_()
        graphs = []
        for (img, lbl), eta in zip(data, etas):
            opt.param_groups[0]["lars_eta"] = eta
            step.run(img, lbl)
            graphs.append(step.graph)
        torch.cuda.synchronize()
        assert graphs[0] is graphs[1] and graphs[2] is graphs[3]
        assert graphs[1] is not graphs[2], "lars_eta change did not re-capture"
        assert float(opt.grad_norm()) > 0
        return [p.detach().clone() for p in model.parameters()]

    pe, pg = eager(etas), graphed()
    for a, b in zip(pe, pg):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-5), (a - b).abs().max()
    # the new eta took effect: the same run without the change ends elsewhere
    same = eager([etas[0]] * 4)
    assert any(not torch.allclose(a, b, atol=1e-4, rtol=0)
               for a, b in zip(same, pg))


# ---- 6. defaults --------------------------------------------------------------

def test_default_step_equals_direct_kernel_call():
    ws0, gs0, _ = _inputs()
    ps = [nn.Parameter(t) for t in _clone(ws0)]
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD)
    ws, ms = _clone(ws0), [torch.zeros_like(w) for w in ws0]
    for step in range(2):
        for p, g in zip(ps, gs0):
            p.grad = g
        opt.step()
        _backend.C().multi_tensor_sgd(ws, list(gs0), ms, LR, MU, WD)
        for p, w, m in zip(ps, ws, ms):
            assert torch.equal(p.detach(), w)
            assert torch.equal(opt.state[p]["momentum_buffer"], m)
    assert opt.grad_norm() is None
