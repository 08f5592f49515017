"""Weight EMA on the GPU (MI355X): the EMA instantiations of the multi-tensor
SGD kernels and `multi_tensor_ema` against float64, vector against scalar
path, FusedSGD and WeightEMA end to end on ResNet-18 under weight shadows, the
hipGraph-captured step, and a skipped fp16 step.

The tensor set is the smallest that reaches every branch: under a chunk
(1, 3, 255), a chunk edge from both sides (8191, 8192, 8193), several chunks
with a tail of size % 4 (2*8192 + 5), a channels_last 4-D weight, a view one
element into its buffer (the scalar path), and 4 x 9 = 36 tensors, which is
past the 32 of one launch.

Inputs are N(0, 0.1^2). One average step is at most three fp32 roundings of
values below 1 (about 9e-8 together) and d < 1 contracts earlier error, so
atol 1e-6 holds with room. d = 0.5, not 0.999: at 0.999 a missing update would
hide under any tolerance.
"""
import functools

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.ops import _backend
from mi355x_ddp.ops.conv import shadow_of
from mi355x_ddp.ops.sgd import FusedSGD, multi_tensor_ema

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
CHUNK = 8192
SIZES = [1, 3, 255, 8191, 8192, 8193, 2 * 8192 + 5]
REPS = 4
LR, MU, WD, D = 0.1, 0.9, 1e-2, 0.5


def _rnd(gen, *shape):
    return (torch.randn(*shape, generator=gen) * 0.1).to(DEV)


def _offset(val):
    """A copy of `val` that starts one element into a buffer: not 16-byte
    aligned (8-byte for 16-bit types: odd element offset)."""
    buf = torch.empty(val.numel() + 1, dtype=val.dtype, device=val.device)
    out = buf[1:].view(val.shape)
    out.copy_(val)
    assert out.data_ptr() % 16 != 0
    return out


def _offset_like(src, val):
    return val if src.data_ptr() % 16 == 0 else _offset(val)


def _clone(ts):
    """Clones that keep strides and (mis)alignment."""
    return [_offset_like(t, t.clone()) for t in ts]


@functools.lru_cache(maxsize=None)
def _inputs():
    """(ws, gs, ms, es): 36 fp32 tensors each. Shared and read-only: every
    test that writes works on clones."""
    gen = torch.Generator().manual_seed(4321)
    out = ([], [], [], [])
    for _ in range(REPS):
        for s in SIZES:
            for ts in out:
                ts.append(_rnd(gen, s))
        for ts in out:
            ts.append(_rnd(gen, 64, 3, 3, 3).contiguous(memory_format=CL))
        for ts in out:
            ts.append(_offset(_rnd(gen, CHUNK + 77)))
    assert len(out[0]) == 36 > _backend.C().MT_MAX_TENSORS
    return out


def _coeffs(n):
    gen = torch.Generator().manual_seed(5)
    gscale = torch.tensor([0.7], device=DEV)
    ratio = (0.5 + torch.rand(n, generator=gen)).to(DEV)
    return gscale, ratio


def _launch(ps, gs, ms, scaled, emas=None, w16s=None, decay=D):
    C = _backend.C()
    kw = {}
    if w16s is not None:
        kw["w16s"] = w16s
    if emas is not None:
        kw.update(emas=emas, ema_decay=decay)
    mu = MU if ms else 0.0
    if scaled:
        gscale, ratio = _coeffs(len(ps))
        C.multi_tensor_sgd_scaled(ps, gs, ms, LR, mu, WD, gscale, ratio, **kw)
    else:
        C.multi_tensor_sgd(ps, gs, ms, LR, mu, WD, **kw)


def _launch_o2(ps, gs, ws, ms, scaled, emas=None, decay=D):
    C = _backend.C()
    kw = {} if emas is None else dict(emas=emas, ema_decay=decay)
    mu = MU if ms else 0.0
    if scaled:
        gscale, ratio = _coeffs(len(ps))
        C.multi_tensor_sgd_o2_scaled(ps, gs, ws, ms, LR, mu, WD, gscale,
                                     ratio, **kw)
    else:
        C.multi_tensor_sgd_o2(ps, gs, ws, ms, LR, mu, WD, **kw)


def _assert_avg(es, e0s, ws, d=D, what=""):
    for i, (e, e0, w) in enumerate(zip(es, e0s, ws)):
        want = d * e0.double() + (1 - d) * w.double()
        err = float((e.double() - want).abs().max())
        assert err <= 1e-6, (what, i, err)


def _assert_equal(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), (what, i)


# ---- 1. the SGD kernels with EMA ------------------------------------------------

@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_sgd_ema_vs_float64(scaled, momentum):
    ws0, gs0, ms0, es0 = _inputs()
    gs = list(gs0)
    p1, p2 = _clone(ws0), _clone(ws0)
    m1, m2 = (_clone(ms0), _clone(ms0)) if momentum else ([], [])
    e1 = _clone(es0)
    assert e1[-1].data_ptr() % 16 != 0 and e1[0].data_ptr() % 16 == 0
    _launch(p1, gs, m1, scaled, emas=e1)
    _launch(p2, gs, m2, scaled)
    _assert_equal(p1, p2, "p")
    _assert_equal(m1, m2, "m")
    for p, w0 in zip(p1, ws0):
        assert not torch.equal(p, w0)
    _assert_avg(e1, es0, p1)
    _assert_equal(gs, gs0, "g unmodified")


@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
def test_sgd_o2_ema_vs_float64(scaled, momentum):
    ws0, gs0, ms0, es0 = _inputs()
    gs = [_offset_like(g, g.bfloat16()) for g in gs0]
    mk = lambda: [_offset_like(w, w.bfloat16()) for w in ws0]   # noqa: E731
    p1, p2 = mk(), mk()
    w1, w2 = _clone(ws0), _clone(ws0)
    m1, m2 = (_clone(ms0), _clone(ms0)) if momentum else ([], [])
    e1 = _clone(es0)
    _launch_o2(p1, gs, w1, m1, scaled, emas=e1)
    _launch_o2(p2, gs, w2, m2, scaled)
    _assert_equal(p1, p2, "p")
    _assert_equal(w1, w2, "master")
    _assert_equal(m1, m2, "m")
    for p, w in zip(p1, w1):
        assert torch.equal(p, w.bfloat16())
    _assert_avg(e1, es0, w1)


# ---- 2. vector path == scalar path ---------------------------------------------

@pytest.mark.parametrize("which", ["p", "g", "m", "ema"])
def test_vector_and_scalar_paths_agree(which):
    ws0, gs0, ms0, es0 = _inputs()
    n = len(SIZES)   # the aligned 1-D tensors of the first repetition
    base = dict(p=ws0[:n], g=gs0[:n], m=ms0[:n], ema=es0[:n])
    for scaled in (False, True):
        a = {k: [t.clone() for t in v] for k, v in base.items()}
        b = {k: [_offset(t) if k == which else t.clone() for t in v]
             for k, v in base.items()}
        assert all(t.data_ptr() % 16 == 0 for v in a.values() for t in v)
        _launch(a["p"], a["g"], a["m"], scaled, emas=a["ema"])
        _launch(b["p"], b["g"], b["m"], scaled, emas=b["ema"])
        for k in ("p", "m", "ema"):
            _assert_equal(a[k], b[k], (which, scaled, k))


# ---- 3. edge cases ---------------------------------------------------------------

def test_none_entries_and_live_shadows():
    ws0, gs0, ms0, es0 = _inputs()
    n = len(ws0)
    p1, p2 = _clone(ws0), _clone(ws0)
    m1, m2 = _clone(ms0), _clone(ms0)
    emas = [None if i % 3 == 1 else e for i, e in enumerate(_clone(es0))]
    # bf16 and fp16 shadows in one launch, on aligned and unaligned tensors
    dts = [None, torch.bfloat16, torch.float16]
    w16s = [None if dts[i % 3] is None else
            _offset_like(ws0[i], torch.zeros_like(ws0[i], dtype=dts[i % 3]))
            for i in range(n)]
    _launch(p1, list(gs0), m1, False, emas=emas, w16s=w16s)
    _launch(p2, list(gs0), m2, False)
    _assert_equal(p1, p2, "p")
    _assert_equal(m1, m2, "m")
    have = [i for i in range(n) if emas[i] is not None]
    assert 0 < len(have) < n
    _assert_avg([emas[i] for i in have], [es0[i] for i in have],
                [p1[i] for i in have])
    for i, w16 in enumerate(w16s):
        if w16 is not None:
            assert torch.equal(w16, p1[i].to(w16.dtype)), i
    # all None in an EMA launch: nothing but the plain update happens
    p3, m3 = _clone(ws0), _clone(ms0)
    _launch(p3, list(gs0), m3, False, emas=[None] * n)
    _assert_equal(p3, p2, "p, all None")


def test_binding_checks():
    ws0, gs0, ms0, es0 = _inputs()
    C = _backend.C()
    p, g, m = [ws0[2].clone()], [gs0[2]], [ms0[2].clone()]
    with pytest.raises(RuntimeError, match="one ema entry"):
        C.multi_tensor_sgd(p, g, m, LR, MU, WD, emas=[None, None],
                           ema_decay=D)
    with pytest.raises(RuntimeError, match="ema must be float32"):
        C.multi_tensor_sgd(p, g, m, LR, MU, WD, emas=[es0[2].bfloat16()],
                           ema_decay=D)
    with pytest.raises(RuntimeError, match="ema must be float32"):
        C.multi_tensor_sgd(p, g, m, LR, MU, WD, emas=[es0[3].clone()],
                           ema_decay=D)
    with pytest.raises(RuntimeError, match="layout"):
        C.multi_tensor_ema([ws0[7]], [ws0[7].contiguous()], D)   # CL vs NCHW
    assert torch.equal(p[0], ws0[2])   # nothing ran


# ---- 4. multi_tensor_ema ---------------------------------------------------------

def test_multi_tensor_ema():
    ws0, _, _, es0 = _inputs()
    srcs = _clone(ws0)
    e1 = _clone(es0)
    multi_tensor_ema(srcs, e1, D)
    _assert_avg(e1, es0, ws0)
    _assert_equal(srcs, ws0, "sources unmodified")
    # aligned == unaligned, each side misaligned in turn
    n = len(SIZES)
    a = [t.clone() for t in es0[:n]]
    multi_tensor_ema([t.clone() for t in ws0[:n]], a, D)
    _assert_equal(a, e1[:n], "same values")
    for side in ("src", "ema"):
        s = [_offset(t) if side == "src" else t.clone() for t in ws0[:n]]
        b = [_offset(t) if side == "ema" else t.clone() for t in es0[:n]]
        multi_tensor_ema(s, b, D)
        _assert_equal(a, b, side)
    # d = 0 copies exactly
    e0 = _clone(es0)
    multi_tensor_ema(srcs, e0, 0.0)
    _assert_equal(e0, ws0, "d = 0")


# ---- 5, 6. ResNet-18 end to end ---------------------------------------------------

@pytest.fixture
def no_autotune(monkeypatch):
    # the launch heuristics hold no kernel that accumulates with atomics, so
    # twin runs agree bit for bit
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    return monkeypatch


def _resnet(ema_decay):
    from mi355x_ddp.config import TrainConfig
    from mi355x_ddp.core.worker import build_training, init_seeds

    init_seeds(0)
    cfg = TrainConfig(batch_size=8, amp="bf16", sync_bn=False,
                      channels_last=True, ema_decay=ema_decay)
    model, crit, opt, _, _ = build_training(
        cfg, torch.device(DEV, 0), world_size=1, rank=0, distributed=True,
        wrap="flat")
    return model, crit, opt


def _batch(i):
    g = torch.Generator().manual_seed(200 + i)
    x = torch.randn(8, 3, 32, 32, generator=g).to(DEV) \
        .contiguous(memory_format=CL)
    return x, torch.randint(0, 100, (8,), generator=g).to(DEV)


def _train_step(model, crit, opt, i):
    x, y = _batch(i)
    model.train()
    model.zero_grad_buffer()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = crit(model(x), y)
    loss.backward()
    model.finalize_backward()
    opt.step()


def _buffers(ema):
    return {k: b for k, (b, _) in ema.buffers.items()}


def _check_shadows(model):
    n = 0
    for p in model.parameters():
        sh = shadow_of(p)
        if sh is not None:
            sh.check(p)
            n += 1
    assert n >= 20   # ResNet-18's convs


def test_resnet18_three_steps(no_autotune):
    model, crit, opt = _resnet(D)
    twin, tcrit, topt = _resnet(0.0)
    ema = opt.weight_ema
    assert not hasattr(topt, "weight_ema")
    ps = list(model.parameters())
    want_p = [p.detach().double().clone() for p in ps]
    want_b = {k: b.double().clone() for k, b in _buffers(ema).items()}
    assert len(want_b) == 40   # 20 BatchNorm layers, mean and var
    for i in range(3):
        _train_step(model, crit, opt, i)
        _train_step(twin, tcrit, topt, i)
        for j, p in enumerate(ps):
            want_p[j] = D * want_p[j] + (1 - D) * p.detach().double()
        for k, b in _buffers(ema).items():
            want_b[k] = D * want_b[k] + (1 - D) * b.double()
    for j, (p, q) in enumerate(zip(ps, twin.parameters())):
        assert torch.equal(p.detach(), q.detach()), j
        assert torch.equal(opt.state[p]["momentum_buffer"],
                           topt.state[q]["momentum_buffer"]), j
        e = opt.state[p]["ema"]
        assert float((e.double() - want_p[j]).abs().max()) <= 1e-6, j
    moved = 0
    for j, p in enumerate(ps):
        moved += not torch.equal(opt.state[p]["ema"], p.detach())
    assert moved == len(ps)
    for a, b in zip(model.buffers(), twin.buffers()):
        assert torch.equal(a, b)
    for k, (b, avg) in ema.buffers.items():
        assert float((avg.double() - want_b[k]).abs().max()) <= 1e-6, k
        assert not torch.equal(avg, b), k
    _check_shadows(model)


def test_swap_under_shadows(no_autotune):
    model, crit, opt = _resnet(D)
    twin, tcrit, topt = _resnet(0.0)
    for i in range(3):
        _train_step(model, crit, opt, i)
        _train_step(twin, tcrit, topt, i)
    ema = opt.weight_ema
    sd = ema.state_dict()
    fresh, _, _ = _resnet(0.0)
    fresh.module.load_state_dict(sd)
    x, _ = _batch(9)

    def eval_forward(m):
        m.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x)

    want = eval_forward(fresh)
    raw = eval_forward(model)
    assert not torch.equal(raw, want)
    with ema.swapped():
        for k, v in model.module.state_dict().items():
            assert torch.equal(v, sd[k]), k
        got = eval_forward(model)
        _check_shadows(model)
    assert torch.equal(got, want)
    _check_shadows(model)   # rewritten at exit, before any forward
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(p.detach(), q.detach())
    _train_step(model, crit, opt, 3)
    _train_step(twin, tcrit, topt, 3)
    for j, (p, q) in enumerate(zip(model.parameters(), twin.parameters())):
        assert torch.equal(p.detach(), q.detach()), j
    for a, b in zip(model.buffers(), twin.buffers()):
        assert torch.equal(a, b)
    _check_shadows(model)


# ---- 7. hipGraph --------------------------------------------------------------------

def _make_net():
    torch.manual_seed(11)
    # ReLU-free, like the exact graph test of test_train_gpu.py: borderline
    # ReLU mask flips would make eager and replay drift legitimately
    return nn.Sequential(
        nn.Conv2d(3, 16, 3, padding=1), nn.BatchNorm2d(16), nn.Tanh(),
        nn.Conv2d(16, 32, 3, stride=2, padding=1),
        nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(), nn.Linear(32, 10))


def test_hip_graph_step_with_ema_matches_eager():
    from mi355x_ddp.config import TrainConfig
    from mi355x_ddp.core.ema import WeightEMA
    from mi355x_ddp.core.graphs import GraphedTrainStep
    from mi355x_ddp.core.worker import init_seeds
    from mi355x_ddp.parallel import FlatDDP

    init_seeds(0, deterministic=True)
    gen = torch.Generator().manual_seed(3)
    data = [(torch.randn(16, 3, 16, 16, generator=gen).pin_memory(),
             torch.randint(0, 10, (16,), generator=gen).pin_memory())
            for _ in range(3)]
    device = torch.device("cuda", 0)
    crit = nn.CrossEntropyLoss()

    def make_opt(model):
        opt = FusedSGD(model.parameters(), lr=0.05, momentum=0.9,
                       weight_decay=1e-4, ema_decay=D)
        return opt, WeightEMA(model, opt)

    def result(model, opt, ema):
        ps = [p.detach().clone() for p in model.parameters()]
        es = [opt.state[p]["ema"].clone() for p in model.parameters()]
        bs = [avg.clone() for _, avg in ema.buffers.values()]
        return ps, es, bs

    def eager():
        model = FlatDDP(_make_net().to(device), overlap=True)
        opt, ema = make_opt(model)
        model.train()
        for img, lbl in data:
            model.zero_grad_buffer()
            crit(model(img.to(device)), lbl.to(device)).backward()
            model.finalize_backward()
            opt.step()
        return result(model, opt, ema)

    def graphed():
        cfg = TrainConfig(batch_size=16, amp="fp32", sync_bn=False,
                          hip_graph=True)
        model = FlatDDP(_make_net().to(device), overlap=False,
                        static_grads=True)
        opt, ema = make_opt(model)
        model.train()
        snap = [p.detach().clone() for p in model.parameters()]
        bufs = [b.detach().clone() for b in model.buffers()]
        # the averages materialise in the warm-up steps, like the momentum
        # buffers; the capture succeeding shows the step has no host sync
        step = GraphedTrainStep(model, crit, opt, cfg, device, batch=16,
                                image_size=16, num_classes=10)
        ptrs = [opt.state[p]["ema"].data_ptr() for p in model.parameters()]
        with torch.no_grad():
            for p, s in zip(model.parameters(), snap):
                p.copy_(s)
                opt.state[p]["ema"].copy_(s)
            for b, s in zip(model.buffers(), bufs):
                b.copy_(s)
            ema.reset_buffers()
            for st in opt.state.values():
                st["momentum_buffer"].zero_()
        graph = step.graph
        for img, lbl in data:
            step.run(img, lbl)
            assert step.graph is graph
        torch.cuda.synchronize()
        assert ptrs == [opt.state[p]["ema"].data_ptr()
                        for p in model.parameters()]
        return result(model, opt, ema) + (snap,)

    (pe, ee, be), (pg, eg, bg, start) = eager(), graphed()
    for what, xs, ys in (("p", pe, pg), ("ema", ee, eg), ("buf ema", be, bg)):
        for a, b in zip(xs, ys):
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-5), \
                (what, (a - b).abs().max())
    # A capture that dropped the average would leave ema == w0, one that
    # copied would leave ema == p. Where the weight moved (everywhere but the
    # first conv's bias, whose gradient BatchNorm makes zero), the average of
    # w0..w3 is neither.
    moved = 0
    for p, e, w0 in zip(pg, eg, start):
        if torch.equal(p, w0):
            continue
        moved += 1
        assert not torch.equal(e, p) and not torch.equal(e, w0)
    assert moved >= len(pg) - 1
    assert len(bg) == 2


# ---- 8. a skipped fp16 step ---------------------------------------------------------

def test_overflow_skips_the_averages():
    from mi355x_ddp.core.amp import DynamicLossScaler

    ws0, gs0, _, _ = _inputs()
    n = len(SIZES)
    ps = [nn.Parameter(w.clone()) for w in ws0[:n]]
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, ema_decay=D)
    stat = ws0[n + 1].clone()
    avg = stat.clone()
    opt.track_buffers([(stat, avg)])
    scaler = DynamicLossScaler(init_scale=4.0)
    for p, g in zip(ps, gs0[:n]):
        p.grad = g * 4.0
    assert scaler.unscale_([p.grad for p in ps]) is False
    assert scaler.step(opt) is True
    before = [opt.state[p]["ema"].clone() for p in ps]
    for p, e, w0 in zip(ps, before, ws0[:n]):
        assert not torch.equal(e, w0)   # the step that ran did average
    stat.add_(1.0)
    avg0 = avg.clone()
    for p, g in zip(ps, gs0[:n]):
        p.grad = g * 4.0
    ps[2].grad[5] = float("inf")
    weights = [p.detach().clone() for p in ps]
    assert scaler.unscale_([p.grad for p in ps]) is True
    assert scaler.step(opt) is False
    assert scaler.scale == 2.0
    for p, e, w in zip(ps, before, weights):
        assert torch.equal(opt.state[p]["ema"], e)
        assert torch.equal(p.detach(), w)
    assert torch.equal(avg, avg0)


# ---- 9. O2 state through load_state_dict ----------------------------------------

def test_o2_resume_keeps_fp32_state_and_steps_natively():
    """torch's load_state_dict would cast master, momentum and average to the
    bf16 parameter's dtype, and the native step refuses those."""
    import copy

    ws0, gs0, _, _ = _inputs()
    n = len(SIZES)
    mk = lambda: [nn.Parameter(w.bfloat16()) for w in ws0[:n]]   # noqa: E731
    ps, qs = mk(), mk()
    kw = dict(lr=LR, momentum=MU, weight_decay=WD, ema_decay=D)
    opt, opt2 = FusedSGD(ps, **kw), FusedSGD(qs, **kw)
    for p, g in zip(ps, gs0[:n]):
        p.grad = g.bfloat16()
    opt.step()
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    rep = n + 2   # tensors per repetition of _inputs: the same sizes again
    for p, q, g in zip(ps, qs, gs0[rep:rep + n]):
        assert g.shape == p.shape
        p.grad, q.grad = g.bfloat16(), g.bfloat16()
    opt.step()
    opt2.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
        for k in ("master", "momentum_buffer", "ema"):
            a, b = opt.state[p][k], opt2.state[q][k]
            assert b.dtype == torch.float32 and torch.equal(a, b), k
