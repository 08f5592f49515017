"""LARS and gradient-norm clipping in FusedSGD: the torch fallback path.

Clipping against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD, LARS
against a float64 reference written out here from the documented formulas,
the unchanged default step, config/CLI wiring, and a 2-rank gloo run.
"""
import argparse
import copy
import json

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from mi355x_ddp.config import TrainConfig, add_common_args, config_from_args
from mi355x_ddp.ops import FusedSGD
from mi355x_ddp.ops.sgd import sgd_coeffs_torch

LR, MU, WD = 0.1, 0.9, 1e-2


def _params(shapes, seed, std=0.1):
    gen = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(*s, generator=gen) * std)
            for s in shapes]


def _grads(shapes, seed, std=0.1):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) * std for s in shapes]


def ref_step64(ws, gs, ms, lr, mu, wd, lars, eta, max_norm):
    """One step of the documented formulas in float64, in place on the
    float64 lists ws/ms. Returns (norm, c, ratios)."""
    norm = sum(float(g.pow(2).sum()) for g in gs) ** 0.5
    c = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    ratios = []
    for w, g, m in zip(ws, gs, ms):
        wn, gn = float(w.norm()), float(g.norm())
        r = 1.0
        if lars and w.ndim > 1 and wn > 0 and gn > 0:
            r = eta * wn / (c * gn + wd * wn + 1e-8)
        ratios.append(r)
        d = r * (c * g + wd * w)
        m.mul_(mu).add_(d)
        w.sub_(lr * m)
    return norm, c, ratios


# ---- clipping vs torch ------------------------------------------------------

@pytest.mark.parametrize("max_norm,clips", [(0.5, True), (1e3, False)])
def test_clip_matches_torch(max_norm, clips):
    shapes = [(8, 5), (5,), (4, 3, 3, 3), (1,)]
    ours = _params(shapes, 1, std=1.0)
    theirs = [nn.Parameter(p.detach().clone()) for p in ours]
    o1 = FusedSGD(ours, lr=LR, momentum=MU, weight_decay=WD,
                  clip_grad_norm=max_norm)
    o2 = torch.optim.SGD(theirs, lr=LR, momentum=MU, weight_decay=WD)
    for step in range(3):
        grads = _grads(shapes, 10 + step, std=1.0)
        for p, q, g in zip(ours, theirs, grads):
            p.grad = g.clone()
            q.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(theirs, max_norm)
        assert (float(total) > max_norm) == clips
        o1.step()
        o2.step()
        # the gradients are not modified: clipping happens inside the update
        for p, g in zip(ours, grads):
            assert torch.equal(p.grad, g)
        assert torch.allclose(o1.grad_norm(), total, rtol=1e-6)
        for p, q in zip(ours, theirs):
            assert torch.allclose(p, q, atol=1e-6), (p - q).abs().max()


# ---- LARS vs the float64 reference -------------------------------------------

# 0: ordinary, 1: zero gradient, 2: zero weight, 3: 1-D, 4: ordinary 4-D
LARS_SHAPES = [(8, 5), (4, 3), (3, 3), (7,), (4, 2, 3, 3)]


@pytest.mark.parametrize("max_norm", [0.0, 0.2])
def test_lars_matches_float64_reference(max_norm):
    eta = 1.0   # ratios of order 1: a wrong ratio cannot hide under atol
    ps = _params(LARS_SHAPES, 2)
    with torch.no_grad():
        ps[2].zero_()
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, lars=True,
                   lars_eta=eta, clip_grad_norm=max_norm)
    ws = [p.detach().double().clone() for p in ps]
    ms = [torch.zeros_like(w) for w in ws]
    for step in range(2):
        grads = _grads(LARS_SHAPES, 20 + step)
        grads[1].zero_()
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        norm, c, ratios = ref_step64(ws, [g.double() for g in grads], ms,
                                     LR, MU, WD, True, eta, max_norm)
        if step == 0:
            assert ratios[1] == 1.0 and ratios[2] == 1.0 and ratios[3] == 1.0
            assert ratios[0] != 1.0 and ratios[4] != 1.0
            assert (c < 1.0) == (max_norm > 0)
        assert abs(float(opt.grad_norm()) - norm) <= 1e-6 * norm
        # values are N(0, 0.1^2) and ratios O(1): fp32 rounding of the few
        # operations per step stays far below the project's SGD atol
        for p, w, m in zip(ps, ws, ms):
            assert torch.allclose(p.detach().double(), w, atol=1e-6, rtol=0), \
                (p.detach().double() - w).abs().max()
            buf = opt.state[p]["momentum_buffer"].double()
            assert torch.allclose(buf, m, atol=1e-6, rtol=0)


def test_coeffs_ratio_one_cases():
    """Zero gradient, zero weight and excluded tensors get exactly 1; so does
    every tensor when LARS is off."""
    sq_w = torch.tensor([4.0, 9.0, 0.0, 1.0, 16.0])
    sq_g = torch.tensor([1.0, 0.0, 2.0, 3.0, 4.0])
    excluded = [False, False, False, True, False]
    c, ratio, norm = sgd_coeffs_torch(sq_w, sq_g, excluded, 1.0, True, 1.0,
                                      WD)
    assert torch.allclose(norm, torch.tensor(10.0).sqrt())
    want_c = 1.0 / (10.0 ** 0.5 + 1e-6)
    assert abs(float(c) - want_c) < 1e-6
    assert ratio[1] == 1 and ratio[2] == 1 and ratio[3] == 1
    for t in (0, 4):
        wn, gn = float(sq_w[t]) ** 0.5, float(sq_g[t]) ** 0.5
        want = wn / (want_c * gn + WD * wn + 1e-8)
        assert abs(float(ratio[t]) - want) <= 1e-5 * want
    c, ratio, _ = sgd_coeffs_torch(sq_w, sq_g, excluded, 0.0, False, 1.0, WD)
    assert float(c) == 1.0 and torch.equal(ratio, torch.ones(5))


def test_bf16_master_path_matches_reference():
    """O2 parameters: norms and the update run on the fp32 master."""
    eta, max_norm = 1.0, 0.2
    shapes = [(8, 5), (6,)]
    ps = [nn.Parameter(p.detach().bfloat16()) for p in _params(shapes, 3)]
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, lars=True,
                   lars_eta=eta, clip_grad_norm=max_norm)
    ws = [p.detach().double().clone() for p in ps]
    ms = [torch.zeros_like(w) for w in ws]
    for step in range(2):
        grads = [g.bfloat16() for g in _grads(shapes, 30 + step)]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ref_step64(ws, [g.double() for g in grads], ms, LR, MU, WD, True,
                   eta, max_norm)
        for p, w in zip(ps, ws):
            master = opt.state[p]["master"]
            assert torch.allclose(master.double(), w, atol=1e-6, rtol=0)
            assert torch.equal(p.detach(), master.bfloat16())


# ---- defaults ----------------------------------------------------------------

def test_default_step_is_bitwise_unchanged():
    shapes = [(8, 5), (5,), (4, 3, 3, 3)]
    ps = _params(shapes, 4)
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD)
    assert opt.grad_norm() is None
    ws = [p.detach().clone() for p in ps]
    bufs = [torch.zeros_like(w) for w in ws]
    for step in range(3):
        grads = _grads(shapes, 40 + step)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        # the step as it was before LARS and clipping existed
        for w, g, buf in zip(ws, grads, bufs):
            g = g.add(w, alpha=WD)
            buf.mul_(MU).add_(g)
            w.add_(buf, alpha=-LR)
        for p, w in zip(ps, ws):
            assert torch.equal(p.detach(), w)
    assert opt.grad_norm() is None
    group = opt.param_groups[0]
    assert (group["lars"], group["lars_eta"], group["clip_grad_norm"]) \
        == (False, 1e-3, 0.0)


def test_old_state_dict_loads_and_steps():
    shapes = [(6, 4), (4,)]
    ps = _params(shapes, 5)
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD)
    for p, g in zip(ps, _grads(shapes, 50)):
        p.grad = g
    opt.step()
    sd = copy.deepcopy(opt.state_dict())   # as if saved and loaded
    for group in sd["param_groups"]:   # a checkpoint from before this change
        for k in ("lars", "lars_eta", "clip_grad_norm"):
            del group[k]
    qs = [nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = FusedSGD(qs, lr=1.0)
    opt2.load_state_dict(sd)
    assert "lars" not in opt2.param_groups[0]
    for p, q, g in zip(ps, qs, _grads(shapes, 51)):
        p.grad = g.clone()
        q.grad = g.clone()
    opt.step()
    opt2.step()
    assert opt2.grad_norm() is None
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())


def test_param_without_grad_is_skipped():
    shapes = [(6, 4), (5, 3), (4,)]
    ps = _params(shapes, 6)
    before = ps[1].detach().clone()
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, lars=True,
                   lars_eta=1.0, clip_grad_norm=0.1)
    grads = _grads(shapes, 60)
    ps[0].grad, ps[2].grad = grads[0].clone(), grads[2].clone()
    opt.step()
    assert torch.equal(ps[1].detach(), before)
    want = (grads[0].double().pow(2).sum()
            + grads[2].double().pow(2).sum()).sqrt()
    assert abs(float(opt.grad_norm()) - float(want)) <= 1e-6 * float(want)


# ---- config, CLI, engine -----------------------------------------------------

def test_validation_errors():
    cfg = TrainConfig()
    assert (cfg.lars, cfg.lars_eta, cfg.clip_grad_norm) == (False, 1e-3, 0.0)
    TrainConfig(lars=True, lars_eta=0.02, clip_grad_norm=1.0)
    p = nn.Parameter(torch.zeros(2))
    for bad in (0.0, -1e-3):
        with pytest.raises(ValueError, match="lars_eta"):
            TrainConfig(lars_eta=bad)
        with pytest.raises(ValueError, match="lars_eta"):
            FusedSGD([p], lr=0.1, lars_eta=bad)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        TrainConfig(clip_grad_norm=-1.0)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        FusedSGD([p], lr=0.1, clip_grad_norm=-1.0)


def test_cli_flags():
    parser = add_common_args(argparse.ArgumentParser())
    cfg = config_from_args(parser.parse_args([]))
    assert (cfg.lars, cfg.lars_eta, cfg.clip_grad_norm) == (False, 1e-3, 0.0)
    cfg = config_from_args(parser.parse_args(
        ["--lars", "--lars_eta", "0.02", "--clip_grad_norm", "2.5"]))
    assert (cfg.lars, cfg.lars_eta, cfg.clip_grad_norm) == (True, 0.02, 2.5)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        config_from_args(parser.parse_args(["--clip_grad_norm", "-1"]))


def _train_records(tmp_path, **kw):
    from mi355x_ddp.core.engine import train_one_epoch
    from mi355x_ddp.core.metrics import JsonlSink
    from mi355x_ddp.core.worker import build_training, init_seeds
    from mi355x_ddp.data import build_loaders

    init_seeds(0)
    device = torch.device("cpu")
    cfg = TrainConfig(batch_size=8, epochs=1, num_workers=0, log_interval=1,
                      synthetic=True, lr=0.05, stall_dump_s=None, **kw)
    model, crit, opt, sched, scaler = build_training(
        cfg, device, 1, 0, distributed=True, wrap="flat")
    train_loader, _, _ = build_loaders(cfg, 1, 0, distributed=False)
    sink = JsonlSink(str(tmp_path), name="m")
    train_one_epoch(model, train_loader, crit, opt, 0, cfg, device,
                    sink=sink, max_steps=2)
    with open(sink.path) as f:
        return opt, [json.loads(line) for line in f]


def test_build_wiring_and_grad_norm_record(tmp_path):
    opt, records = _train_records(tmp_path / "on", lars=True, lars_eta=0.02,
                                  clip_grad_norm=1.0)
    group = opt.param_groups[0]
    assert (group["lars"], group["lars_eta"], group["clip_grad_norm"]) \
        == (True, 0.02, 1.0)
    assert len(records) == 2
    for r in records:
        assert r["grad_norm"] > 0
    # features off: the record is the one from before
    _, records = _train_records(tmp_path / "off")
    assert len(records) == 2
    for r in records:
        assert set(r) == {"kind", "epoch", "step", "loss", "lr", "step_time",
                          "ts"}


# ---- two ranks ---------------------------------------------------------------

def _worker(rank, world, port):
    dist.init_process_group(
        backend="gloo", init_method=f"tcp://127.0.0.1:{port}",
        world_size=world, rank=rank)
    try:
        from mi355x_ddp.parallel import FlatDDP
        torch.manual_seed(42)   # same init on both ranks
        net = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))
        model = FlatDDP(net, bucket_cap_mb=1e-5)
        opt = FusedSGD(model.parameters(), lr=LR, momentum=MU,
                       weight_decay=WD, lars=True, clip_grad_norm=1.0)
        start = [p.detach().clone() for p in net.parameters()]
        gen = torch.Generator().manual_seed(7 + rank)   # different data
        for _ in range(2):
            model.zero_grad_buffer()
            model(torch.randn(4, 8, generator=gen)).pow(2).mean().backward()
            model.finalize_backward()
            opt.step()
        assert any(not torch.equal(p.detach(), s)
                   for p, s in zip(net.parameters(), start))
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]
                         + [opt.grad_norm().reshape(1)])
        gathered = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(gathered, flat)
        assert torch.equal(gathered[0], gathered[1])
    finally:
        dist.destroy_process_group()


def test_two_ranks_end_with_identical_parameters(free_port):
    mp.spawn(_worker, nprocs=2, args=(2, free_port))
