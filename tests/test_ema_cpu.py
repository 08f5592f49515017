"""Weight EMA without a GPU: the average kept by FusedSGD's torch path against
a float64 recursion, the untouched update, WeightEMA's swap and state dict, the
O2 masters, skipped fp16 steps, checkpoints, config and a short `fit`.

Inputs are N(0, 0.1^2) as in test_lars_clip_gpu.py. One average step is at
most three roundings (d*e, omd*w, their sum) of values below 1, about 9e-8
together, and d < 1 contracts what earlier steps left: atol 1e-6 holds with
room. The decay is 0.5, not 0.999: at 0.999 a missing update would hide under
any tolerance.
"""
import argparse
import copy
import json

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.config import TrainConfig, add_common_args, config_from_args
from mi355x_ddp.core.amp import DynamicLossScaler, cast_model_bf16
from mi355x_ddp.core.checkpoint import load_checkpoint, save_checkpoint
from mi355x_ddp.core.ema import WeightEMA
from mi355x_ddp.ops import sgd
from mi355x_ddp.ops.sgd import FusedSGD

LR, MU, WD, D = 0.1, 0.9, 1e-2, 0.5
SHAPES = [(1,), (3,), (255,), (64, 3, 3, 3), (17, 33)]


def _rnd(gen, *shape):
    return torch.randn(*shape, generator=gen) * 0.1


def _params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [nn.Parameter(_rnd(gen, *s)) for s in SHAPES]


def _grads(seed):
    gen = torch.Generator().manual_seed(seed)
    return [_rnd(gen, *s) for s in SHAPES]


# ---- 1-3. the average in the optimizer ---------------------------------------

def test_ema_vs_float64_recursion():
    ps = _params(1)
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, ema_decay=D)
    want = [p.detach().double().clone() for p in ps]   # e0 = w0
    for step in range(3):
        for p, g in zip(ps, _grads(10 + step)):
            p.grad = g
        opt.step()
        for i, p in enumerate(ps):
            want[i] = D * want[i] + (1 - D) * p.detach().double()
            got = opt.state[p]["ema"]
            assert got.dtype == torch.float32 and got.shape == p.shape
            err = float((got.double() - want[i]).abs().max())
            assert err <= 1e-6, (step, i, err)
    # an average that followed nothing would still equal w0
    for p, e0 in zip(ps, _params(1)):
        assert not torch.equal(opt.state[p]["ema"], e0.detach())


@pytest.mark.parametrize("scaled", [False, True])
def test_ema_leaves_update_bit_for_bit(scaled):
    kw = dict(lars=True, lars_eta=1.0, clip_grad_norm=0.1) if scaled else {}
    ps, qs = _params(2), _params(2)
    on = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, ema_decay=D, **kw)
    off = FusedSGD(qs, lr=LR, momentum=MU, weight_decay=WD, **kw)
    assert on.param_groups[0]["ema_decay"] == D
    assert off.param_groups[0]["ema_decay"] == 0.0
    for step in range(3):
        for p, q, g in zip(ps, qs, _grads(20 + step)):
            p.grad, q.grad = g.clone(), g.clone()
        on.step()
        off.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(on.state[p]["momentum_buffer"],
                           off.state[q]["momentum_buffer"])
        assert "ema" in on.state[p] and "ema" not in off.state[q]


def test_decay_zero_copies_the_new_weight():
    ws = [p.detach().clone() for p in _params(3)]
    emas = [torch.full_like(w, 7.0) for w in ws]
    emas[1] = None   # no average for this tensor
    sgd._update_torch(ws, _grads(30), [torch.zeros_like(w) for w in ws],
                      LR, MU, WD, None, None, emas=emas, ema_decay=0.0)
    for i, (w, e) in enumerate(zip(ws, emas)):
        if i != 1:
            assert torch.equal(e, w)
    # and the public function, on buffers
    srcs = _grads(31)
    avgs = [torch.full_like(s, -3.0) for s in srcs]
    keep = [s.clone() for s in srcs]
    sgd.multi_tensor_ema(srcs, avgs, 0.0)
    for s, a, k in zip(srcs, avgs, keep):
        assert torch.equal(a, s) and torch.equal(s, k)


def test_coefficients_are_float32_values():
    d, omd = sgd.ema_coeffs(0.999)
    assert d == float(torch.tensor(0.999, dtype=torch.float32))
    assert omd == float(torch.tensor(1.0) - torch.tensor(0.999))
    assert sgd.ema_coeffs(0.0) == (0.0, 1.0)


# ---- 4. the swap --------------------------------------------------------------

def _net():
    torch.manual_seed(5)
    return nn.Sequential(
        nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(),
        nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(), nn.Linear(8, 4))


def _trained(steps=3, **kw):
    """A small conv+BN net, its optimizer and WeightEMA after `steps` real
    training steps (the BN statistics move too)."""
    model = _net()
    opt = FusedSGD(model.parameters(), lr=LR, momentum=MU, weight_decay=WD,
                   ema_decay=D, **kw)
    ema = WeightEMA(model, opt)
    gen = torch.Generator().manual_seed(6)
    model.train()
    for _ in range(steps):
        x = torch.randn(8, 3, 8, 8, generator=gen)
        y = torch.randint(0, 4, (8,), generator=gen)
        opt.zero_grad()
        nn.functional.cross_entropy(model(x), y).backward()
        opt.step()
    return model, opt, ema


def _everything(model, opt, ema):
    out = {f"model.{k}": v.detach().clone()
           for k, v in model.state_dict().items()}
    for i, p in enumerate(model.parameters()):
        for k, v in opt.state[p].items():
            out[f"state.{i}.{k}"] = v.detach().clone()
    for k, (_, avg) in ema.buffers.items():
        out[f"avg.{k}"] = avg.clone()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_buffer_averages_follow_running_stats():
    model, opt, ema = _trained(steps=0)
    assert list(ema.buffers) == ["1.running_mean", "1.running_var"]
    want = {k: b.double().clone() for k, (b, _) in ema.buffers.items()}
    gen = torch.Generator().manual_seed(6)
    model.train()
    for _ in range(3):
        x = torch.randn(8, 3, 8, 8, generator=gen)
        y = torch.randint(0, 4, (8,), generator=gen)
        opt.zero_grad()
        nn.functional.cross_entropy(model(x), y).backward()
        opt.step()
        for k, (b, avg) in ema.buffers.items():
            want[k] = D * want[k] + (1 - D) * b.double()
            assert float((avg.double() - want[k]).abs().max()) <= 1e-6
    for b, avg in ema.buffers.values():
        assert not torch.equal(b, avg)


def test_swapped_holds_the_averages_and_restores():
    model, opt, ema = _trained()
    before = _everything(model, opt, ema)
    sd = ema.state_dict()
    assert list(sd) == list(model.state_dict())
    for i, (name, p) in enumerate(model.named_parameters()):
        assert torch.equal(sd[name], opt.state[p]["ema"])
        assert not torch.equal(sd[name], p.detach())
    assert torch.equal(sd["1.num_batches_tracked"], torch.tensor(3))
    ptrs = [p.data_ptr() for p in model.parameters()]
    versions = [p._version for p in model.parameters()]
    with ema.swapped():
        _assert_same(dict(model.state_dict()), dict(sd))
        _assert_same(dict(ema.state_dict()), dict(sd))
        assert [p.data_ptr() for p in model.parameters()] == ptrs
        # the writes went through the version counter (weight shadows)
        assert all(p._version > v
                   for p, v in zip(model.parameters(), versions))
        with pytest.raises(RuntimeError):
            ema.load_state_dict(sd)
    _assert_same(_everything(model, opt, ema), before)
    # the averaged model deploys into a fresh model
    fresh = _net()
    fresh.load_state_dict(sd)


def test_swapped_nested_and_exception():
    model, opt, ema = _trained()
    before = _everything(model, opt, ema)
    sd = ema.state_dict()
    with ema.swapped():
        with ema.swapped():
            _assert_same(dict(model.state_dict()), dict(sd))
        _assert_same(dict(model.state_dict()), dict(sd))
    _assert_same(_everything(model, opt, ema), before)
    with pytest.raises(ZeroDivisionError):
        with ema.swapped():
            1 / 0
    _assert_same(_everything(model, opt, ema), before)


def test_swapped_before_first_step_is_a_no_op_for_parameters():
    model, opt, ema = _trained(steps=0)
    before = _everything(model, opt, ema)
    with ema.swapped():
        _assert_same(dict(model.state_dict()), dict(ema.state_dict()))
        for k, v in model.state_dict().items():
            assert torch.equal(v, before[f"model.{k}"])
    _assert_same(_everything(model, opt, ema), before)


def test_unwraps_module():
    class Wrap(nn.Module):
        def __init__(self, m):
            super().__init__()
            self.module = m

    model = _net()
    opt = FusedSGD(model.parameters(), lr=LR, ema_decay=D)
    ema = WeightEMA(Wrap(model), opt)
    assert ema.module is model
    assert list(ema.state_dict()) == list(model.state_dict())


# ---- 5. O2 --------------------------------------------------------------------

def test_o2_average_tracks_the_master():
    torch.manual_seed(7)
    model = cast_model_bf16(nn.Sequential(
        nn.Linear(6, 5), nn.BatchNorm1d(5), nn.Linear(5, 3)))
    ps = list(model.parameters())
    assert all(p.dtype == torch.bfloat16 for p in ps)
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, ema_decay=D)
    ema = WeightEMA(model, opt)
    gen = torch.Generator().manual_seed(8)
    want = [p.detach().float().double() for p in ps]   # e0 = first master
    for _ in range(3):
        for p in ps:
            p.grad = _rnd(gen, *p.shape).bfloat16()
        opt.step()
        for i, p in enumerate(ps):
            st = opt.state[p]
            want[i] = D * want[i] + (1 - D) * st["master"].double()
            assert st["ema"].dtype == torch.float32
            assert float((st["ema"].double() - want[i]).abs().max()) <= 1e-6
            assert torch.equal(p.detach(), st["master"].bfloat16())
    before = _everything(model, opt, ema)
    avgs = [opt.state[p]["ema"].clone() for p in ps]
    with ema.swapped():
        for p, e in zip(ps, avgs):
            assert p.dtype == torch.bfloat16
            assert torch.equal(p.detach(), e.bfloat16())
            assert torch.equal(opt.state[p]["master"], e)
        sd = ema.state_dict()
        for (name, _), e in zip(model.named_parameters(), avgs):
            assert sd[name].dtype == torch.float32
            assert torch.equal(sd[name], e)
    _assert_same(_everything(model, opt, ema), before)


# ---- 6. a skipped step --------------------------------------------------------

def test_skipped_scaler_step_leaves_the_averages():
    model, opt, ema = _trained()
    before = _everything(model, opt, ema)
    for p in model.parameters():
        p.grad = torch.full_like(p, float("inf"))
    with torch.no_grad():
        model[1].running_mean.add_(1.0)   # a forward moved the statistics
    scaler = DynamicLossScaler()
    scaler.found_inf = True
    assert scaler.step(opt) is False
    after = _everything(model, opt, ema)
    assert not torch.equal(after.pop("model.1.running_mean"),
                           before.pop("model.1.running_mean"))
    _assert_same(after, before)   # parameter and buffer averages included
    # and a step that runs moves them
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    assert scaler.step(opt) is True
    assert not torch.equal(ema.buffers["1.running_mean"][1],
                           before["avg.1.running_mean"])
    p0 = next(model.parameters())
    assert not torch.equal(opt.state[p0]["ema"], before["state.0.ema"])


# ---- 7. checkpoints, config ----------------------------------------------------

def _attach(model, **kw):
    opt = FusedSGD(model.parameters(), lr=LR, momentum=MU, weight_decay=WD,
                   **kw)
    if kw.get("ema_decay", 0) > 0:
        opt.weight_ema = WeightEMA(model, opt)
    return opt


def test_checkpoint_round_trip(tmp_path):
    model, opt, ema = _trained()
    opt.weight_ema = ema
    path = save_checkpoint(str(tmp_path), "net", 0, model, opt)
    state = torch.load(path, weights_only=False)
    _assert_same(dict(state["ema"]), dict(ema.state_dict()))
    model2 = _net()
    opt2 = _attach(model2, ema_decay=D)
    load_checkpoint(path, model2, opt2)
    _assert_same(dict(opt2.weight_ema.state_dict()), dict(ema.state_dict()))
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(opt.state[p]["ema"], opt2.state[q]["ema"])
    for (_, a), (_, b) in zip(ema.buffers.values(),
                              opt2.weight_ema.buffers.values()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("written_by", ["this tree", "before the feature"])
def test_checkpoint_without_ema_loads(tmp_path, written_by):
    # written by a run without averages
    torch.manual_seed(9)
    model = _net()
    with torch.no_grad():
        model[1].running_mean.normal_()
    opt = _attach(model)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    path = save_checkpoint(str(tmp_path), "net", 0, model, opt)
    state = torch.load(path, weights_only=False)
    assert "ema" not in state
    for group in state["optimizer"]["param_groups"]:
        assert group["ema_decay"] == 0.0
        if written_by == "before the feature":
            del group["ema_decay"]   # the key did not exist
    torch.save(state, path)
    # into a run without averages: as before
    m2 = _net()
    opt2 = _attach(m2)
    load_checkpoint(path, m2, opt2)
    assert opt2.param_groups[0]["ema_decay"] == 0.0
    # into a run with them: the averages start from the loaded weights
    m3 = _net()
    opt3 = _attach(m3, ema_decay=D)
    load_checkpoint(path, m3, opt3)
    assert opt3.param_groups[0]["ema_decay"] == D
    _assert_same(dict(opt3.weight_ema.state_dict()), dict(m3.state_dict()))
    loaded = [p.detach().clone() for p in m3.parameters()]
    mean0 = m3[1].running_mean.clone()
    assert torch.equal(mean0, model[1].running_mean)
    for p in m3.parameters():
        p.grad = torch.ones_like(p)
    with torch.no_grad():
        m3[1].running_mean.add_(1.0)   # a forward moved the statistics
    opt3.step()
    for p, w0 in zip(m3.parameters(), loaded):
        want = D * w0.double() + (1 - D) * p.detach().double()
        assert float((opt3.state[p]["ema"].double() - want).abs().max()) \
            <= 1e-6
    # the buffer averages go on from the loaded statistics as well
    want = D * mean0.double() + (1 - D) * m3[1].running_mean.double()
    got = opt3.weight_ema.buffers["1.running_mean"][1]
    assert float((got.double() - want).abs().max()) <= 1e-6


def test_checkpoint_with_ema_into_a_run_without(tmp_path):
    model, opt, ema = _trained()
    opt.weight_ema = ema
    path = save_checkpoint(str(tmp_path), "net", 0, model, opt)
    m2 = _net()
    opt2 = _attach(m2)
    load_checkpoint(path, m2, opt2)
    assert opt2.param_groups[0]["ema_decay"] == 0.0   # the run's own
    kept = [opt2.state[p]["ema"].clone() for p in m2.parameters()]
    for p in m2.parameters():
        p.grad = torch.ones_like(p)
    opt2.step()
    for p, e in zip(m2.parameters(), kept):
        assert torch.equal(opt2.state[p]["ema"], e)   # carried, not updated


def test_buffers_need_one_positive_decay():
    model = _net()
    with pytest.raises(RuntimeError, match="ema_decay"):
        WeightEMA(model, FusedSGD(model.parameters(), lr=LR))
    ps = list(model.parameters())
    opt = FusedSGD([dict(params=ps[:2]), dict(params=ps[2:], ema_decay=0.9)],
                   lr=LR, ema_decay=D)
    with pytest.raises(RuntimeError, match="ema_decay"):
        WeightEMA(model, opt)
    # a decay that goes away later is caught at the step
    opt = FusedSGD(ps, lr=LR, ema_decay=D)
    WeightEMA(model, opt)
    opt.param_groups[0]["ema_decay"] = 0.0
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.step()


def test_o2_state_stays_fp32_through_load_state_dict():
    gen = torch.Generator().manual_seed(12)
    mk = lambda: [nn.Parameter(_rnd(gen, 33).bfloat16()),   # noqa: E731
                  nn.Parameter(_rnd(gen, 7))]
    ps = mk()
    opt = FusedSGD(ps, lr=LR, momentum=MU, weight_decay=WD, ema_decay=D)
    for _ in range(2):
        for p in ps:
            p.grad = _rnd(gen, *p.shape).to(p.dtype)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    qs = mk()
    opt2 = FusedSGD(qs, lr=LR, momentum=MU, weight_decay=WD, ema_decay=D)
    opt2.load_state_dict(sd)
    assert set(opt2.state[qs[0]]) == {"master", "momentum_buffer", "ema"}
    for p, q in zip(ps, qs):
        for k, v in opt.state[p].items():
            got = opt2.state[q][k]
            assert got.dtype == torch.float32 and torch.equal(got, v), k
    for k, v in sd["state"][0].items():   # copies, not the dict's tensors
        assert opt2.state[qs[0]][k].data_ptr() != v.data_ptr()


def test_state_dict_carries_the_averages():
    ps = _params(4)
    opt = FusedSGD(ps, lr=LR, momentum=MU, ema_decay=D)
    for p, g in zip(ps, _grads(40)):
        p.grad = g
    opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert sd["param_groups"][0]["ema_decay"] == D
    qs = _params(4)
    opt2 = FusedSGD(qs, lr=LR, momentum=MU, ema_decay=D)
    opt2.load_state_dict(sd)
    for p, q in zip(ps, qs):
        assert torch.equal(opt.state[p]["ema"], opt2.state[q]["ema"])


def test_config_and_validation():
    assert TrainConfig().ema_decay == 0.0
    assert TrainConfig(ema_decay=0.999).ema_decay == 0.999
    parser = add_common_args(argparse.ArgumentParser())
    assert config_from_args(parser.parse_args([])).ema_decay == 0.0
    cfg = config_from_args(parser.parse_args(["--ema_decay", "0.9998"]))
    assert cfg.ema_decay == 0.9998
    p = nn.Parameter(torch.zeros(2))
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="ema_decay"):
            TrainConfig(ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            FusedSGD([p], lr=0.1, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            config_from_args(parser.parse_args(["--ema_decay", str(bad)]))
    opt = FusedSGD([p], lr=0.1)
    with pytest.raises(ValueError, match="track_buffers"):
        opt.track_buffers([(torch.zeros(2), torch.zeros(3))])
    with pytest.raises(ValueError, match="track_buffers"):
        opt.track_buffers([(torch.zeros(2), torch.zeros(2).double())])


# ---- 8. fit -------------------------------------------------------------------

def _fit_records(tmp_path, **kw):
    from mi355x_ddp.core.engine import fit
    from mi355x_ddp.core.worker import build_training, init_seeds
    from mi355x_ddp.data import build_loaders

    init_seeds(0)
    device = torch.device("cpu")
    cfg = TrainConfig(batch_size=8, epochs=2, num_workers=0, log_interval=1,
                      synthetic=True, lr=0.05, stall_dump_s=None,
                      max_train_steps=3, max_eval_steps=1,
                      metrics_dir=str(tmp_path / "runs"),
                      ckpt_dir=str(tmp_path / "ckpts"), **kw)
    built = build_training(cfg, device, 1, 0, distributed=True, wrap="flat")
    assert len(built) == 5
    model, crit, opt, sched, scaler = built
    train_loader, test_loader, sampler = build_loaders(
        cfg, 1, 0, distributed=False)
    fit(model, train_loader, test_loader, sampler, crit, opt, sched, cfg,
        device, scaler=scaler)
    with open(tmp_path / "runs" / "metrics.jsonl") as f:
        records = [json.loads(line) for line in f]
    return cfg, model, opt, records


def test_fit_evaluates_the_averaged_weights(tmp_path):
    cfg, model, opt, records = _fit_records(tmp_path, ema_decay=D)
    ema = opt.weight_ema
    assert isinstance(ema, WeightEMA)
    assert opt.param_groups[0]["ema_decay"] == D
    vals = [r for r in records if r["kind"] == "val"]
    assert len(vals) == 2
    assert all(r["weights"] == "ema" for r in vals)
    # the model holds its own weights again, not the averages
    for p in model.parameters():
        assert not torch.equal(opt.state[p]["ema"], p.detach())
    state = torch.load(tmp_path / "ckpts" / f"{cfg.arch}_final.pt",
                       weights_only=False)
    _assert_same(dict(state["ema"]), dict(ema.state_dict()))
    from mi355x_ddp.models import build_model
    build_model(cfg.arch, cfg.num_classes).load_state_dict(state["ema"])


def test_fit_without_ema_is_as_before(tmp_path):
    cfg, model, opt, records = _fit_records(tmp_path)
    assert not hasattr(opt, "weight_ema")
    vals = [r for r in records if r["kind"] == "val"]
    assert len(vals) == 2
    for r in vals:
        assert set(r) == {"kind", "epoch", "loss", "acc1", "acc5", "ts"}
    state = torch.load(tmp_path / "ckpts" / f"{cfg.arch}_final.pt",
                       weights_only=False)
    assert "ema" not in state
