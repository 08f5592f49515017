"""The fused evaluation forward without a GPU: `fold_bn` against float64, the
`fused_inference` context manager (set / restore, exception, nesting,
wrappers, DataParallel), the torch definition of `conv_bn_act` through every
arch of the zoo against the float64 model, and the plumbing (`--fused_eval`,
`TrainConfig.fused_eval`, `validate`, `tools/bench_eval.py`).

Tolerances. `fold_bn` is four fp32 operations per channel on inputs of order
one (each rounding at most 6e-8 relative): 1e-6 relative to the largest table
entry holds with an order of magnitude to spare. The fp32 logits of either
path measured 1.1e-7 to 2.0e-7 relative Frobenius error against the float64
model; the bound is 1e-5.
"""
import os
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn as nn

from mi355x_ddp.config import (TrainConfig, add_common_args,
                               config_from_args)
from mi355x_ddp.core import inference
from mi355x_ddp.core.inference import folded_modules, fused_inference
from mi355x_ddp.models import build_model
from mi355x_ddp.models.resnet import _FACTORIES, conv_bn_pairs
from mi355x_ddp.ops import fused_eval
from mi355x_ddp.ops.batchnorm import MI355SyncBatchNorm
from mi355x_ddp.ops.conv import MI355Conv2d
from mi355x_ddp.ops.fused_eval import FOLDED_ATTR, conv_bn_act, fold_bn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# convs (= BatchNorms = conv_bn calls) of one forward
N_PAIRS = {"resnet18": 20, "resnet34": 36, "resnet50": 53, "resnet101": 104,
           "resnet152": 155, "resnet18_imagenet": 20, "resnet50_imagenet": 53}


def _randomize_bn(model, seed=7):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
                m.weight.copy_(0.5 + 0.5 * torch.rand(c, generator=g))
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return model


def _model(arch="resnet18", classes=10):
    torch.manual_seed(0)
    return _randomize_bn(MI355Conv2d.convert(build_model(arch, classes)))


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# ---- fold_bn ----------------------------------------------------------------------

def _bn(kind, c=24):
    g = torch.Generator().manual_seed(3)
    eps = 1e-3 if kind == "eps" else 1e-5
    bn = MI355SyncBatchNorm(c, eps=eps) if kind == "sync" \
        else nn.BatchNorm2d(c, eps=eps)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(0.05 + torch.rand(c, generator=g) * 2)
        bn.weight.copy_(torch.randn(c, generator=g))
        bn.bias.copy_(torch.randn(c, generator=g))
    if kind == "bf16_affine":   # bf16_o2: parameters bf16, statistics too
        bn = bn.bfloat16()
    return bn.eval()


@pytest.mark.parametrize("kind", ["plain", "sync", "bf16_affine", "eps"])
def test_fold_bn_against_float64(kind):
    bn = _bn(kind)
    t = fold_bn(bn)
    assert t.dtype == torch.float32 and t.shape == (4, 24)
    assert t.is_contiguous()
    invstd = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
    scale = bn.weight.detach().double() * invstd
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    for row, want in ((0, bn.running_mean.double()), (1, invstd), (2, scale),
                      (3, shift)):
        err = float((t[row].double() - want).abs().max() / want.abs().max())
        assert err <= 1e-6, (kind, row, err)
    # the module is left alone
    assert not hasattr(bn, FOLDED_ATTR)


def test_fold_bn_refuses_what_it_cannot_fold():
    with pytest.raises(ValueError, match="running statistics"):
        fold_bn(nn.BatchNorm2d(8, track_running_stats=False).eval())
    with pytest.raises(ValueError, match="eval mode"):
        fold_bn(nn.BatchNorm2d(8).train())
    with pytest.raises(TypeError):
        fold_bn(nn.Conv2d(3, 8, 3))


def test_fold_bn_without_affine():
    bn = nn.BatchNorm2d(8, affine=False).eval()
    bn.running_var.fill_(4.0)
    bn.running_mean.fill_(2.0)
    t = fold_bn(bn)
    assert torch.allclose(t[2], torch.full((8,), 0.5), atol=1e-5)
    assert torch.allclose(t[3], torch.full((8,), -1.0), atol=1e-5)


# ---- conv_bn_act, the torch definition ---------------------------------------------

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("has_res", [False, True])
def test_conv_bn_act_cpu_definition(relu, has_res):
    g = torch.Generator().manual_seed(5)
    conv = MI355Conv2d(6, 24, 3, stride=2, padding=1, bias=False)
    bn = _bn("plain")
    x = torch.randn(2, 6, 9, 9, generator=g)
    res = torch.randn(2, 24, 5, 5, generator=g) if has_res else None
    got = conv_bn_act(x, conv, fold_bn(bn), relu, res)
    want = bn.double()(conv.double()(x.double()))
    if has_res:
        want = want + res.double()
    if relu:
        want = torch.relu(want)
    assert got.dtype == torch.float32 and not got.requires_grad
    err = float((got.double() - want).norm() / want.norm())
    assert err <= 1e-6, err


# ---- the context manager -------------------------------------------------------------

def test_context_sets_and_restores():
    model = _model().eval()
    before = _state(model)
    assert len(list(conv_bn_pairs(model))) == 20
    with fused_inference(model) as m:
        assert m is model
        mods = folded_modules(model)
        assert len(mods) == 20
        assert all(isinstance(b, nn.BatchNorm2d) for b in mods)
        assert set(model.state_dict()) == set(before)   # no new keys
    assert folded_modules(model) == []
    assert not model.training
    after = _state(model)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


def test_context_restores_on_exception():
    model = _model().eval()
    with pytest.raises(RuntimeError, match="boom"):
        with fused_inference(model):
            assert len(folded_modules(model)) == 20
            raise RuntimeError("boom")
    assert folded_modules(model) == []
    with fused_inference(model):   # usable again
        assert len(folded_modules(model)) == 20
    assert folded_modules(model) == []


def test_nested_use_is_one_fold(monkeypatch):
    model = _model().eval()
    n = []
    real = inference.fold_bn
    monkeypatch.setattr(inference, "fold_bn",
                        lambda bn: (n.append(1), real(bn))[1])
    with fused_inference(model):
        tables = [getattr(b, FOLDED_ATTR) for b in folded_modules(model)]
        with fused_inference(model):
            assert len(n) == 20
            assert all(getattr(b, FOLDED_ATTR) is t
                       for b, t in zip(folded_modules(model), tables))
        assert len(folded_modules(model)) == 20   # the inner exit keeps them
    assert folded_modules(model) == [] and len(n) == 20


def test_training_bn_is_not_folded_and_mode_is_kept():
    model = _model()
    model.train()
    with fused_inference(model):
        assert folded_modules(model) == [] and model.training
    model.eval()
    model.layer1[0].bn1.train()
    with fused_inference(model):
        assert len(folded_modules(model)) == 19
        assert model.layer1[0].bn1.training and not model.training
    assert model.layer1[0].bn1.training and not model.training
    # a BN that went to training inside the context runs unfolded
    model.eval()
    x = torch.randn(4, 3, 16, 16)
    with torch.no_grad(), fused_inference(model):
        model.train()
        fused_eval.calls.reset()
        model(x)
        assert fused_eval.calls.fallback == 0
    model.eval()


def test_unwraps_flat_ddp_and_torch_ddp(tmp_path):
    import torch.distributed as dist
    from mi355x_ddp.parallel import FlatDDP, wrap_torch_ddp

    model = _model().eval()
    flat = FlatDDP(model)
    flat.eval()
    with fused_inference(flat) as m:
        assert m is flat and len(folded_modules(model)) == 20
    assert folded_modules(model) == []

    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        ddp = wrap_torch_ddp(_model(), None).eval()
        with fused_inference(ddp):
            assert len(folded_modules(ddp.module)) == 20
        assert folded_modules(ddp) == []
    finally:
        dist.destroy_process_group()


def test_data_parallel_is_a_noop_with_one_warning(monkeypatch):
    monkeypatch.setattr(inference, "_warned_dp", False)
    dp = nn.DataParallel(_model().eval())
    with pytest.warns(UserWarning, match="DataParallel"):
        with fused_inference(dp) as m:
            assert m is dp and folded_modules(dp) == []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with fused_inference(dp):
            assert folded_modules(dp) == []


# ---- every arch against float64 -------------------------------------------------------

@pytest.mark.parametrize("arch", sorted(_FACTORIES))
def test_cpu_logits_against_float64(arch):
    assert set(N_PAIRS) == set(_FACTORIES)
    model = _model(arch).eval()
    size = 32 if arch.endswith("imagenet") else 16
    x = torch.randn(2, 3, size, size,
                    generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        plain = model(x)
        fused_eval.calls.reset()
        with fused_inference(model):
            fused = model(x)
        assert fused_eval.calls.fallback == N_PAIRS[arch]
        assert fused_eval.calls.fused == fused_eval.calls.unfused == 0
        ref = model.double()(x.double())
    assert torch.isfinite(ref).all() and float(ref.norm()) > 0
    e_plain = float((plain.double() - ref).norm() / ref.norm())
    e_fused = float((fused.double() - ref).norm() / ref.norm())
    print(f"{arch}: unfused {e_plain:.2e} fused {e_fused:.2e}")
    assert e_plain <= 1e-5 and e_fused <= 1e-5, (e_plain, e_fused)
    # the two paths are different arithmetic: equal bits would mean the
    # context did nothing
    assert not torch.equal(plain, fused)


# ---- plumbing -------------------------------------------------------------------------

def test_flag_and_config():
    import argparse
    p = add_common_args(argparse.ArgumentParser())
    assert TrainConfig().fused_eval is False
    assert config_from_args(p.parse_args([])).fused_eval is False
    assert config_from_args(p.parse_args(["--fused_eval"])).fused_eval is True
    assert config_from_args(p.parse_args(["--fused-eval"])).fused_eval is True
    assert TrainConfig(fused_eval=True).replace(lr=0.2).fused_eval is True


def _tiny_eval(cfg):
    from mi355x_ddp.core.worker import build_training, init_seeds
    from mi355x_ddp.data import build_loaders

    init_seeds(0)
    model, crit, _, _, _ = build_training(cfg, torch.device("cpu"), 1, 0,
                                          distributed=True, wrap="flat")
    _randomize_bn(model)
    _, test_loader, _ = build_loaders(cfg, 1, 0, distributed=False)
    return model, crit, test_loader


@pytest.mark.parametrize("asked", [False, True])
def test_validate_enters_the_context_only_when_asked(asked, monkeypatch,
                                                     tmp_path):
    import contextlib
    from mi355x_ddp.core import engine
    from mi355x_ddp.core.metrics import JsonlSink

    cfg = TrainConfig(batch_size=16, num_workers=0, log_interval=100,
                      synthetic=True, max_eval_steps=2, fused_eval=asked,
                      metrics_dir=str(tmp_path))
    model, crit, loader = _tiny_eval(cfg)
    seen = []

    @contextlib.contextmanager
    def spy(m):
        with fused_inference(m):
            seen.append(len(folded_modules(m)))
            yield m

    monkeypatch.setattr(engine, "fused_inference", spy)
    model.train()
    fused_eval.calls.reset()
    sink = JsonlSink(cfg.metrics_dir, enabled=True)
    acc = engine.validate(model, loader, crit, torch.device("cpu"), cfg,
                          sink=sink, epoch=3)
    assert 0.0 <= acc <= 100.0
    assert seen == ([20] if asked else [])   # entered after model.eval()
    assert fused_eval.calls.fallback == (40 if asked else 0)
    assert folded_modules(model) == []
    import json
    rec = [json.loads(line) for line in open(sink.path)]
    val = [r for r in rec if r.get("kind") == "val"]
    assert len(val) == 1
    assert {"kind", "epoch", "loss", "acc1", "acc5"} <= set(val[0])
    assert "weights" not in val[0] and val[0]["epoch"] == 3


def test_bench_eval_arguments_and_no_gpu():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import bench_eval
    finally:
        sys.path.pop(0)
    args = bench_eval.parse_args([])
    assert args.configs == ["r18-bf16", "r18-fp16", "r50-bf16", "r50-fp16",
                            "r50i-bf16"]
    assert bench_eval.CONFIGS["r50i-bf16"] == ("resnet50_imagenet", 224, 64,
                                               "bf16")
    assert bench_eval.CONFIGS["r18-fp16"] == ("resnet18", 32, 256, "fp16")
    args = bench_eval.parse_args(["--configs", "r50-fp16", "--steps", "3",
                                  "--repeats", "2"])
    assert (args.configs, args.steps, args.repeats) == (["r50-fp16"], 3, 2)
    with pytest.raises(SystemExit):
        bench_eval.parse_args(["--configs", "resnet9"])
    if torch.cuda.is_available():
        return   # the measuring path is for tools runs, not for the suite
    r = subprocess.run([sys.executable,
                        os.path.join(REPO, "tools", "bench_eval.py"),
                        "--configs", "r18-bf16"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "found none" in r.stderr
