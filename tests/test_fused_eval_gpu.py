"""The fused evaluation forward on the GPU (MI355X): the BN-epilogue
instantiations of the forward conv kernels and of the split-K reduce
(`conv_fwd_bn_igemm`), `conv_bn_act` with its tuner, `fused_inference` on
ResNet-18/50, under a weight-EMA swap, through `validate`, and the per-layer
fallback of fp32 and NCHW models.

Exact checks. Four fold tables make the epilogue free of rounding, so
`torch.equal` applies: the identity (scale 1, shift 0) must give the plain
kernel's bits at the same tile and splits, with relu its `torch.relu`;
scale 0 and shift 0 must return the residual; scale 0 and shift[k] = k % 64
(exact in both formats) must return that value in every pixel of channel k.
Together they pin row, column and residual indexing on every edge tile, in
the direct kernels and in the reduce.

Parity. As in test_conv_fp16_gpu.py: against the fp32 CPU composition of the
same 16-bit-rounded operands, relative Frobenius error, bounds 4e-3 (bf16) and
5e-4 (fp16). The reference's own rounding to the output format on these
shapes is at most 1.74e-3 (bf16) and 2.13e-4 (fp16).

Model level. Fused and unfused logits are each compared with the fp32 CPU
model on the same inputs; `e_fused <= 1.5 * e_unfused`. The fused path drops
one rounding per layer, so it should be no worse; a CPU emulation gave ratios
of 0.96 to 1.06, with e about 2-3e-3 (bf16) and 3e-4 (fp16), and an indexing
or folding bug gives O(1). BatchNorm statistics and affine parameters are
randomized: a fresh model folds to the identity and would show nothing.

Measured on an MI355X. Parity over all cases: bf16 1.62e-3 to 1.69e-3 (the
split-K reduce at most 1.69e-3), fp16 1.99e-4 to 2.15e-4 (split-K 2.10e-4).
Model level, e_unfused / e_fused: resnet18 bf16 4.16e-3 / 4.14e-3, fp16
5.51e-4 / 4.97e-4; resnet50 bf16 4.72e-3 / 4.59e-3, fp16 5.76e-4 / 5.49e-4
(ratios 0.90 to 1.00). Under the EMA swap 2.08e-3 / 2.05e-3.
"""
import copy
import functools
import json
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from mi355x_ddp.core.inference import folded_modules, fused_inference
from mi355x_ddp.models import build_model
from mi355x_ddp.ops import conv as conv_ops
from mi355x_ddp.ops import fused_eval
from mi355x_ddp.ops.conv import (MI355Conv2d, TILE_128X128, UNFUSED,
                                 shadow_of, splitk_candidates)
from mi355x_ddp.ops.fused_eval import conv_bn_act
from mi355x_ddp.ops.pool import MI355MaxPool2d

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}
DTYPES = [torch.bfloat16, torch.float16]
AMP = {torch.bfloat16: "bf16", torch.float16: "fp16"}

# (N, C, H, W, K, R, stride, pad): each the smallest that reaches its path
SHAPES = [
    (2, 64, 8, 8, 64, 3, 1, 1),      # FAST, M = 128 exactly
    (3, 64, 10, 10, 128, 3, 2, 1),   # stride 2, ragged M = 75
    (2, 32, 6, 6, 48, 3, 1, 1),      # generic gather, ragged M, part N tile
    (2, 3, 10, 10, 64, 3, 1, 1),     # PADC stem, ragged
    (2, 3, 16, 16, 64, 7, 2, 3),     # 7x7 stem
    (2, 128, 8, 8, 256, 1, 1, 0),    # 1x1, 128-wide N tile
    (2, 64, 8, 8, 100, 3, 1, 1),     # N = 100: N % 8 != 0, >= 96 for 228
    (3, 256, 8, 8, 256, 3, 1, 1),    # split-K, ragged M = 192, 36 K-tiles
]
SPLITK = SHAPES[7]


def _takes_228(shape):
    return shape[1] % 64 == 0 and shape[4] >= 96


# (tile, splits); splits 2 and 4 where the 128x128 tile applies
CASES = [(s, t, 1) for s in SHAPES for t in (0, 64, 128, 228)] + \
        [(s, 228, z) for s in SHAPES if _takes_228(s) for z in (2, 4)]


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, tuple):
        return "x".join(str(i) for i in
                        (v[0] + v[1:] if isinstance(v[0], tuple) else v))
    return None


def _C():
    from mi355x_ddp import _C
    return _C


def _table(scale, shift):
    """fp32 [4][K] as fold_bn lays it out; the kernels read rows 2 and 3."""
    z = torch.zeros_like(scale)
    return torch.stack([z, z, scale, shift]).contiguous().to(DEV)


class _Case:
    """Rounded operands on the GPU, a random fold and the fp32 CPU reference
    of the conv. Built once per (shape, dtype) and never written to."""

    def __init__(self, shape, dt):
        N, C, H, W, K, R, stride, pad = shape
        g = torch.Generator().manual_seed(4321 + sum(shape))
        x = torch.randn(N, C, H, W, generator=g).to(dt)
        w = (torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5).to(dt)
        self.y = F.conv2d(x.float(), w.float(), None, stride, pad)
        res = torch.randn(self.y.shape, generator=g).to(dt)
        gamma = 0.5 + torch.rand(K, generator=g)
        beta = torch.randn(K, generator=g) * 0.5
        mean = torch.randn(K, generator=g) * 0.5
        var = 0.25 + torch.rand(K, generator=g)
        self.scale = gamma * torch.rsqrt(var + 1e-5)
        self.shift = beta - mean * self.scale
        self.res_cpu = res.float()
        self.x = x.to(DEV).contiguous(memory_format=CL)
        self.w = w.to(DEV).contiguous(memory_format=CL)
        self.res = res.to(DEV).contiguous(memory_format=CL)
        self.table = _table(self.scale, self.shift)
        self.K, self.stride, self.pad, self.dt = K, stride, pad, dt

    def ref(self, has_res, relu):
        v = self.y * self.scale.view(1, -1, 1, 1) + \
            self.shift.view(1, -1, 1, 1)
        if has_res:
            v = v + self.res_cpu
        return torch.relu(v) if relu else v


@functools.lru_cache(maxsize=None)
def _case(shape, dt):
    return _Case(shape, dt)


def _rel_err(got, ref):
    got = got.float().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _fused(c, table, res, relu, tile, splits):
    return _C().conv_fwd_bn_igemm(c.x, c.w, table, res, relu, c.stride, c.pad,
                                  tile, splits)


# ---- 1. exact checks ------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_exact(case, dt):
    shape, tile, splits = case
    c = _case(shape, dt)
    K = c.K
    plain = _C().conv_fwd_igemm(c.x, c.w, c.stride, c.pad, tile, splits)
    one, zero = torch.ones(K), torch.zeros(K)
    ident = _table(one, zero)
    got = _fused(c, ident, None, False, tile, splits)
    assert got.dtype == dt and got.shape == plain.shape
    assert got.is_contiguous(memory_format=CL)
    assert torch.equal(got, plain), "identity fold"
    assert torch.equal(_fused(c, ident, None, True, tile, splits),
                       torch.relu(plain)), "identity fold + relu"
    assert torch.equal(_fused(c, _table(zero, zero), c.res, False, tile,
                              splits), c.res), "residual pass-through"
    ramp = (torch.arange(K) % 64).float()
    want = ramp.to(dt).to(DEV).view(1, K, 1, 1).expand_as(plain)
    assert torch.equal(_fused(c, _table(zero, ramp), None, False, tile,
                              splits), want), "shift broadcast"


# ---- 2. parity --------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_parity(case, dt):
    shape, tile, splits = case
    c = _case(shape, dt)
    for has_res in (False, True):
        for relu in (False, True):
            got = _fused(c, c.table, c.res if has_res else None, relu, tile,
                         splits)
            err = _rel_err(got, c.ref(has_res, relu))
            print(f"fwd_bn {shape} tile {tile} splits {splits} {dt} "
                  f"res {has_res} relu {relu}: rel err {err:.3e}")
            assert err < TOL[dt], (has_res, relu, err)
            if relu:
                assert float(got.min()) >= 0.0


def test_operand_checks():
    c = _case(SHAPES[0], torch.bfloat16)
    f = _C().conv_fwd_bn_igemm
    with pytest.raises(RuntimeError, match="scale_shift"):
        f(c.x, c.w, c.table[:, :32].contiguous(), None, False, 1, 1)
    with pytest.raises(RuntimeError, match="scale_shift"):
        f(c.x, c.w, c.table[2:].contiguous(), None, False, 1, 1)
    with pytest.raises(RuntimeError, match="scale_shift"):
        f(c.x, c.w, c.table.double(), None, False, 1, 1)
    with pytest.raises(RuntimeError, match="residual"):   # shape
        f(c.x, c.w, c.table, c.res[:, :, :4], False, 1, 1)
    with pytest.raises(RuntimeError, match="residual"):   # dtype
        f(c.x, c.w, c.table, c.res.half(), False, 1, 1)
    with pytest.raises(RuntimeError, match="residual"):   # layout: NCHW
        f(c.x, c.w, c.table, c.res.contiguous(), False, 1, 1)
    assert not c.res.contiguous().is_contiguous(memory_format=CL)


# ---- 3. the tuner, one shape ---------------------------------------------------------

def _conv_module(c):
    N, C, H, W, K, R, stride, pad = SPLITK
    conv = MI355Conv2d(C, K, R, stride=stride, padding=pad, bias=False)
    conv = conv.to(DEV).to(c.dt).to(memory_format=CL)
    with torch.no_grad():
        conv.weight.copy_(c.w)
    return conv


def test_tuner_picks_a_candidate(monkeypatch):
    monkeypatch.setenv("MI355X_AUTOTUNE", "1")
    # the process-wide cache goes back to what it was
    monkeypatch.setattr(conv_ops, "_TUNE_CACHE", {})
    c = _case(SPLITK, torch.bfloat16)
    conv = _conv_module(c)
    fused_eval.calls.reset()
    got = conv_bn_act(c.x, conv, c.table, True, c.res)
    keys = [k for k in conv_ops._TUNE_CACHE if k[0] == "fwd_bn"]
    assert keys == [("fwd_bn", torch.bfloat16, c.x.shape, c.w.shape, 1, 1,
                     True)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cands = (64, 128, TILE_128X128) + splitk_candidates(
        "fwd", c.x.shape, c.w.shape, 1, 1, cus) + (UNFUSED,)
    assert (TILE_128X128, 4) in cands
    choice = conv_ops._TUNE_CACHE[keys[0]]
    assert choice in cands
    print("fwd_bn choice:", choice, "\n" + conv_ops.tune_report())
    assert "fwd_bn" in conv_ops.tune_report()
    assert fused_eval.calls.fused + fused_eval.calls.unfused == 1
    assert (fused_eval.calls.unfused == 1) == (choice == UNFUSED)
    err = _rel_err(got, c.ref(True, True))
    print(f"tuned fwd_bn: rel err {err:.3e}")
    assert err < TOL[torch.bfloat16], err
    # whatever won is replayed from the cache
    assert torch.equal(conv_bn_act(c.x, conv, c.table, True, c.res), got)


def test_unfused_candidate_meets_the_bound(monkeypatch):
    monkeypatch.setenv("MI355X_AUTOTUNE", "1")
    c = _case(SPLITK, torch.float16)
    key = ("fwd_bn", torch.float16, c.x.shape, c.w.shape, 1, 1, False)
    monkeypatch.setattr(conv_ops, "_TUNE_CACHE", {key: UNFUSED})
    fused_eval.calls.reset()
    got = conv_bn_act(c.x, _conv_module(c), c.table, False, None)
    assert fused_eval.calls.unfused == 1 and fused_eval.calls.fused == 0
    # two roundings (conv output, then BN output): twice the one-rounding
    # bound
    err = _rel_err(got, c.ref(False, False))
    assert err < 2 * TOL[torch.float16], err


# ---- 4. model level --------------------------------------------------------------------

@pytest.fixture
def no_autotune(monkeypatch):
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    return monkeypatch


N_CONVS = {"resnet18": 20, "resnet50": 53}


def _randomize_bn(model, seed=7):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                dev = m.weight.device
                m.running_mean.copy_((torch.randn(c, generator=g) * .1).to(dev))
                m.running_var.copy_(
                    (0.25 + 0.5 * torch.rand(c, generator=g)).to(dev))
                m.weight.copy_((1.0 + torch.rand(c, generator=g)).to(dev))
                m.bias.copy_((torch.randn(c, generator=g) * 0.1).to(dev))
    return model


def _images(n=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 32, 32, generator=g)


@functools.lru_cache(maxsize=None)
def _cpu_model_and_ref(arch):
    """The fp32 CPU eager model and its logits: the reference of both dtypes.
    Never written to."""
    torch.manual_seed(0)
    model = _randomize_bn(build_model(arch, 100)).eval()
    with torch.no_grad():
        return model, model(_images())


def _gpu_model(arch, fmt=CL):
    cpu, _ = _cpu_model_and_ref(arch)
    model = MI355MaxPool2d.convert(MI355Conv2d.convert(copy.deepcopy(cpu)))
    return model.to(DEV).to(memory_format=fmt).eval()


def _forward(model, x, dt):
    with torch.no_grad(), torch.autocast("cuda", dtype=dt, enabled=dt is not None):
        return model(x)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_model_logits(arch, dt, no_autotune):
    _, ref = _cpu_model_and_ref(arch)
    model = _gpu_model(arch)
    x = _images().to(DEV).contiguous(memory_format=CL)
    before = _state(model)
    unfused = _forward(model, x, dt)
    fused_eval.calls.reset()
    with fused_inference(model):
        assert len(folded_modules(model)) == N_CONVS[arch]
        fused = _forward(model, x, dt)
        assert fused_eval.calls.fused == N_CONVS[arch]
        assert fused_eval.calls.unfused == fused_eval.calls.fallback == 0
    e_u, e_f = _rel_err(unfused, ref), _rel_err(fused, ref)
    print(f"{arch} {AMP[dt]}: e_unfused {e_u:.3e} e_fused {e_f:.3e} "
          f"ratio {e_f / e_u:.3f}")
    assert e_f <= 1.5 * e_u, (e_f, e_u)
    assert folded_modules(model) == [] and not model.training
    after = _state(model)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


# ---- 5. under a weight-EMA swap -----------------------------------------------------------

D = 0.5


def _training(fused_eval_flag=True, **kw):
    from mi355x_ddp.config import TrainConfig
    from mi355x_ddp.core.worker import build_training, init_seeds

    init_seeds(0)
    cfg = TrainConfig(batch_size=8, amp="bf16", sync_bn=False,
                      channels_last=True, fused_eval=fused_eval_flag,
                      log_interval=100, **kw)
    model, crit, opt, _, _ = build_training(
        cfg, torch.device(DEV, 0), world_size=1, rank=0, distributed=True,
        wrap="flat")
    return cfg, model, crit, opt


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
    return float(loss.detach())


class _Keep(nn.Module):
    """A criterion that keeps the logits it is given."""

    def __init__(self, crit):
        super().__init__()
        self.crit, self.seen = crit, []

    def forward(self, out, target):
        self.seen.append(out.detach().clone())
        return self.crit(out, target)


def test_ema_swap_then_fused(no_autotune):
    from mi355x_ddp.core.engine import validate_with

    cfg, model, crit, opt = _training(ema_decay=D)
    for i in range(3):
        _train_step(model, crit, opt, i)
    ema = opt.weight_ema
    x, y = _batch(9)
    bf16 = torch.bfloat16
    model.eval()
    raw = _forward(model, x, bf16)
    # the fp32 CPU model of the averaged weights and statistics
    cpu = build_model("resnet18", 100)
    cpu.load_state_dict({k: v.cpu() for k, v in ema.state_dict().items()})
    with torch.no_grad():
        ref = cpu.eval()(x.cpu().contiguous())
    weights = [p.detach().clone() for p in model.parameters()]
    buffers = [b.detach().clone() for b in model.buffers()]
    with ema.swapped():
        unfused = _forward(model, x, bf16)
        with fused_inference(model):
            fused = _forward(model, x, bf16)
    e_u, e_f = _rel_err(unfused, ref), _rel_err(fused, ref)
    e_raw = _rel_err(raw, ref)
    print(f"ema swap: e_unfused {e_u:.3e} e_fused {e_f:.3e}; raw weights "
          f"against the averaged reference {e_raw:.3e}")
    assert e_f <= 1.5 * e_u, (e_f, e_u)
    assert not torch.equal(fused, raw)
    # validate_with under cfg.fused_eval: the same logits, bit for bit
    keep = _Keep(crit)
    fused_eval.calls.reset()
    validate_with(ema, model, [(x, y)], keep, torch.device(DEV, 0), cfg)
    assert fused_eval.calls.fused == 20 and len(keep.seen) == 1
    assert torch.equal(keep.seen[0], fused)
    # afterwards: weights, statistics and shadows are the model's own again
    assert folded_modules(model) == []
    for p, w in zip(model.parameters(), weights):
        assert torch.equal(p.detach(), w)
    for b, w in zip(model.buffers(), buffers):
        assert torch.equal(b, w)
    n = 0
    for p in model.parameters():
        sh = shadow_of(p)
        if sh is not None:
            sh.check(p)
            n += 1
    assert n >= 20
    assert math.isfinite(_train_step(model, crit, opt, 3))


# ---- 6. validate() ------------------------------------------------------------------------

def test_validate_counts_match_unfused(no_autotune, tmp_path):
    """Top-1 predictions of the fused and unfused runs agree on every sample
    whose top-1 / top-2 margin rules a flip out. Check 4 bounds each path's
    relative error by e_u resp. 1.5 e_u, with e_u = 3e-3 for bf16 (the
    emulation's figure). A flip needs two logits of a row to move towards
    each other by the margin, |d_a| + |d_b| <= sqrt(2) |d_row|, so with the
    error spread over the rows like the logits are, no flip happens where
        margin > sqrt(2) * 2.5 * 3e-3 * |row|.
    At most 10% of the samples may fall under that rule (seed 0 on the CPU:
    none of 32)."""
    from mi355x_ddp.core.engine import validate
    from mi355x_ddp.core.metrics import JsonlSink

    cfg, model, crit, _ = _training(fused_eval_flag=False, num_classes=10)
    _randomize_bn(model)
    g = torch.Generator().manual_seed(0)
    loader = [(torch.randn(16, 3, 32, 32, generator=g),
               torch.randint(0, 10, (16,), generator=g)) for _ in range(2)]
    dev = torch.device(DEV, 0)
    runs = {}
    for flag in (False, True):
        keep = _Keep(crit)
        sink = JsonlSink(str(tmp_path / f"fused{int(flag)}"), enabled=True)
        fused_eval.calls.reset()
        acc = validate(model, loader, keep, dev,
                       cfg.replace(fused_eval=flag), sink=sink, epoch=1)
        assert fused_eval.calls.fused == (40 if flag else 0)
        rec = [json.loads(line) for line in open(sink.path)]
        val = [r for r in rec if r["kind"] == "val"]
        assert len(val) == 1
        runs[flag] = (acc, torch.cat(keep.seen).float(), val[0])
    assert set(runs[True][2]) == set(runs[False][2])
    lu, lf = runs[False][1], runs[True][1]
    top = lu.topk(2, dim=1).values
    tau = math.sqrt(2) * 2.5 * 3e-3 * lu.norm(dim=1)
    sure = (top[:, 0] - top[:, 1]) > tau
    share = 1.0 - float(sure.float().mean())
    print(f"validate: excluded share {share:.3f}, acc1 unfused "
          f"{runs[False][0]:.3f} fused {runs[True][0]:.3f}")
    assert share <= 0.10, share
    labels = torch.cat([y for _, y in loader]).to(DEV)
    hit_u = (lu.argmax(1) == labels) & sure
    hit_f = (lf.argmax(1) == labels) & sure
    assert int(hit_u.sum()) == int(hit_f.sum())
    assert torch.equal(lu.argmax(1)[sure], lf.argmax(1)[sure])
    if bool(sure.all()):
        assert runs[True][0] == runs[False][0]


# ---- 7. fp32 and NCHW take the per-layer fallback -------------------------------------------

@pytest.mark.parametrize("kind", ["fp32", "nchw"])
def test_fallback_layers_are_bit_equal(kind, no_autotune):
    # these layers run on MIOpen, inside the context and outside it: ask it
    # for its repeatable kernels, as the exact fp32 tests of test_train_gpu.py
    # do (without that the fp32 logits inside and outside differed in their
    # last bits, from the same ops on both sides), and let its first call,
    # which picks the kernels, pass before comparing
    no_autotune.setattr(torch.backends.cudnn, "deterministic", True)
    fmt = CL if kind == "fp32" else torch.contiguous_format
    dt = None if kind == "fp32" else torch.bfloat16
    model = _gpu_model("resnet18", fmt)
    x = _images().to(DEV).contiguous(memory_format=fmt)
    first = _forward(model, x, dt)
    outside = _forward(model, x, dt)
    print(f"{kind}: first call equals the second: "
          f"{torch.equal(first, outside)}")
    fused_eval.calls.reset()
    with fused_inference(model):
        inside = _forward(model, x, dt)
    assert fused_eval.calls.fallback == 20 and fused_eval.calls.fused == 0
    assert torch.equal(inside, outside)
