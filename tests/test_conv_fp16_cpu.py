"""fp16 conv weight shadows and dtype-keyed autotune choices, through the
torch fallbacks (no GPU needed)."""
import pytest
import torch
import torch.nn as nn

from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import (WeightShadow, _shadow_for, rotate_wT,
                                 shadow_of)
from mi355x_ddp.ops.sgd import fused_sgd_step


def _weight(K=6, C=5, R=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(K, C, R, R, generator=g)
    return nn.Parameter(w.contiguous(memory_format=torch.channels_last))


def _rotated(w16):
    """Definition of the rotated filter, element by element."""
    K, C, R, S = w16.shape
    ref = torch.empty(C, R, S, K, dtype=w16.dtype)
    for i in range(R):
        for j in range(S):
            ref[:, i, j, :] = w16[:, :, R - 1 - i, S - 1 - j].t()
    return ref


def test_fp16_shadow_refresh_through_the_fallback():
    w = _weight()
    sh = WeightShadow(w, dtype=torch.float16)
    assert sh.dtype == torch.float16
    assert sh.w16.dtype == torch.float16 and sh.wT.dtype == torch.float16
    assert sh.matches(w) and not sh.fresh(w)
    sh.refresh(w)
    assert sh.fresh(w) and sh.refreshes == 1
    assert torch.equal(sh.w16, w.detach().half())
    assert sh.w16.stride() == w.stride()
    assert torch.equal(sh.wT, _rotated(w.detach().half()))
    assert torch.equal(sh.wT, rotate_wT(w.detach().half()))
    sh.check(w)
    # fp16 and bf16 round differently: the check tells them apart
    with torch.no_grad():
        sh.w16.copy_(w.detach().bfloat16())
    with pytest.raises(RuntimeError, match="float16"):
        sh.check(w)


def test_one_argument_shadow_is_bf16():
    w = _weight()
    sh = WeightShadow(w)
    assert sh.dtype == torch.bfloat16 and sh.w16.dtype == torch.bfloat16
    assert _shadow_for(_weight(seed=1)).dtype == torch.bfloat16


def test_shadow_dtype_must_be_16bit():
    with pytest.raises(ValueError):
        WeightShadow(_weight(), dtype=torch.float32)


def test_shadow_for_replaces_a_shadow_of_the_other_dtype():
    w = _weight()
    b = _shadow_for(w, torch.bfloat16)
    assert _shadow_for(w, torch.bfloat16) is b
    h = _shadow_for(w, torch.float16)
    assert h is not b and shadow_of(w) is h
    assert h.dtype == torch.float16 and h.w16.dtype == torch.float16
    assert h.fresh(w) and h.refreshes == 1
    assert torch.equal(h.w16, w.detach().half())
    assert _shadow_for(w, torch.float16) is h and h.refreshes == 1
    b2 = _shadow_for(w, torch.bfloat16)
    assert b2 is not h and b2.w16.dtype == torch.bfloat16
    assert torch.equal(b2.wT, rotate_wT(w.detach().bfloat16()))


def test_cpu_sgd_step_invalidates_an_fp16_shadow():
    w = _weight()
    sh = _shadow_for(w, torch.float16)
    assert sh.fresh(w)
    g = torch.ones_like(w)
    with torch.no_grad():
        fused_sgd_step([w], [g], None, lr=0.1, momentum=0.0,
                       weight_decay=0.0, shadows=[sh])
    assert not sh.fresh(w)
    assert _shadow_for(w, torch.float16) is sh and sh.refreshes == 2
    assert torch.equal(sh.w16, w.detach().half())


def test_autotune_keys_differ_by_dtype(monkeypatch):
    """A choice cached for bf16 is not replayed for fp16: keys built the way
    _ConvIGEMM builds them differ in the dtype alone."""
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    shapes = (torch.Size((8, 64, 32, 32)), torch.Size((64, 64, 3, 3)), 1, 1)
    kb = convmod._tune_key("fwd", torch.bfloat16, *shapes)
    kh = convmod._tune_key("fwd", torch.float16, *shapes)
    assert kb != kh and kb[0] == kh[0] and kb[2:] == kh[2:]
    assert kb[1] is torch.bfloat16 and kh[1] is torch.float16
    monkeypatch.setitem(convmod._TUNE_CACHE, kb, 128)
    run = lambda c: None   # noqa: E731 (never measured: autotune is off)
    assert convmod._tuned_choice(kb, (64, 128), run, default=0) == 128
    assert convmod._tuned_choice(kh, (64, 128), run, default=0) == 0
    monkeypatch.setitem(convmod._TUNE_CACHE, kh, 64)
    assert convmod._tuned_choice(kh, (64, 128), run, default=0) == 64
    assert convmod._tuned_choice(kb, (64, 128), run, default=0) == 128
    report = convmod.tune_report()
    assert "bfloat16" in report and " float16" in report


def test_fp16_switch_only_touches_fp16(monkeypatch):
    assert convmod.native_conv_fp16_wanted()
    monkeypatch.setenv("MI355X_NATIVE_CONV_FP16", "0")
    assert not convmod.native_conv_fp16_wanted()
    assert convmod.native_conv_wanted()
