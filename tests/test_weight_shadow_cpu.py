"""Conv weight shadows: the freshness stamp, through the torch fallback of
the refresh (no GPU needed).

A WeightShadow holds the bf16 copy (w16) and the rotated transposed copy (wT)
of an fp32 conv weight. It must be rewritten exactly when the weight's
(_version, data_ptr) stamp moved or it was invalidated, and never otherwise.
"""
import torch
import torch.nn as nn

from mi355x_ddp.ops.conv import (MI355Conv2d, WeightShadow, _shadow_for,
                                 invalidate_weight_shadows, rotate_wT,
                                 shadow_of)
from mi355x_ddp.ops.sgd import fused_sgd_step


def _weight(K=6, C=5, R=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(K, C, R, R, generator=g)
    return nn.Parameter(w.contiguous(memory_format=torch.channels_last))


def _assert_current(sh, w):
    w16 = w.detach().to(torch.bfloat16)
    assert torch.equal(sh.w16, w16)
    assert sh.w16.stride() == w.stride()
    K, C, R, S = w.shape
    assert sh.wT.shape == (C, R, S, K) and sh.wT.is_contiguous()
    # definition of the rotated filter, element by element
    ref = torch.empty(C, R, S, K, dtype=torch.bfloat16)
    for i in range(R):
        for j in range(S):
            ref[:, i, j, :] = w16[:, :, R - 1 - i, S - 1 - j].t()
    assert torch.equal(sh.wT, ref)
    assert torch.equal(rotate_wT(w16), ref)


def test_first_use_creates_and_fills():
    w = _weight()
    assert shadow_of(w) is None
    sh = _shadow_for(w)
    assert shadow_of(w) is sh and sh.refreshes == 1
    _assert_current(sh, w)


def test_no_refresh_when_nothing_changed():
    w = _weight()
    sh = _shadow_for(w)
    ptrs = (sh.w16.data_ptr(), sh.wT.data_ptr())
    for _ in range(5):
        assert _shadow_for(w) is sh
    assert sh.refreshes == 1
    assert (sh.w16.data_ptr(), sh.wT.data_ptr()) == ptrs


def test_version_bump_forces_refresh():
    w = _weight()
    sh = _shadow_for(w)
    ptrs = (sh.w16.data_ptr(), sh.wT.data_ptr())
    with torch.no_grad():
        w.mul_(0.5)
    assert not sh.fresh(w)
    assert _shadow_for(w) is sh and sh.refreshes == 2
    _assert_current(sh, w)
    # rewritten in place: the addresses a captured graph holds stay valid
    assert (sh.w16.data_ptr(), sh.wT.data_ptr()) == ptrs
    _shadow_for(w)
    assert sh.refreshes == 2


def test_load_state_dict_forces_refresh():
    conv = MI355Conv2d(5, 6, 3, bias=False)
    conv.weight = _weight()
    sh = _shadow_for(conv.weight)
    conv.load_state_dict({"weight": _weight(seed=1).detach()})
    assert _shadow_for(conv.weight) is sh and sh.refreshes == 2
    _assert_current(sh, conv.weight)


def test_data_ptr_change_forces_refresh():
    w = _weight()
    sh = _shadow_for(w)
    w.data = _weight(seed=2).detach().clone(
        memory_format=torch.preserve_format)
    assert not sh.fresh(w)
    assert _shadow_for(w) is sh and sh.refreshes == 2
    _assert_current(sh, w)


def test_layout_change_replaces_shadow():
    w = _weight()
    sh = _shadow_for(w)
    w.data = torch.randn(4, 5, 1, 1)
    sh2 = _shadow_for(w)
    assert sh2 is not sh and sh2.refreshes == 1
    _assert_current(sh2, w)


def test_explicit_invalidate_forces_refresh():
    conv = MI355Conv2d(5, 6, 3, bias=False)
    conv.weight = _weight()
    sh = _shadow_for(conv.weight)
    # a write the version counter cannot see
    conv.weight.data.mul_(2.0)
    assert sh.fresh(conv.weight)      # that is the problem ...
    invalidate_weight_shadows(conv)   # ... and this the remedy
    assert not sh.fresh(conv.weight)
    assert _shadow_for(conv.weight) is sh and sh.refreshes == 2
    _assert_current(sh, conv.weight)
    # the parameter and iterable forms
    invalidate_weight_shadows(conv.weight)
    _shadow_for(conv.weight)
    invalidate_weight_shadows([conv.weight])
    _shadow_for(conv.weight)
    assert sh.refreshes == 4


def test_fallback_sgd_step_never_leaves_a_stale_shadow():
    """fused_sgd_step refreshes or invalidates: after the torch-path step the
    next use rebuilds the shadow from the new weight."""
    w = _weight()
    sh = _shadow_for(w)
    g = torch.ones_like(w)
    with torch.no_grad():
        fused_sgd_step([w], [g], None, lr=0.1, momentum=0.0,
                       weight_decay=0.0, shadows=[sh])
    assert not sh.fresh(w)
    _shadow_for(w)
    assert sh.refreshes == 2
    _assert_current(sh, w)


def test_check_shadows_raises_on_stale(monkeypatch):
    monkeypatch.setenv("MI355X_CHECK_SHADOWS", "1")
    w = _weight()
    _shadow_for(w)
    w.data.mul_(3.0)   # unseen write, no invalidate
    try:
        _shadow_for(w)
    except RuntimeError as e:
        assert "stale" in str(e)
    else:
        raise AssertionError("stale shadow not detected")
