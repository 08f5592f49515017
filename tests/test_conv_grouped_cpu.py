"""Host-side logic of the grouped convolution that needs no GPU: the
`_grouped_ok` decision table, the tuner report's labels for the grouped keys,
and a self-check that the shape list of tests/test_conv_grouped_exact_gpu.py
still reaches every kernel variant of csrc/conv_grouped.hip off its first
tile."""
import importlib.util
import os

import pytest
import torch

from mi355x_ddp.ops import _backend
from mi355x_ddp.ops import conv as convmod
from mi355x_ddp.ops.conv import MIOPEN, _grouped_ok

CL = torch.channels_last
BF, HALF = torch.bfloat16, torch.float16


def _exact_module():
    """The GPU test module, loaded by path: it holds the shape list and the
    plain-Python mirror of the host dispatch."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "test_conv_grouped_exact_gpu.py")
    spec = importlib.util.spec_from_file_location("_grouped_exact", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- _grouped_ok -------------------------------------------------------------

def _ok(C=64, Cg=8, K=None, k=3, dt=BF, wdt=None, nchw=False, stride=(1, 1),
        padding=(1, 1), dilation=(1, 1), groups=None):
    x = torch.zeros(2, C, 8, 8, dtype=dt)
    if not nchw:
        x = x.contiguous(memory_format=CL)
    w = torch.zeros(K or C, Cg, k, k, dtype=wdt or dt).contiguous(
        memory_format=CL)
    return _grouped_ok(x, w, stride, padding, dilation,
                       groups if groups is not None else C // Cg)


@pytest.fixture
def native(monkeypatch):
    monkeypatch.setattr(_backend, "native_enabled", lambda t=None: True)
    for name in ("MI355X_NATIVE_GROUPED", "MI355X_NATIVE_CONV",
                 "MI355X_NATIVE_CONV_FP16"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_grouped_ok_takes_the_supported_convs(native):
    assert _ok() is True                      # the baseline of the table below
    assert _ok(stride=(2, 2)) is True
    assert _ok(dt=HALF) is True
    for cg in (4, 16, 32):
        assert _ok(Cg=cg) is True
    assert _ok(C=128, Cg=64) is True


@pytest.mark.parametrize("deviation", [
    dict(Cg=64, groups=1),                    # groups 1: the dense kernels'
    dict(Cg=2),
    dict(C=256, Cg=128),
    dict(C=16, Cg=4),                         # C no multiple of the pack width
    dict(K=128),                              # out_channels != in_channels
    dict(k=1),
    dict(k=5),
    dict(padding=(0, 0)),
    dict(dilation=(2, 2)),
    dict(stride=(3, 3)),
    dict(stride=(1, 2)),
    dict(nchw=True),
    dict(wdt=torch.float32),
    dict(wdt=HALF),                           # mixed 16-bit dtypes
    dict(dt=HALF, wdt=BF),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()).replace(
    "torch.", ""))
def test_grouped_ok_refuses_each_single_deviation(native, deviation):
    assert _ok() is True
    assert _ok(**deviation) is False


def test_grouped_ok_switches(native):
    native.setenv("MI355X_NATIVE_GROUPED", "0")
    assert _ok() is False
    native.setenv("MI355X_NATIVE_GROUPED", "1")
    native.setenv("MI355X_NATIVE_CONV_FP16", "0")
    assert _ok(dt=HALF) is False
    assert _ok() is True                      # bf16 is not that switch's
    native.setenv("MI355X_NATIVE_CONV_FP16", "1")
    native.setenv("MI355X_NATIVE_CONV", "0")
    assert _ok() is False


def test_grouped_ok_is_false_off_the_gpu():
    assert _ok() is False                     # CPU tensors, nothing patched


# ---- tune_report -------------------------------------------------------------

def test_tune_report_labels_the_grouped_keys(monkeypatch):
    xs, ws = torch.Size((2, 64, 12, 12)), torch.Size((64, 8, 3, 3))
    cache = {
        ("g_fwd", BF, xs, ws, 8, 1): 0,
        ("g_fwd", HALF, xs, ws, 8, 1): MIOPEN,
        ("g_dgrad", BF, xs, xs, 8, 1): 0,
        ("g_dgrad", HALF, xs, xs, 8, 1): MIOPEN,
        ("g_wgrad", BF, xs, xs, 8, 1): ("splits", 0),
        ("g_wgrad", BF, xs, xs, 8, 2): ("splits", 32),
        ("g_wgrad", HALF, xs, xs, 8, 1): MIOPEN,
    }
    monkeypatch.setattr(convmod, "_TUNE_CACHE", cache)
    lines = convmod.tune_report().splitlines()
    assert len(lines) == len(cache)

    def label(kind, dt, stride=1):
        hit = [ln for ln in lines
               if ln.split()[0] == kind and ln.split()[1] == dt and
               f"8, {stride})" in ln]
        assert len(hit) == 1, (kind, dt, stride, lines)
        return hit[0].split("-> ")[1]

    assert label("g_fwd", "bfloat16") == "native grouped"
    assert label("g_fwd", "float16") == "MIOpen"
    assert label("g_dgrad", "bfloat16") == "native grouped"
    assert label("g_dgrad", "float16") == "MIOpen"
    assert label("g_wgrad", "bfloat16") == "native grouped, splits auto"
    assert label("g_wgrad", "bfloat16", 2) == "native grouped, splits 32"
    assert label("g_wgrad", "float16") == "MIOpen"


# ---- the exact tests' shape list against the host dispatch --------------------

FWD_DGRAD_VARIANTS = [          # conv_grouped_kernel<T, P, S, TH, ZINS>
    (32, 1, 8, False), (32, 2, 8, False), (32, 1, 8, True),
    (64, 1, 8, False), (64, 2, 4, False), (64, 1, 8, True)]
WGRAD_VARIANTS = [(32, 1), (32, 2), (64, 1), (64, 2)]


def test_dispatch_mirror_on_known_shapes():
    d = _exact_module().grouped_dispatch((2, 128, 18, 35, 2, 2))
    assert d["fwd"]["variant"] == (64, 2, 4, False)
    assert (d["fwd"]["tiles_h"], d["fwd"]["tiles_w"]) == (3, 2)
    assert d["dgrad"]["variant"] == (64, 1, 8, True)
    assert (d["dgrad"]["tiles_h"], d["dgrad"]["tiles_w"]) == (3, 3)
    assert d["wgrad"]["variant"] == (64, 2)
    assert (d["wgrad"]["tiles_h"], d["wgrad"]["tiles_w"]) == (2, 2)
    assert d["fwd"]["packs"] == 2 and d["fwd"]["N"] == 2
    d = _exact_module().grouped_dispatch((2, 32, 20, 36, 8, 1))
    assert d["fwd"]["variant"] == d["dgrad"]["variant"] == (32, 1, 8, False)
    assert (d["wgrad"]["tiles_h"], d["wgrad"]["tiles_w"]) == (3, 3)


def test_exact_shapes_reach_every_variant_off_the_first_tile():
    mod = _exact_module()
    reached = {}
    some_packs = some_images = False
    for shape in mod.EXACT_SHAPES:
        for p in mod.grouped_dispatch(shape).values():
            eh, ew = p["extent"]
            if p["tiles_h"] > 1 and p["tiles_w"] > 1 and \
                    eh % p["TH"] != 0 and ew % 16 != 0:
                reached.setdefault(p["variant"], []).append(shape)
                some_packs |= p["packs"] > 1
                some_images |= p["N"] > 1
    for v in FWD_DGRAD_VARIANTS + WGRAD_VARIANTS:
        print(v, "reached off the first tile, ragged, by", reached.get(v))
    missing = [v for v in FWD_DGRAD_VARIANTS + WGRAD_VARIANTS
               if v not in reached]
    assert not missing, f"no multi-tile ragged shape launches {missing}"
    assert some_packs and some_images
    # the wgrad split test needs more tiles than its largest inner split
    for shape in mod.SPLIT_SHAPES:
        p = mod.grouped_dispatch(shape)["wgrad"]
        assert p["N"] * p["tiles_h"] * p["tiles_w"] > 7
        assert p["tiles_h"] * p["tiles_w"] > 1
    assert {mod.grouped_dispatch(s)["wgrad"]["variant"]
            for s in mod.SPLIT_SHAPES} >= {(32, 1), (64, 2)}
    assert {max(s[1] // s[4], 32) for s in mod.RANGE_SHAPES} == {32, 64}
