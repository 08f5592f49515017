"""The tuner's split-K candidate rule for conv forward / input-grad: a plain
function of the shapes, checked here without a GPU."""
import pytest

from mi355x_ddp.ops import conv as conv_mod
from mi355x_ddp.ops.conv import splitk_candidates

CUS = 256     # MI355X
B = 256       # the benchmark's batch

# ResNet-18 / CIFAR convs: name -> (x shape, w shape, stride, pad)
R18 = {
    "stem":       ((B, 3, 32, 32), (64, 3, 3, 3), 1, 1),
    "l1 3x3":     ((B, 64, 32, 32), (64, 64, 3, 3), 1, 1),
    "l2 3x3/2":   ((B, 64, 32, 32), (128, 64, 3, 3), 2, 1),
    "l2 1x1/2":   ((B, 64, 32, 32), (128, 64, 1, 1), 2, 0),
    "l2 3x3":     ((B, 128, 16, 16), (128, 128, 3, 3), 1, 1),
    "l3 3x3/2":   ((B, 128, 16, 16), (256, 128, 3, 3), 2, 1),
    "l3 1x1/2":   ((B, 128, 16, 16), (256, 128, 1, 1), 2, 0),
    "l3 3x3":     ((B, 256, 8, 8), (256, 256, 3, 3), 1, 1),
    "l4 3x3/2":   ((B, 256, 8, 8), (512, 256, 3, 3), 2, 1),
    "l4 1x1/2":   ((B, 256, 8, 8), (512, 256, 1, 1), 2, 0),
    "l4 3x3":     ((B, 512, 4, 4), (512, 512, 3, 3), 1, 1),
}
BOTH = ((228, 2), (228, 4))


@pytest.fixture(autouse=True)
def _splitk_on(monkeypatch):
    monkeypatch.delenv("MI355X_CONV_SPLITK", raising=False)


def _cands(kind, name, cus=CUS):
    x, w, stride, pad = R18[name]
    return splitk_candidates(kind, x, w, stride, pad, cus)


@pytest.mark.parametrize("name", ["l3 3x3", "l4 3x3"])
def test_layer3_and_layer4_3x3_get_both_splits(name):
    assert _cands("fwd", name) == BOTH
    assert _cands("dgrad", name) == BOTH


@pytest.mark.parametrize("name", ["l3 3x3/2", "l4 3x3/2"])
def test_stride2_3x3_forward_only(name):
    """The stride-2 input-grad with even H, W is the parity kernels'."""
    assert _cands("fwd", name) == BOTH
    assert _cands("dgrad", name) == ()


@pytest.mark.parametrize("name", ["stem", "l1 3x3", "l2 3x3/2", "l2 1x1/2",
                                  "l2 3x3", "l3 1x1/2", "l4 1x1/2"])
def test_no_split_for_layer1_layer2_and_1x1(name):
    assert _cands("fwd", name) == ()
    assert _cands("dgrad", name) == ()


def test_rule_follows_the_cu_count_and_the_slice_length():
    # layer3 3x3 is 128 x 2 = 256 tiles of 128x128: one CU fewer, no split
    assert _cands("fwd", "l3 3x3", cus=255) == ()
    assert _cands("fwd", "l3 3x3", cus=256) == BOTH
    # 8 K-tiles: two slices of 4 qualify, four slices of 2 do not
    assert splitk_candidates("fwd", (B, 512, 4, 4), (512, 512, 1, 1), 1, 0,
                             CUS) == ((228, 2),)
    # odd H, W with stride 2: not the parity path, so dgrad may split
    assert splitk_candidates("dgrad", (B, 256, 7, 7), (512, 256, 3, 3), 2, 1,
                             CUS) == BOTH
    # gathered channels not a multiple of 64 (not FAST), or N < 96
    assert splitk_candidates("fwd", (B, 160, 4, 4), (512, 160, 3, 3), 1, 1,
                             CUS) == ()
    assert splitk_candidates("fwd", (B, 512, 4, 4), (64, 512, 3, 3), 1, 1,
                             CUS) == ()
    assert splitk_candidates("wgrad", *R18["l4 3x3"], CUS) == ()


def test_env_switch_removes_the_candidates(monkeypatch):
    monkeypatch.setenv("MI355X_CONV_SPLITK", "0")
    for name in R18:
        assert _cands("fwd", name) == ()
        assert _cands("dgrad", name) == ()


def test_autotune_off_keeps_the_heuristic(monkeypatch):
    """With the tuner off the choice is the default 0, the kernels' size
    heuristic, which never splits; nothing is measured or cached."""
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    key = ("fwd", "test_conv_splitk_cpu")

    def boom(*a):
        raise AssertionError("the tuner must not run")

    assert conv_mod._tuned_choice(key, boom, boom, default=0) == 0
    assert key not in conv_mod._TUNE_CACHE


def test_report_names_a_split_choice():
    key = conv_mod._tune_key("fwd", "bf16-test", (1,), (2,), 1, 1)
    conv_mod._TUNE_CACHE[key] = (228, 4)
    try:
        assert "128x128 tile, split-K x4" in conv_mod.tune_report()
    finally:
        del conv_mod._TUNE_CACHE[key]
