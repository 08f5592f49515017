"""CutMix on the device-data path, without a GPU: the table builder, the
torch definition, the loader's tuple target, and the config/CLI/engine
wiring."""
import argparse

import numpy as np
import pytest
import torch

from mi355x_ddp.config import TrainConfig, add_common_args, config_from_args
from mi355x_ddp.data import DeviceCIFAR, DeviceLoader, build_loaders
from mi355x_ddp.data import device as device_data
from mi355x_ddp.ops import (batch_augment_cutmix, build_norm_lut,
                            draw_aug_params, draw_cutmix_params)
from mi355x_ddp.ops.augment import (_batch_augment_cutmix_torch,
                                    _batch_augment_torch)


def _unpack(mix):
    m = mix.long()
    return (m[:, 0], m[:, 1] & 0xffff, m[:, 1] >> 16, m[:, 2] & 0xffff,
            m[:, 2] >> 16)


# ---- draw_cutmix_params -----------------------------------------------------

def test_tables_deterministic_per_seed_and_epoch():
    a = draw_cutmix_params(500, 32, 32, 1.0, 0.5, seed=3, epoch=7)
    b = draw_cutmix_params(500, 32, 32, 1.0, 0.5, seed=3, epoch=7)
    assert a[0].dtype == torch.int32 and a[0].shape == (500, 3)
    assert a[1].dtype == torch.float32 and a[1].shape == (500,)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for other in (draw_cutmix_params(500, 32, 32, 1.0, 0.5, seed=3, epoch=8),
                  draw_cutmix_params(500, 32, 32, 1.0, 0.5, seed=4, epoch=7)):
        assert not torch.equal(a[0], other[0])
        assert not torch.equal(a[1], other[1])


@pytest.mark.parametrize("hw", [(32, 32), (6, 5), (1, 9)])
@pytest.mark.parametrize("alpha", [0.3, 1.0])
def test_boxes_lie_inside_and_lam_is_the_area_left(hw, alpha):
    H, W = hw
    n = 2000
    mix, lam = draw_cutmix_params(n, H, W, alpha, 0.5, seed=1, epoch=2)
    partner, y0, y1, x0, x1 = _unpack(mix)
    assert ((partner >= -1) & (partner < n)).all()
    assert ((0 <= y0) & (y0 <= y1) & (y1 <= H)).all()
    assert ((0 <= x0) & (x0 <= x1) & (x1 <= W)).all()
    mixed = partner >= 0
    # a row is mixed with probability 0.5: 2000 draws, 5 sigma is 112
    assert abs(int(mixed.sum()) - n // 2) < 112
    area = ((y1 - y0) * (x1 - x0)).double()
    want = torch.where(mixed, 1.0 - area / (H * W),
                       torch.ones((), dtype=torch.float64)).float()
    assert torch.equal(lam, want)
    assert (lam >= 0).all() and (lam <= 1).all()
    if (H, W) == (32, 32):
        # both sides of Beta(alpha, alpha) are drawn (on a tiny image the
        # halved, floored sides keep the box well below the whole image)
        assert lam[mixed].min() < 0.3 and lam[mixed].max() > 0.7


def test_prob_zero_mixes_nothing_and_prob_one_everything():
    mix, lam = draw_cutmix_params(300, 32, 32, 1.0, 0.0, seed=0, epoch=0)
    assert (mix[:, 0] == -1).all() and (lam == 1).all()
    mix, lam = draw_cutmix_params(300, 32, 32, 1.0, 1.0, seed=0, epoch=0)
    assert (mix[:, 0] >= 0).all()


def test_draw_aug_params_is_what_it_was():
    """The new builder has a generator of its own and does not touch the
    global one either: the augmentation table keeps these words (first eight
    of seed 9, epoch 0, pad 4, hflip on, written down from the code before
    CutMix existed) whether or not CutMix tables are drawn around it."""
    before = draw_aug_params(4, 4, True, seed=9, epoch=0)
    torch.manual_seed(77)
    state = torch.get_rng_state()
    draw_cutmix_params(50, 32, 32, 1.0, 0.5, seed=9, epoch=0)
    assert torch.equal(torch.get_rng_state(), state)
    after = draw_aug_params(4, 4, True, seed=9, epoch=0)
    assert torch.equal(before, after)
    gen = torch.Generator().manual_seed(9 * 1_000_003 + 0)
    top = torch.randint(0, 9, (4,), generator=gen)
    left = torch.randint(0, 9, (4,), generator=gen)
    flip = torch.randint(0, 2, (4,), generator=gen)
    assert torch.equal(after, (top | (left << 8) | (flip << 16)).int())


def test_bad_table_arguments_raise():
    with pytest.raises(ValueError, match="alpha"):
        draw_cutmix_params(4, 8, 8, 0.0, 0.5, 0, 0)
    with pytest.raises(ValueError, match="prob"):
        draw_cutmix_params(4, 8, 8, 1.0, 1.5, 0, 0)


# ---- the torch definition ---------------------------------------------------

def _pack_aug(top, left, flip):
    return top | (left << 8) | (flip << 16)


def _pack_mix(partner, y0, y1, x0, x1):
    return [partner, y0 | (y1 << 16), x0 | (x1 << 16)]


def test_definition_on_a_hand_made_case():
    """8x8, pad 2, M=3. Expected pixels come from the definition, one pixel
    at a time: inside the box the partner's byte under the PARTNER's crop and
    flip, outside the sample's byte under its own; zero byte over padding."""
    H = W = 8
    pad = 2
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (3, H, W, 3), dtype=torch.uint8,
                           generator=gen)
    labels = torch.tensor([10, 20, 30])
    aug_rows = [(0, 4, 0), (3, 1, 1), (2, 2, 0)]
    aug = torch.tensor([_pack_aug(*r) for r in aug_rows], dtype=torch.int32)
    mix_rows = [(1, 2, 6, 1, 8), (-1, 0, 8, 0, 8), (2, 0, 3, 5, 8)]
    mix = torch.tensor([_pack_mix(*r) for r in mix_rows], dtype=torch.int32)
    lam = torch.tensor([1 - 28 / 64, 1.0, 1 - 9 / 64])
    idx = torch.tensor([2, 0, 1, 0], dtype=torch.int32)
    lut = build_norm_lut()

    def augmented(k, c, h, w):
        top, left, flip = aug_rows[k]
        sh = h + top - pad
        sw = (W - 1 - w if flip else w) + left - pad
        byte = int(images[k, sh, sw, c]) if 0 <= sh < H and 0 <= sw < W else 0
        return lut[c, byte]

    want = torch.empty(4, 3, H, W)
    for n, i in enumerate(idx.tolist()):
        p, y0, y1, x0, x1 = mix_rows[i]
        for c in range(3):
            for h in range(H):
                for w in range(W):
                    inside = p >= 0 and y0 <= h < y1 and x0 <= w < x1
                    want[n, c, h, w] = augmented(p if inside else i, c, h, w)

    for fn in (_batch_augment_cutmix_torch, batch_augment_cutmix):
        out, la, lb, lo = fn(images, labels, idx, aug, mix, lam, lut, pad,
                             False, torch.float32)
        assert torch.equal(out, want)
        assert torch.equal(la, torch.tensor([30, 10, 20, 10]))
        assert torch.equal(lb, torch.tensor([30, 20, 20, 20]))
        assert torch.equal(lo, lam[idx.long()])
    # the mixed rows differ from the unmixed image, the unmixed one does not
    plain, _ = _batch_augment_torch(images, labels, idx, aug, lut, pad, False,
                                    torch.float32)
    assert torch.equal(out[2], plain[2])
    assert not torch.equal(out[1], plain[1])
    # channels_last and a 16-bit dtype hold the same values, rounded
    out_cl, _, _, _ = _batch_augment_cutmix_torch(
        images, labels, idx, aug, mix, lam, lut, pad, True, torch.bfloat16)
    assert out_cl.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out_cl, want.to(torch.bfloat16))


def test_partner_out_of_range_is_not_mixed_and_args_are_checked():
    images = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    labels = torch.tensor([1, 2])
    idx = torch.tensor([0, 1], dtype=torch.int32)
    mix = torch.tensor([_pack_mix(2, 0, 4, 0, 4), _pack_mix(-1, 0, 4, 0, 4)],
                       dtype=torch.int32)
    lam = torch.tensor([0.0, 0.0])
    lut = build_norm_lut()
    _, la, lb, lo = batch_augment_cutmix(images, labels, idx, None, mix, lam,
                                         lut, 1)
    assert torch.equal(la, labels) and torch.equal(lb, labels)
    assert torch.equal(lo, torch.ones(2))
    with pytest.raises(ValueError, match="mix_i32"):
        batch_augment_cutmix(images, labels, idx, None, mix.long(), lam, lut)
    with pytest.raises(ValueError, match="mix_i32"):
        batch_augment_cutmix(images, labels, idx, None, mix[:1], lam, lut)
    with pytest.raises(ValueError, match="lam_f32"):
        batch_augment_cutmix(images, labels, idx, None, mix, lam.double(),
                             lut)
    with pytest.raises(ValueError, match="lam_f32"):
        batch_augment_cutmix(images, labels, idx, None, mix, lam[:1], lut)


# ---- loader -----------------------------------------------------------------

def _loader(ds, world, rank, **kw):
    base = dict(batch_size=8, world_size=world, rank=rank, shuffle=True,
                drop_last=False, seed=3, augment=True, pad=2, hflip=True,
                cutmix_alpha=1.0, cutmix_prob=0.5)
    base.update(kw)
    return DeviceLoader(ds, **base)


def test_loader_yields_tuple_target_with_cutmix_and_plain_without():
    ds = DeviceCIFAR.synthetic(n=40, size=8, seed=2, device="cpu")
    ld = _loader(ds, 1, 0)
    ld.set_epoch(0)
    batches = list(ld)
    assert len(batches) == 5
    mixed_rows = 0
    for b, (images, target) in enumerate(batches):
        labels_a, labels_b, lam = target
        idx = ld.indices[b * 8:(b + 1) * 8].long()
        assert images.shape == (8, 3, 8, 8)
        assert labels_a.dtype == labels_b.dtype == torch.int64
        assert lam.dtype == torch.float32 and lam.shape == (8,)
        assert torch.equal(labels_a, ds.labels[idx])
        partner = ld.mix[idx, 0].long()
        assert torch.equal(labels_b, torch.where(
            partner >= 0, ds.labels[partner.clamp(min=0)], labels_a))
        assert torch.equal(lam, ld.lam[idx])
        mixed_rows += int((partner >= 0).sum())
    assert 0 < mixed_rows < 40
    # off by default, and the test loader's arguments never mix
    plain = _loader(ds, 1, 0, cutmix_alpha=0.0)
    images, labels = next(iter(plain))
    assert isinstance(labels, torch.Tensor) and plain.mix is None
    with pytest.raises(ValueError, match="cutmix_alpha"):
        _loader(ds, 1, 0, cutmix_alpha=-1.0)
    with pytest.raises(ValueError, match="cutmix_prob"):
        _loader(ds, 1, 0, cutmix_prob=2.0)


def test_cutmix_sample_is_world_size_invariant():
    ds = DeviceCIFAR.synthetic(n=64, size=8, seed=2, device="cpu")

    def by_index(world):
        rows = {}
        for rank in range(world):
            ld = _loader(ds, world, rank, batch_size=16 // world)
            ld.set_epoch(1)
            batches = list(ld)
            flat = torch.cat([b[0] for b in batches])
            lb = torch.cat([b[1][1] for b in batches])
            lam = torch.cat([b[1][2] for b in batches])
            for i, img, b, l in zip(ld.indices.tolist(), flat, lb, lam):
                rows[i] = (img, int(b), float(l))
        return rows

    one, two = by_index(1), by_index(2)
    assert sorted(one) == sorted(two) == list(range(64))
    for i in one:
        assert torch.equal(one[i][0], two[i][0]) and one[i][1:] == two[i][1:]


# ---- config, CLI, engine ----------------------------------------------------

def test_config_validation():
    cfg = TrainConfig()
    assert cfg.label_smoothing == 0.0 and cfg.cutmix_alpha == 0.0
    assert cfg.cutmix_prob == 0.5
    TrainConfig(label_smoothing=0.1)              # needs no device_data
    TrainConfig(device_data=True, cutmix_alpha=1.0, cutmix_prob=1.0)
    with pytest.raises(ValueError, match="device_data"):
        TrainConfig(cutmix_alpha=1.0)
    with pytest.raises(ValueError, match="cutmix_alpha"):
        TrainConfig(device_data=True, cutmix_alpha=-0.5)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            TrainConfig(label_smoothing=bad)
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError, match="cutmix_prob"):
            TrainConfig(cutmix_prob=bad)


def test_cli_flags():
    parser = add_common_args(argparse.ArgumentParser())
    cfg = config_from_args(parser.parse_args([]))
    assert (cfg.label_smoothing, cfg.cutmix_alpha, cfg.cutmix_prob) \
        == (0.0, 0.0, 0.5)
    cfg = config_from_args(parser.parse_args(
        ["--device_data", "--cutmix_alpha", "1.0", "--cutmix_prob", "0.25",
         "--label_smoothing", "0.1"]))
    assert (cfg.label_smoothing, cfg.cutmix_alpha, cfg.cutmix_prob) \
        == (0.1, 1.0, 0.25)
    with pytest.raises(ValueError, match="device_data"):
        config_from_args(parser.parse_args(["--cutmix_alpha", "1.0"]))


def test_build_wiring_and_one_cpu_epoch(monkeypatch):
    from mi355x_ddp.core.engine import train_one_epoch
    from mi355x_ddp.core.worker import build_training, init_seeds

    monkeypatch.setattr(device_data, "SYNTHETIC_TRAIN_N", 64)
    monkeypatch.setattr(device_data, "SYNTHETIC_TEST_N", 64)
    init_seeds(0)
    device = torch.device("cpu")
    cfg = TrainConfig(batch_size=8, num_workers=0, synthetic=True, lr=0.05,
                      log_interval=1, device_data=True, cutmix_alpha=1.0,
                      cutmix_prob=1.0, label_smoothing=0.1,
                      stall_dump_s=None)
    train_loader, test_loader, sampler = build_loaders(
        cfg, 1, 0, distributed=False, device=device)
    assert train_loader.cutmix_alpha == 1.0 and train_loader.cutmix_prob == 1.0
    assert test_loader.cutmix_alpha == 0.0
    assert isinstance(next(iter(test_loader))[1], torch.Tensor)
    model, crit, opt, sched, scaler = build_training(
        cfg, device, 1, 0, distributed=True, wrap="flat")
    assert crit.label_smoothing == 0.1
    targets = []

    class Recording(torch.nn.Module):
        def forward(self, out, target):
            targets.append(target)
            return crit(out, target)

    sampler.set_epoch(0)
    mean = train_one_epoch(model, train_loader, Recording(), opt, 0, cfg,
                           device, max_steps=2)
    assert np.isfinite(mean) and len(targets) == 2
    assert all(isinstance(t, tuple) and len(t) == 3 for t in targets)
    # gradient accumulation slices the tuple like a tensor
    targets.clear()
    mean = train_one_epoch(model, train_loader, Recording(), opt, 0,
                           cfg.replace(grad_accu_steps=2), device, max_steps=1)
    assert np.isfinite(mean) and len(targets) == 2
    assert all(t[0].shape == t[1].shape == t[2].shape == (4,)
               for t in targets)
