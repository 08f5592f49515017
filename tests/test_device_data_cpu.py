"""Device-resident input path on the torch fallback (device="cpu"): the
augmentation table, the batch_augment definition, DeviceLoader sharding and
the build_loaders / CLI wiring."""
import argparse
import pickle

import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

from mi355x_ddp.config import TrainConfig, add_common_args, config_from_args
from mi355x_ddp.data import (DeviceCIFAR, DeviceLoader, PickleCIFAR100,
                             build_loaders, normalize)
from mi355x_ddp.data import device as device_data
from mi355x_ddp.ops import batch_augment, build_norm_lut, draw_aug_params


def _unpack(a):
    a = a.long()
    return a & 0xff, (a >> 8) & 0xff, (a >> 16) & 0xff, a >> 24


def _pack(top, left, flip):
    return top | (left << 8) | (flip << 16)


# ---- draw_aug_params -------------------------------------------------------

def test_draw_aug_params_field_ranges():
    a = draw_aug_params(4096, 4, True, seed=3, epoch=0)
    assert a.dtype == torch.int32 and a.shape == (4096,)
    top, left, flip, rest = _unpack(a)
    assert int(top.min()) == 0 and int(top.max()) == 8
    assert int(left.min()) == 0 and int(left.max()) == 8
    assert set(flip.tolist()) == {0, 1}
    assert int(rest.abs().max()) == 0
    # pad 0: the only window is the image itself
    t0, l0, _, _ = _unpack(draw_aug_params(64, 0, True, seed=3, epoch=0))
    assert int(t0.max()) == 0 and int(l0.max()) == 0


def test_draw_aug_params_seed_and_epoch():
    a = draw_aug_params(512, 4, True, seed=5, epoch=0)
    assert torch.equal(a, draw_aug_params(512, 4, True, seed=5, epoch=0))
    assert not torch.equal(a, draw_aug_params(512, 4, True, seed=5, epoch=1))
    assert not torch.equal(a, draw_aug_params(512, 4, True, seed=6, epoch=0))


def test_draw_aug_params_hflip_leaves_crop_alone():
    on = draw_aug_params(512, 4, True, seed=1, epoch=2)
    off = draw_aug_params(512, 4, False, seed=1, epoch=2)
    t1, l1, f1, _ = _unpack(on)
    t0, l0, f0, _ = _unpack(off)
    assert torch.equal(t1, t0) and torch.equal(l1, l0)
    assert int(f0.max()) == 0 and int(f1.max()) == 1


# ---- batch_augment definition ---------------------------------------------

def _triple_loop(images, labels, idx, aug, lut, pad):
    """The definition, one output pixel at a time."""
    M, H, W, _ = images.shape
    out = torch.empty(len(idx), 3, H, W)
    lab = torch.empty(len(idx), dtype=torch.int64)
    for n, i in enumerate(idx.tolist()):
        top, left, flip = (pad, pad, 0) if aug is None else (
            int(aug[i]) & 0xff, (int(aug[i]) >> 8) & 0xff,
            (int(aug[i]) >> 16) & 1)
        lab[n] = labels[i]
        for c in range(3):
            for h in range(H):
                for w in range(W):
                    sh = h + top - pad
                    sw = (W - 1 - w if flip else w) + left - pad
                    byte = int(images[i, sh, sw, c]) \
                        if 0 <= sh < H and 0 <= sw < W else 0
                    out[n, c, h, w] = lut[c, byte]
    return out, lab


def _small_case():
    gen = torch.Generator().manual_seed(0)
    images = torch.randint(1, 256, (2, 4, 4, 3), dtype=torch.uint8,
                           generator=gen)
    labels = torch.tensor([7, 42])
    aug = torch.tensor([_pack(0, 0, 0), _pack(2, 2, 1)], dtype=torch.int32)
    return images, labels, aug, build_norm_lut()


@pytest.mark.parametrize("channels_last", [False, True])
def test_fallback_matches_triple_loop(channels_last):
    images, labels, aug, lut = _small_case()
    idx = torch.tensor([1, 0, 1], dtype=torch.int32)
    out, lab = batch_augment(images, labels, idx, aug, lut, pad=1,
                             channels_last=channels_last)
    ref, ref_lab = _triple_loop(images, labels, idx, aug, lut, 1)
    assert out.shape == (3, 3, 4, 4) and out.dtype == torch.float32
    assert torch.equal(out, ref) and torch.equal(lab, ref_lab)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert out.is_contiguous(memory_format=fmt)
    # a third table entry: crop only (top=1 is centred, left=2 shifts), and a
    # flip without a shift
    aug2 = torch.tensor([_pack(1, 2, 0), _pack(1, 1, 1)], dtype=torch.int32)
    out2, _ = batch_augment(images, labels, idx, aug2, lut, pad=1)
    assert torch.equal(out2, _triple_loop(images, labels, idx, aug2, lut, 1)[0])
    centred = batch_augment(images, labels, idx, None, lut, pad=1)[0]
    assert torch.equal(out2[0], centred[0].flip(-1))


def test_padded_border_is_lut_of_zero_byte():
    images, labels, aug, lut = _small_case()   # bytes are all >= 1
    idx = torch.tensor([0, 1], dtype=torch.int32)
    out, _ = batch_augment(images, labels, idx, aug, lut, pad=1)
    for c in range(3):
        # image 0: top=0,left=0 -> first output row and column are padding
        assert torch.all(out[0, c, 0, :] == lut[c, 0])
        assert torch.all(out[0, c, :, 0] == lut[c, 0])
        assert torch.all(out[0, c, 1:, 1:] != lut[c, 0])
        # image 1: top=2,left=2 with a flip -> last row; the flipped window's
        # padding column lands on output column 0
        assert torch.all(out[1, c, 3, :] == lut[c, 0])
        assert torch.all(out[1, c, :, 0] == lut[c, 0])
        assert float(lut[c, 0]) != 0.0


def test_eval_identity_equals_normalize_bitwise():
    gen = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (5, 32, 32, 3), dtype=torch.uint8,
                           generator=gen)
    # every byte value in every channel at least once
    images[0].view(-1, 3)[:256] = torch.arange(256, dtype=torch.uint8)[:, None]
    labels = torch.arange(5)
    idx = torch.arange(5, dtype=torch.int32)
    out, lab = batch_augment(images, labels, idx, None, build_norm_lut(),
                             pad=4)
    want = torch.stack([normalize(im.permute(2, 0, 1).float().div(255))
                        for im in images])
    assert torch.equal(out, want) and torch.equal(lab, labels)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fallback_low_precision_is_rounded_fp32(dtype):
    images, labels, aug, lut = _small_case()
    idx = torch.tensor([0, 1], dtype=torch.int32)
    lo, _ = batch_augment(images, labels, idx, aug, lut, pad=1,
                          out_dtype=dtype)
    hi, _ = batch_augment(images, labels, idx, aug, lut, pad=1)
    assert lo.dtype == dtype and torch.equal(lo, hi.to(dtype))


def test_batch_augment_rejects_bad_arguments():
    images, labels, aug, lut = _small_case()
    idx = torch.tensor([0], dtype=torch.int32)
    with pytest.raises(ValueError):
        batch_augment(images[..., :2].contiguous(), labels, idx, aug, lut, 1)
    with pytest.raises(ValueError):
        batch_augment(images.float(), labels, idx, aug, lut, 1)
    with pytest.raises(ValueError):
        batch_augment(images.permute(0, 2, 1, 3), labels, idx, aug, lut, 1)
    with pytest.raises(ValueError):
        batch_augment(images, labels, idx.long(), aug, lut, 1)
    with pytest.raises(ValueError):
        batch_augment(images, labels, idx, aug, lut, 128)


# ---- DeviceLoader ----------------------------------------------------------

def _loader(ds, world, rank, **kw):
    base = dict(batch_size=8, world_size=world, rank=rank, shuffle=True,
                drop_last=True, seed=11, augment=True, hflip=True)
    base.update(kw)
    return DeviceLoader(ds, **base)


@pytest.mark.parametrize("drop_last", [True, False])
def test_device_loader_shards_like_distributed_sampler(drop_last):
    ds = DeviceCIFAR.synthetic(n=61, size=8, seed=2, device="cpu")
    seen = []
    for rank in range(2):
        ld = _loader(ds, 2, rank, drop_last=drop_last)
        ld.set_epoch(3)
        sampler = DistributedSampler(range(61), num_replicas=2, rank=rank,
                                     shuffle=True, seed=11,
                                     drop_last=drop_last)
        sampler.set_epoch(3)
        want = list(sampler)
        assert ld.indices.dtype == torch.int32
        assert ld.indices.tolist() == want
        n_batches = len(want) // 8 if drop_last else -(-len(want) // 8)
        assert len(ld) == n_batches
        batches = list(ld)
        assert len(batches) == n_batches
        got = sum(b[0].shape[0] for b in batches)
        assert got == (n_batches * 8 if drop_last else len(want))
        labels = torch.cat([b[1] for b in batches])
        assert torch.equal(labels, ds.labels[torch.tensor(want)[:got]])
        seen += want
    union = set(seen)
    assert union <= set(range(61))
    assert len(union) == (60 if drop_last else 61)


def test_device_loader_sample_is_world_size_invariant():
    ds = DeviceCIFAR.synthetic(n=64, size=8, seed=2, device="cpu")

    def by_index(world):
        images = {}
        for rank in range(world):
            ld = _loader(ds, world, rank, batch_size=16 // world)
            ld.set_epoch(1)
            flat = torch.cat([b[0] for b in ld])
            for i, img in zip(ld.indices.tolist(), flat):
                images[i] = img
        return images

    one, two = by_index(1), by_index(2)
    assert sorted(one) == sorted(two) == list(range(64))
    assert all(torch.equal(one[i], two[i]) for i in one)
    # and the epoch changes it
    ld = _loader(ds, 1, 0, batch_size=16)
    ld.set_epoch(2)
    other = dict(zip(ld.indices.tolist(), torch.cat([b[0] for b in ld])))
    assert any(not torch.equal(one[i], other[i]) for i in one)


def test_device_loader_defaults_to_epoch_zero_and_ignores_global_rng():
    ds = DeviceCIFAR.synthetic(n=40, size=8, seed=2, device="cpu")
    a = _loader(ds, 1, 0)
    torch.manual_seed(123)
    first = [b[0] for b in a]
    b = _loader(ds, 1, 0)
    b.set_epoch(0)
    torch.manual_seed(456)
    second = [x[0] for x in b]
    assert a.epoch == 0 and len(first) == len(second) == 5
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    assert sorted(a.indices.tolist()) != a.indices.tolist()   # shuffled


def test_synthetic_dataset_deterministic_per_seed_and_split():
    a = DeviceCIFAR.synthetic(n=16, size=8, seed=4, device="cpu")
    b = DeviceCIFAR.synthetic(n=16, size=8, seed=4, device="cpu")
    assert a.images_u8.shape == (16, 8, 8, 3)
    assert a.images_u8.dtype == torch.uint8 and a.labels.dtype == torch.int64
    assert torch.equal(a.images_u8, b.images_u8)
    assert torch.equal(a.labels, b.labels)
    for other in (DeviceCIFAR.synthetic(n=16, size=8, seed=5, device="cpu"),
                  DeviceCIFAR.synthetic(n=16, size=8, seed=4, train=False,
                                        device="cpu")):
        assert not torch.equal(a.images_u8, other.images_u8)


@pytest.mark.parametrize("world", [1, 2])
def test_device_loader_len_matches_dataloader(world):
    cfg = TrainConfig(batch_size=48, num_workers=0, synthetic=True)
    old_train, old_test, _ = build_loaders(cfg, world, 0,
                                           distributed=world > 1)
    train_ds = DeviceCIFAR.synthetic(n=len(old_train.dataset), size=2,
                                     device="cpu")
    test_ds = DeviceCIFAR.synthetic(n=len(old_test.dataset), size=2,
                                    train=False, device="cpu")
    per_rank = cfg.per_rank_batch(world)
    new_train = DeviceLoader(train_ds, per_rank, world, 0, shuffle=True,
                             drop_last=True, augment=True)
    new_test = DeviceLoader(test_ds, per_rank, world, 0, shuffle=False,
                            drop_last=False)
    assert len(new_train) == len(old_train)
    assert len(new_test) == len(old_test)


# ---- wiring ----------------------------------------------------------------

def test_build_loaders_device_data_runs_fit(tmp_path, monkeypatch):
    from mi355x_ddp.core.engine import fit
    from mi355x_ddp.core.worker import build_training, init_seeds

    monkeypatch.setattr(device_data, "SYNTHETIC_TRAIN_N", 64)
    monkeypatch.setattr(device_data, "SYNTHETIC_TEST_N", 64)
    init_seeds(0)
    cfg = TrainConfig(batch_size=8, epochs=2, num_workers=0, synthetic=True,
                      lr=0.05, log_interval=1, max_train_steps=2,
                      max_eval_steps=1, save_epoch=0,
                      ckpt_dir=str(tmp_path / "ckpts"),
                      metrics_dir=str(tmp_path / "runs"))
    device = torch.device("cpu")
    train_loader, test_loader, sampler = build_loaders(
        cfg.replace(device_data=True), 1, 0, distributed=False, device=device)
    assert isinstance(train_loader, DeviceLoader)
    assert isinstance(test_loader, DeviceLoader)
    assert sampler is train_loader          # fit calls set_epoch on it
    assert len(train_loader) == 8 and len(test_loader) == 8
    assert train_loader.augment and not test_loader.augment

    # record what the model is fed and the loss of every step
    model, crit, opt, sched, scaler = build_training(
        cfg, device, 1, 0, distributed=True, wrap="flat")
    fed, losses = [], []
    model.register_forward_pre_hook(
        lambda m, args: fed.append(args[0].detach().clone()))

    class Recording(torch.nn.Module):
        def forward(self, out, target):
            loss = crit(out, target)
            losses.append(float(loss.detach()))
            return loss

    fit(model, train_loader, test_loader, sampler, Recording(), opt, sched,
        cfg, device)
    assert train_loader.epoch == 1
    assert len(losses) == 6 and all(np.isfinite(losses))   # 2x(2 train+1 eval)
    epoch0, epoch1 = fed[0:2], fed[3:5]
    assert all(x.shape == (8, 3, 32, 32) and x.dtype == torch.float32
               for x in epoch0 + epoch1)
    assert not any(torch.equal(a, b) for a in epoch0 for b in epoch1)
    # the evaluation batch is the same in both epochs
    assert torch.equal(fed[2], fed[5])


def test_build_loaders_flag_off_is_dataloader():
    cfg = TrainConfig(batch_size=32, num_workers=0, synthetic=True)
    assert cfg.device_data is False and cfg.hflip is False
    train_loader, _, sampler = build_loaders(cfg, 1, 0, distributed=False,
                                             device=torch.device("cpu"))
    assert isinstance(train_loader, torch.utils.data.DataLoader)
    assert sampler is None


@pytest.mark.parametrize("amp,dtype", [("fp32", torch.float32),
                                       ("bf16", torch.bfloat16),
                                       ("bf16_o2", torch.bfloat16),
                                       ("fp16", torch.float16)])
def test_build_loaders_out_dtype_follows_amp(monkeypatch, amp, dtype):
    monkeypatch.setattr(device_data, "SYNTHETIC_TRAIN_N", 16)
    monkeypatch.setattr(device_data, "SYNTHETIC_TEST_N", 16)
    cfg = TrainConfig(batch_size=8, synthetic=True, amp=amp,
                      channels_last=True, device_data=True, hflip=True)
    train_loader, test_loader, _ = build_loaders(cfg, 2, 1,
                                                 device=torch.device("cpu"))
    assert train_loader.batch_size == 4 and train_loader.hflip
    for loader in (train_loader, test_loader):
        images, labels = next(iter(loader))
        assert images.dtype == dtype and images.shape == (4, 3, 32, 32)
        assert images.is_contiguous(memory_format=torch.channels_last)
        assert labels.dtype == torch.int64


def test_cli_flags():
    parser = add_common_args(argparse.ArgumentParser())
    cfg = config_from_args(parser.parse_args([]))
    assert not cfg.device_data and not cfg.hflip
    cfg = config_from_args(parser.parse_args(["--device_data"]))
    assert cfg.device_data and not cfg.hflip
    cfg = config_from_args(parser.parse_args(["--device_data", "--hflip"]))
    assert cfg.device_data and cfg.hflip
    with pytest.raises(ValueError, match="device_data"):
        config_from_args(parser.parse_args(["--hflip"]))
    with pytest.raises(ValueError, match="device_data"):
        TrainConfig(hflip=True)


def test_cli_entry_trains_with_device_data(tmp_path):
    """The flag through a whole entry script (what this test is about): one
    capped epoch and an evaluation with --device_data --hflip."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(
        [sys.executable, os.path.join(root, "dataparallel.py"),
         "--epochs", "1", "--batch_size", "16", "--num_workers", "0",
         "--synthetic", "--max_train_steps", "2", "--max_eval_steps", "1",
         "--log_interval", "1", "--save_epoch", "0", "--device_data",
         "--hflip"],
        cwd=tmp_path, env=dict(os.environ, PYTHONPATH=root),
        capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch: [0][1/3125]" in r.stdout      # 50000 // 16 batches
    assert "Acc@1" in r.stdout


def test_pickle_constructor_matches_pickle_cifar100_eval(tmp_path):
    d = tmp_path / "cifar-100-python"
    d.mkdir()
    rng = np.random.default_rng(0)
    for name, n in (("train", 12), ("test", 6)):
        payload = {b"data": rng.integers(0, 256, (n, 3072), dtype=np.uint8),
                   b"fine_labels": [int(x) for x in rng.integers(0, 100, n)]}
        with open(d / name, "wb") as f:
            pickle.dump(payload, f)

    for train, n in ((True, 12), (False, 6)):
        ds = DeviceCIFAR.from_pickle(str(tmp_path), train=train, device="cpu")
        assert len(ds) == n and ds.images_u8.shape == (n, 32, 32, 3)
        assert ds.images_u8.dtype == torch.uint8
        old = PickleCIFAR100(str(tmp_path), train=False)
        if train:   # read the train file, but without the crop
            old = PickleCIFAR100(str(tmp_path), train=True)
            old.train = False
        loader = DeviceLoader(ds, batch_size=5, shuffle=False,
                              drop_last=False, augment=False)
        images = torch.cat([b[0] for b in loader])
        labels = torch.cat([b[1] for b in loader])
        assert len(loader) == -(-n // 5)
        for i in range(n):
            want, want_label = old[i]
            assert torch.equal(images[i], want)
            assert int(labels[i]) == want_label

    # build_loaders picks the real data when synthetic=False and it exists
    cfg = TrainConfig(synthetic=False, data_root=str(tmp_path), batch_size=4,
                      device_data=True)
    train_loader, test_loader, _ = build_loaders(cfg, 1, 0, distributed=False,
                                                 device=torch.device("cpu"))
    assert len(train_loader.dataset) == 12 and len(test_loader.dataset) == 6
