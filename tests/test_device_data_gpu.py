"""Device-resident input path on the GPU: the batch_augment HIP kernel against
the torch definition (bit for bit: both are a table lookup plus one
round-to-nearest-even), DeviceLoader on the device, and one training epoch
fed by it."""
import pytest
import torch

from mi355x_ddp.config import TrainConfig
from mi355x_ddp.data import DeviceCIFAR, DeviceLoader, build_loaders
from mi355x_ddp.data import device as device_data
from mi355x_ddp.ops import (_backend, batch_augment, build_norm_lut,
                            draw_aug_params)
from mi355x_ddp.ops.augment import _batch_augment_torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _pack(top, left, flip):
    return top | (left << 8) | (flip << 16)


def _dataset(m, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (m, h, w, 3), dtype=torch.uint8,
                           generator=gen)
    labels = torch.randint(0, 100, (m,), generator=gen)
    return images, labels


def _case_borders():
    """M=7, N=5, 8x8, pad=2: a repeated index, passed as a slice view with a
    non-zero offset; windows in every corner, flip on and off."""
    images, labels = _dataset(7, 8, 8, 0)
    aug = torch.tensor([_pack(0, 0, 0), _pack(4, 4, 1), _pack(0, 4, 1),
                        _pack(4, 0, 1), _pack(4, 4, 0), _pack(0, 0, 1),
                        _pack(2, 2, 1)], dtype=torch.int32)
    base = torch.tensor([6, 4, 0, 2, 3, 3, 5, 1], dtype=torch.int32)
    return images, labels, base, slice(1, 6), aug, 2


def _case_real_size():
    """M=4, N=3, 32x32, pad=4, drawn parameters: the fast path at the size
    training uses."""
    images, labels = _dataset(4, 32, 32, 1)
    aug = draw_aug_params(4, 4, True, seed=9, epoch=0)
    base = torch.tensor([2, 0, 3], dtype=torch.int32)
    return images, labels, base, slice(0, 3), aug, 4


def _case_odd():
    """M=3, N=3, 6x5, pad=1: 90 elements per image, scalar path."""
    images, labels = _dataset(3, 6, 5, 2)
    aug = torch.tensor([_pack(0, 2, 1), _pack(2, 0, 0), _pack(1, 1, 1)],
                       dtype=torch.int32)
    base = torch.tensor([1, 2, 0], dtype=torch.int32)
    return images, labels, base, slice(0, 3), aug, 1


def _case_eval():
    """aug=None at 8x8: the identity window."""
    images, labels = _dataset(6, 8, 8, 3)
    base = torch.tensor([5, 0, 0, 3], dtype=torch.int32)
    return images, labels, base, slice(0, 4), None, 2


def _case_single():
    """N=1."""
    images, labels = _dataset(3, 8, 8, 4)
    aug = torch.tensor([_pack(1, 3, 0), _pack(3, 1, 1), _pack(4, 0, 1)],
                       dtype=torch.int32)
    base = torch.tensor([0, 1, 2], dtype=torch.int32)
    return images, labels, base, slice(1, 2), aug, 2


def _case_narrow_source():
    """M=3, N=2, 2x4, pad=1: 24 bytes per image, so the 16-byte-store path
    runs (bf16/fp16/fp32 images are 48/96 bytes) but the source image is not
    a whole number of 16-byte loads and is staged bytewise."""
    images, labels = _dataset(3, 2, 4, 5)
    aug = torch.tensor([_pack(0, 2, 1), _pack(2, 0, 0), _pack(1, 1, 1)],
                       dtype=torch.int32)
    base = torch.tensor([2, 2, 0, 1], dtype=torch.int32)
    return images, labels, base, slice(2, 4), aug, 1


def _case_many_blocks():
    """M=40, N=300 (more workgroups than a wave of them, every index
    repeated), 8x8, pad=2, drawn parameters."""
    images, labels = _dataset(40, 8, 8, 6)
    aug = draw_aug_params(40, 2, True, seed=1, epoch=3)
    gen = torch.Generator().manual_seed(7)
    base = torch.randint(0, 40, (301,), generator=gen).to(torch.int32)
    return images, labels, base, slice(1, 301), aug, 2


CASES = {"borders": _case_borders, "real_size": _case_real_size,
         "odd": _case_odd, "eval": _case_eval, "single": _case_single,
         "narrow_source": _case_narrow_source,
         "many_blocks": _case_many_blocks}


@pytest.fixture(scope="module")
def lut():
    return build_norm_lut()


@pytest.mark.parametrize("channels_last", [True, False],
                         ids=["channels_last", "nchw"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_torch_definition(case, dtype, channels_last, lut):
    images, labels, base, sl, aug, pad = CASES[case]()
    want, want_labels = _batch_augment_torch(
        images, labels, base[sl], aug, lut, pad, channels_last, dtype)

    dev = torch.device("cuda", 0)
    idx = base.to(dev)[sl]
    assert idx.storage_offset() == sl.start
    got, got_labels = batch_augment(
        images.to(dev), labels.to(dev), idx,
        None if aug is None else aug.to(dev), lut.to(dev), pad,
        channels_last, dtype)
    assert got.dtype == dtype and got.shape == want.shape
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert got.is_contiguous(memory_format=fmt)
    assert got.stride() == want.stride()
    assert torch.equal(got.cpu(), want)
    assert got_labels.dtype == torch.int64
    assert torch.equal(got_labels.cpu(), want_labels)


def test_kernel_rejects_bad_arguments(lut):
    dev = torch.device("cuda", 0)
    images, labels = _dataset(3, 8, 8, 0)
    images, labels, lut = images.to(dev), labels.to(dev), lut.to(dev)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    native = _backend.C().batch_augment

    def call(im=images, ix=idx, pad=2):
        return native(im, labels, ix, None, lut, pad, True, torch.bfloat16)

    with pytest.raises(RuntimeError, match="3 channels"):
        call(im=torch.zeros(3, 8, 8, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="uint8"):
        call(im=images.float())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(im=images.permute(0, 2, 1, 3))
    with pytest.raises(RuntimeError, match="int32"):
        call(ix=idx.long())
    with pytest.raises(RuntimeError, match="pad"):
        call(pad=128)
    out, _ = call(pad=127)          # the largest pad is accepted
    assert out.shape == (2, 3, 8, 8)


def test_device_loader_on_gpu_equals_cpu():
    """One epoch of a 64-image set, batch 24: two full batches and a short
    last one (drop_last=False)."""
    kw = dict(batch_size=24, shuffle=True, drop_last=False, seed=5,
              augment=True, hflip=True, channels_last=True,
              out_dtype=torch.bfloat16)
    cpu = DeviceLoader(DeviceCIFAR.synthetic(64, seed=1, device="cpu"), **kw)
    gpu = DeviceLoader(DeviceCIFAR.synthetic(64, seed=1, device="cuda:0"),
                       **kw)
    cpu.set_epoch(2)
    gpu.set_epoch(2)
    cpu_batches, gpu_batches = list(cpu), list(gpu)
    assert len(gpu) == 3 and len(gpu_batches) == len(cpu_batches) == 3
    assert [b[0].shape[0] for b in gpu_batches] == [24, 24, 16]
    for (gi, gl), (ci, cl) in zip(gpu_batches, cpu_batches):
        assert gi.is_cuda and gl.is_cuda and gi.dtype == torch.bfloat16
        assert gi.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(gi.cpu(), ci) and torch.equal(gl.cpu(), cl)


@pytest.mark.parametrize("n", [5, 256, 300])
def test_xent_loss_is_the_same_bits_every_run(n):
    """The scalar loss is summed over rows in a fixed order, so equal logits
    give equal bits (what the bit-for-bit comparison below rests on).
    Against float64: the kernel's fast exp/log are good to a few ulp, and the
    sum is two strided terms per thread and a shuffle tree eight levels deep,
    ten roundings (6e-7 relative) at worst; 1e-5 relative holds both."""
    gen = torch.Generator().manual_seed(n)
    logits = (4 * torch.randn(n, 100, generator=gen)).to(torch.bfloat16).cuda()
    target = torch.randint(0, 100, (n,), generator=gen).cuda()
    native = _backend.C().xent_fwd
    losses = torch.stack([native(logits, target)[0] for _ in range(6)])
    assert torch.equal(losses, losses[:1].expand(6))
    want = torch.nn.functional.cross_entropy(logits.double(), target)
    torch.testing.assert_close(losses[0].double(), want, rtol=1e-5, atol=0)


def _recording(crit, losses, logits):
    class Recording(torch.nn.Module):
        def forward(self, out, target):
            loss = crit(out, target)
            logits.append(out.detach().clone())
            losses.append(loss.detach().clone())
            return loss
    return Recording()


def test_train_epoch_fed_by_device_loader(monkeypatch):
    """The device path hands the model bf16 channels_last batches, and its
    first loss is bit for bit that of the same batch made as fp32 on the host
    and moved over the old way (.to(device), .to(channels_last), autocast)."""
    from mi355x_ddp.core.engine import train_one_epoch
    from mi355x_ddp.core.worker import build_training, init_seeds
    from mi355x_ddp.ops.conv import clear_autotune_cache

    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setattr(device_data, "SYNTHETIC_TRAIN_N", 64)
    monkeypatch.setattr(device_data, "SYNTHETIC_TEST_N", 64)
    clear_autotune_cache()
    device = torch.device("cuda", 0)
    cfg = TrainConfig(batch_size=32, amp="bf16", channels_last=True,
                      native_ops=True, sync_bn=False, synthetic=True,
                      device_data=True, log_interval=100, stall_dump_s=None)

    def run(loader, run_cfg):
        init_seeds(0)
        model, crit, opt, sched, scaler = build_training(
            run_cfg, device, 1, 0, distributed=True, wrap="flat")
        fed, losses, logits = [], [], []
        model.register_forward_pre_hook(lambda m, args: fed.append(args[0]))
        mean = train_one_epoch(model, loader,
                               _recording(crit, losses, logits), opt, 0,
                               run_cfg, device, max_steps=2)
        torch.cuda.synchronize()
        return fed, losses, logits, mean

    train_loader, _, sampler = build_loaders(cfg, 1, 0, distributed=False,
                                             device=device)
    assert isinstance(train_loader, DeviceLoader) and sampler is train_loader
    sampler.set_epoch(0)
    fed, losses, logits, mean = run(train_loader, cfg)
    assert len(fed) == 2 and len(losses) == 2
    assert torch.isfinite(torch.stack(losses)).all() and mean == mean
    for x in fed:
        assert x.is_cuda and x.dtype == torch.bfloat16
        assert x.shape == (32, 3, 32, 32)
        assert x.is_contiguous(memory_format=torch.channels_last)

    # the same first batch as fp32 NCHW from the CPU implementation
    host = DeviceLoader(DeviceCIFAR.synthetic(64, cfg.num_classes, 32, True,
                                              cfg.seed, "cpu"),
                        32, shuffle=True, drop_last=True, seed=cfg.seed,
                        augment=True, hflip=False, channels_last=False,
                        out_dtype=torch.float32)
    host.set_epoch(0)
    images, labels = next(iter(host))
    assert images.dtype == torch.float32 and not images.is_cuda
    fed_old, losses_old, logits_old, _ = run([(images, labels)],
                                             cfg.replace(device_data=False))
    assert fed_old[0].dtype == torch.float32       # autocast casts it later
    assert torch.equal(fed[0].cpu(), images.to(torch.bfloat16))
    assert torch.equal(logits[0], logits_old[0])
    assert torch.equal(losses[0], losses_old[0]), (losses[0], losses_old[0])
