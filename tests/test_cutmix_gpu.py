"""CutMix in the input kernel on the GPU: batch_augment_cutmix against the
torch definition (bit for bit, images, both label vectors and lam),
DeviceLoader with CutMix on the device, and training fed by it."""
import pytest
import torch
import torch.nn.functional as F

from mi355x_ddp.config import TrainConfig
from mi355x_ddp.data import DeviceCIFAR, DeviceLoader, build_loaders
from mi355x_ddp.data import device as device_data
from mi355x_ddp.ops import (_backend, batch_augment_cutmix, build_norm_lut,
                            draw_aug_params, draw_cutmix_params)
from mi355x_ddp.ops.augment import _batch_augment_cutmix_torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _pack(top, left, flip):
    return top | (left << 8) | (flip << 16)


def _mix(rows):
    """rows of (partner, y0, y1, x0, x1) -> int32 [M, 3]."""
    return torch.tensor([[p, y0 | (y1 << 16), x0 | (x1 << 16)]
                         for p, y0, y1, x0, x1 in rows], dtype=torch.int32)


def _lam(rows, H, W):
    return torch.tensor([1.0 - (y1 - y0) * (x1 - x0) / (H * W)
                         for _, y0, y1, x0, x1 in rows], dtype=torch.float32)


def _dataset(m, h, w, seed):
    gen = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (m, h, w, 3), dtype=torch.uint8,
                           generator=gen)
    labels = torch.randint(0, 100, (m,), generator=gen)
    return images, labels


# M=7, 8x8, pad=2: windows in every corner, flips 0 1 1 1 0 0 1. Every
# dataset index is used, index 3 twice, and idx is a slice view with a
# non-zero offset.
_BORDER_AUG = [_pack(0, 0, 0), _pack(4, 4, 1), _pack(0, 4, 1), _pack(4, 0, 1),
               _pack(4, 4, 0), _pack(0, 0, 1), _pack(2, 2, 1)]
_BORDER_BASE = [6, 4, 0, 2, 3, 3, 5, 1, 6]
_BORDER_SLICE = slice(1, 9)


def _case_boxes_a():
    """Boxes touching the top-left, top-right and bottom-left corners, the
    whole image, an empty box, a one-pixel box, partner == i, partners with
    the opposite flip (rows 0, 1, 3), partner -1."""
    images, labels = _dataset(7, 8, 8, 0)
    rows = [(1, 0, 3, 0, 5), (4, 0, 2, 6, 8), (2, 5, 8, 0, 3),
            (0, 0, 8, 0, 8), (6, 3, 3, 2, 6), (3, 4, 5, 4, 5),
            (-1, 4, 8, 4, 8)]
    return (images, labels, torch.tensor(_BORDER_BASE, dtype=torch.int32),
            _BORDER_SLICE, torch.tensor(_BORDER_AUG, dtype=torch.int32),
            _mix(rows), _lam(rows, 8, 8), 2)


def _case_boxes_b():
    """Partners out of range (M, INT32_MAX, a negative other than -1), all
    with a whole-image box that must not be applied; the bottom-right corner;
    partner == i with a one-pixel box; an opposite-flip partner inside."""
    images, labels = _dataset(7, 8, 8, 0)
    rows = [(7, 0, 8, 0, 8), (-1, 0, 8, 0, 8), (5, 4, 8, 4, 8),
            (3, 7, 8, 0, 1), (1, 2, 6, 1, 7), (2 ** 31 - 1, 0, 8, 0, 8),
            (-5, 0, 8, 0, 8)]
    return (images, labels, torch.tensor(_BORDER_BASE, dtype=torch.int32),
            _BORDER_SLICE, torch.tensor(_BORDER_AUG, dtype=torch.int32),
            _mix(rows), _lam(rows, 8, 8), 2)


def _case_real_size():
    """M=8, N=8, 32x32, pad=4, drawn tables (mixed and unmixed rows): the
    fast path at the size training uses."""
    images, labels = _dataset(8, 32, 32, 1)
    aug = draw_aug_params(8, 4, True, seed=9, epoch=0)
    mix, lam = draw_cutmix_params(8, 32, 32, 1.0, 0.5, seed=12, epoch=0)
    assert 0 < int((mix[:, 0] >= 0).sum()) < 8
    base = torch.tensor([2, 0, 3, 7, 5, 1, 6, 4], dtype=torch.int32)
    return images, labels, base, slice(0, 8), aug, mix, lam, 4


def _case_odd():
    """M=3, N=3, 6x5, pad=1: 90 elements per image, scalar path."""
    images, labels = _dataset(3, 6, 5, 2)
    aug = torch.tensor([_pack(0, 2, 1), _pack(2, 0, 0), _pack(1, 1, 1)],
                       dtype=torch.int32)
    rows = [(1, 1, 5, 0, 3), (-1, 0, 6, 0, 5), (0, 3, 6, 2, 5)]
    base = torch.tensor([1, 2, 0], dtype=torch.int32)
    return (images, labels, base, slice(0, 3), aug, _mix(rows),
            _lam(rows, 6, 5), 1)


def _case_narrow_source():
    """M=3, N=2, 2x4, pad=1: 24 bytes per image, so the 16-byte-store path
    runs but both sources are staged bytewise, and the partner's LDS region
    starts at the rounded-up offset 32, not at 24."""
    images, labels = _dataset(3, 2, 4, 5)
    aug = torch.tensor([_pack(0, 2, 1), _pack(2, 0, 0), _pack(1, 1, 1)],
                       dtype=torch.int32)
    rows = [(2, 0, 2, 1, 3), (0, 1, 2, 0, 4), (1, 0, 1, 2, 4)]
    base = torch.tensor([2, 2, 0, 1], dtype=torch.int32)
    return (images, labels, base, slice(2, 4), aug, _mix(rows),
            _lam(rows, 2, 4), 1)


def _case_many_blocks():
    """M=40, N=300 (more workgroups than a wave of them, every index
    repeated), 8x8, pad=2, drawn tables."""
    images, labels = _dataset(40, 8, 8, 6)
    aug = draw_aug_params(40, 2, True, seed=1, epoch=3)
    mix, lam = draw_cutmix_params(40, 8, 8, 1.0, 0.5, seed=1, epoch=3)
    gen = torch.Generator().manual_seed(7)
    base = torch.randint(0, 40, (301,), generator=gen).to(torch.int32)
    return images, labels, base, slice(1, 301), aug, mix, lam, 2


def _case_two_do_not_fit():
    """M=N=2, 104x104, pad=4: one 32448-byte image fits the fast path's LDS
    budget, the table plus two do not fit 64 KB, so channels_last takes the
    scalar path too."""
    images, labels = _dataset(2, 104, 104, 8)
    aug = torch.tensor([_pack(1, 7, 1), _pack(8, 0, 0)], dtype=torch.int32)
    rows = [(1, 10, 90, 0, 57), (0, 50, 104, 33, 104)]
    base = torch.tensor([1, 0], dtype=torch.int32)
    return (images, labels, base, slice(0, 2), aug, _mix(rows),
            _lam(rows, 104, 104), 4)


CASES = {"boxes_a": _case_boxes_a, "boxes_b": _case_boxes_b,
         "real_size": _case_real_size, "odd": _case_odd,
         "narrow_source": _case_narrow_source,
         "many_blocks": _case_many_blocks,
         "two_do_not_fit": _case_two_do_not_fit}


@pytest.fixture(scope="module")
def lut():
    return build_norm_lut()


@pytest.fixture(scope="module")
def on_device():
    """Each case's inputs uploaded once for the whole dtype x layout grid."""
    dev = torch.device("cuda", 0)
    cache = {}

    def get(case):
        if case not in cache:
            host = CASES[case]()
            images, labels, base, sl, aug, mix, lam, pad = host
            cache[case] = (host, images.to(dev), labels.to(dev),
                           base.to(dev), aug.to(dev), mix.to(dev),
                           lam.to(dev))
        return cache[case]
    return get


@pytest.mark.parametrize("channels_last", [True, False],
                         ids=["channels_last", "nchw"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_torch_definition(case, dtype, channels_last, lut,
                                         on_device):
    host, d_images, d_labels, d_base, d_aug, d_mix, d_lam = on_device(case)
    images, labels, base, sl, aug, mix, lam, pad = host
    want, want_a, want_b, want_lam = _batch_augment_cutmix_torch(
        images, labels, base[sl], aug, mix, lam, lut, pad, channels_last,
        dtype)

    idx = d_base[sl]
    assert idx.storage_offset() == sl.start
    got, got_a, got_b, got_lam = batch_augment_cutmix(
        d_images, d_labels, idx, d_aug, d_mix, d_lam, lut.to(d_images.device),
        pad, channels_last, dtype)
    assert got.dtype == dtype and got.shape == want.shape
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert got.is_contiguous(memory_format=fmt)
    assert got.stride() == want.stride()
    assert torch.equal(got.cpu(), want)
    assert got_a.dtype == got_b.dtype == torch.int64
    assert got_lam.dtype == torch.float32
    assert torch.equal(got_a.cpu(), want_a)
    assert torch.equal(got_b.cpu(), want_b)
    assert torch.equal(got_lam.cpu(), want_lam)


def test_unmixed_table_gives_batch_augment_and_eval_window_works(lut):
    """All partners -1: the images are batch_augment's, labels_b == labels_a
    and lam == 1 whatever the table says. aug=None is the identity window for
    the sample and its partner."""
    from mi355x_ddp.ops import batch_augment
    dev = torch.device("cuda", 0)
    images, labels, base, sl, aug, mix, lam, pad = _case_boxes_a()
    none = mix.clone()
    none[:, 0] = -1
    args = (images.to(dev), labels.to(dev), base.to(dev)[sl])
    got, la, lb, lo = batch_augment_cutmix(
        *args, aug.to(dev), none.to(dev), lam.to(dev), lut.to(dev), pad, True,
        torch.bfloat16)
    plain, pl = batch_augment(*args, aug.to(dev), lut.to(dev), pad, True,
                              torch.bfloat16)
    assert torch.equal(got, plain)
    assert torch.equal(la, pl) and torch.equal(lb, pl)
    assert torch.equal(lo, torch.ones_like(lo))
    got, la, lb, lo = batch_augment_cutmix(
        *args, None, mix.to(dev), lam.to(dev), lut.to(dev), pad, True,
        torch.bfloat16)
    want = _batch_augment_cutmix_torch(images, labels, base[sl], None, mix,
                                       lam, lut, pad, True, torch.bfloat16)
    assert torch.equal(got.cpu(), want[0]) and torch.equal(lb.cpu(), want[2])


def test_kernel_rejects_bad_arguments(lut):
    dev = torch.device("cuda", 0)
    images, labels = _dataset(3, 8, 8, 0)
    images, labels, lut = images.to(dev), labels.to(dev), lut.to(dev)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    mix = torch.full((3, 3), -1, dtype=torch.int32, device=dev)
    lam = torch.ones(3, device=dev)
    native = _backend.C().batch_augment_cutmix

    def call(mx=mix, lm=lam, ix=idx, pad=2):
        return native(images, labels, ix, None, mx, lm, lut, pad, True,
                      torch.bfloat16)

    with pytest.raises(RuntimeError, match="mix_i32 must be int32"):
        call(mx=mix.long())
    with pytest.raises(RuntimeError, match=r"\[M, 3\]"):
        call(mx=mix[:2])
    with pytest.raises(RuntimeError, match=r"\[M, 3\]"):
        call(mx=mix.repeat(1, 2)[:, :3])        # right shape, strided
    with pytest.raises(RuntimeError, match=r"\[M, 3\]"):
        call(mx=mix.cpu())
    with pytest.raises(RuntimeError, match="lam_f32 must be float32"):
        call(lm=lam.double())
    with pytest.raises(RuntimeError, match=r"\[M\]"):
        call(lm=lam[:2])
    with pytest.raises(RuntimeError, match="int32"):
        call(ix=idx.long())
    with pytest.raises(RuntimeError, match="pad"):
        call(pad=128)
    out, la, lb, lo = call()
    assert out.shape == (2, 3, 8, 8) and torch.equal(la, lb)


def test_device_loader_on_gpu_equals_cpu():
    """One epoch of a 64-image set, batch 24: two full batches and a short
    last one (drop_last=False), CutMix on."""
    kw = dict(batch_size=24, shuffle=True, drop_last=False, seed=5,
              augment=True, hflip=True, channels_last=True,
              out_dtype=torch.bfloat16, cutmix_alpha=1.0, cutmix_prob=0.5)
    cpu = DeviceLoader(DeviceCIFAR.synthetic(64, seed=1, device="cpu"), **kw)
    gpu = DeviceLoader(DeviceCIFAR.synthetic(64, seed=1, device="cuda:0"),
                       **kw)
    cpu.set_epoch(2)
    gpu.set_epoch(2)
    cpu_batches, gpu_batches = list(cpu), list(gpu)
    assert len(gpu) == 3 and len(gpu_batches) == len(cpu_batches) == 3
    assert [b[0].shape[0] for b in gpu_batches] == [24, 24, 16]
    differ = 0
    for (gi, gt), (ci, ct) in zip(gpu_batches, cpu_batches):
        assert gi.is_cuda and gi.dtype == torch.bfloat16
        assert gi.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(gi.cpu(), ci)
        assert len(gt) == 3 and all(t.is_cuda for t in gt)
        for g, c in zip(gt, ct):
            assert g.dtype == c.dtype and torch.equal(g.cpu(), c)
        differ += int((gt[2] < 1).sum())
    assert differ > 0          # something was mixed


def _recording(crit, losses, logits, targets):
    class Recording(torch.nn.Module):
        def forward(self, out, target):
            loss = crit(out, target)
            logits.append(out.detach().clone())
            losses.append(loss.detach().clone())
            targets.append(target)
            return loss
    return Recording()


def _two_steps(cfg, device):
    from mi355x_ddp.core.engine import train_one_epoch
    from mi355x_ddp.core.worker import build_training, init_seeds

    init_seeds(0)
    train_loader, _, sampler = build_loaders(cfg, 1, 0, distributed=False,
                                             device=device)
    assert isinstance(train_loader, DeviceLoader) and sampler is train_loader
    sampler.set_epoch(0)
    model, crit, opt, sched, scaler = build_training(
        cfg, device, 1, 0, distributed=True, wrap="flat")
    losses, logits, targets = [], [], []
    mean = train_one_epoch(model, train_loader,
                           _recording(crit, losses, logits, targets), opt, 0,
                           cfg, device, max_steps=2)
    torch.cuda.synchronize()
    assert len(losses) == 2 and mean == mean
    assert torch.isfinite(torch.stack(losses)).all()
    return losses, logits, targets


@pytest.fixture
def small_synthetic(monkeypatch):
    from mi355x_ddp.ops.conv import clear_autotune_cache
    monkeypatch.setenv("MI355X_AUTOTUNE", "0")
    monkeypatch.setattr(device_data, "SYNTHETIC_TRAIN_N", 64)
    monkeypatch.setattr(device_data, "SYNTHETIC_TEST_N", 64)
    clear_autotune_cache()
    return TrainConfig(batch_size=32, amp="bf16", channels_last=True,
                       native_ops=True, sync_bn=False, synthetic=True,
                       device_data=True, log_interval=100, stall_dump_s=None)


def test_training_with_cutmix_and_smoothing(small_synthetic):
    """Two steps of ResNet-18, bf16 channels_last: finite losses, and the
    first one is the float64 formula of the recorded logits and targets at
    the loss tolerance of tests/test_xent_mix_gpu.py."""
    device = torch.device("cuda", 0)
    cfg = small_synthetic.replace(cutmix_alpha=1.0, label_smoothing=0.1)
    losses, logits, targets = _two_steps(cfg, device)
    labels_a, labels_b, lam = targets[0]
    assert labels_a.shape == labels_b.shape == lam.shape == (32,)
    assert (lam < 1).any() and (lam == 1).any()      # prob 0.5, 32 rows
    x64 = logits[0].double()
    ce = lambda t: F.cross_entropy(x64, t, reduction="none",  # noqa: E731
                                   label_smoothing=0.1)
    want = (lam.double() * ce(labels_a)
            + (1 - lam.double()) * ce(labels_b)).mean()
    print(f"loss {float(losses[0]):.9g} want {float(want):.9g}")
    torch.testing.assert_close(losses[0].double(), want, rtol=1e-5, atol=1e-6)


def test_cutmix_that_never_mixes_is_the_plain_run_bit_for_bit(small_synthetic):
    """cutmix_prob=0 and no smoothing: the CutMix input kernel and the
    two-label loss kernels run (tuple target, lam == 1), and the first logits
    and loss are those of the plain device_data run."""
    device = torch.device("cuda", 0)
    plain = _two_steps(small_synthetic, device)
    never = _two_steps(small_synthetic.replace(cutmix_alpha=1.0,
                                               cutmix_prob=0.0), device)
    assert isinstance(plain[2][0], torch.Tensor)
    labels_a, labels_b, lam = never[2][0]
    assert torch.equal(labels_a, plain[2][0]) and torch.equal(labels_b,
                                                              labels_a)
    assert torch.equal(lam, torch.ones_like(lam))
    assert torch.equal(never[1][0], plain[1][0])
    assert torch.equal(never[0][0], plain[0][0]), (never[0][0], plain[0][0])
