#!/usr/bin/env python3
"""What the input pipeline costs: DataLoader path against --device_data.

bench.py reuses eight prefabricated batches, so its figure excludes the input
pipeline. This tool measures, on one GPU, for resnet18 / bf16 / channels_last
at batch 256 (the flagship configuration):

  input_only   images/s of the input path with no training behind it
               loader: build_loaders' DataLoader (cfg.num_workers workers),
                       plus the host-to-device copy and the channels_last
                       conversion the engine does per step
               device: DeviceLoader, whole epochs including set_epoch
               device+cutmix: the same with CutMix (--cutmix_alpha,
                       --cutmix_prob; by default every sample is mixed, the
                       most the kernel can be asked to read)
  train_epoch  steps/s of engine.train_one_epoch, the first --discard steps
               left out, fed by
               static: eight pinned prefabricated batches (what bench.py
                       times, run through the same engine loop)
               loader: the DataLoader path
               device: the --device_data path
               device+cutmix: the --device_data path with CutMix, the loss
                       taking (labels_a, labels_b, lam)

Every measurement is repeated --repeats times, the variants alternating, and
printed as one JSON line each so the spread is visible. Windows end in a
device synchronise. Worker count comes from --num_workers (cfg.num_workers);
nothing is sized by the machine's CPU count.

Usage: python tools/bench_input.py [--steps 60] [--discard 10] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from mi355x_ddp.config import TrainConfig
from mi355x_ddp.core.engine import train_one_epoch
from mi355x_ddp.core.worker import build_training, init_seeds
from mi355x_ddp.data import build_loaders


def parse_args():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--arch", default="resnet18")
    p.add_argument("--amp", default="bf16")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--steps", type=int, default=60,
                   help="train_one_epoch steps per measurement")
    p.add_argument("--discard", type=int, default=10,
                   help="leading steps/batches left out of every window")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--loader_batches", type=int, default=60,
                   help="batches per input_only measurement of the loader")
    p.add_argument("--device_epochs", type=int, default=3,
                   help="whole epochs per input_only measurement of the "
                        "device path")
    p.add_argument("--cutmix_alpha", type=float, default=1.0,
                   help="Beta parameter of the device+cutmix variant")
    p.add_argument("--cutmix_prob", type=float, default=1.0,
                   help="share of samples the device+cutmix variant mixes")
    p.add_argument("--no-channels-last", dest="channels_last",
                   action="store_false", default=True)
    p.add_argument("--rehearse", action="store_true",
                   help="run without a GPU to check the plumbing; rows are "
                        "marked and are not measurements")
    return p.parse_args()


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


class Window:
    """Hands out `steps` batches of `source` (restarting it when it runs out)
    and opens the timed window when batch number `discard` is asked for,
    i.e. after `discard` whole steps. The caller closes it."""

    def __init__(self, source, steps, discard, device):
        self.source, self.steps, self.discard = source, steps, discard
        self.device = device
        self.t0 = None

    def __len__(self):
        return self.steps

    def __iter__(self):
        it = iter(self.source)
        for i in range(self.steps):
            if i == self.discard:
                sync(self.device)
                self.t0 = time.perf_counter()
            try:
                batch = next(it)
            except StopIteration:
                it = iter(self.source)
                batch = next(it)
            yield batch

    def close(self):
        sync(self.device)
        return time.perf_counter() - self.t0


def input_only_loader(loader, cfg, device, batches, discard):
    win = Window(loader, batches + discard, discard, device)
    for images, labels in win:
        images = images.to(device, non_blocking=True)
        labels = labels.to(device, non_blocking=True)
        if cfg.channels_last:
            images = images.to(memory_format=torch.channels_last)
    return batches * cfg.batch_size / win.close(), batches


def input_only_device(loader, cfg, device, epochs, first_epoch):
    sync(device)
    t0 = time.perf_counter()
    n = 0
    for e in range(epochs):
        loader.set_epoch(first_epoch + e)
        for images, labels in loader:
            n += 1
    sync(device)
    return n * cfg.batch_size / (time.perf_counter() - t0), n


def train_window(source, model, crit, opt, cfg, device, steps, discard):
    win = Window(source, steps, discard, device)
    train_one_epoch(model, win, crit, opt, 0, cfg, device, max_steps=steps)
    elapsed = win.close()
    timed = steps - discard
    return timed / elapsed, timed


def main():
    args = parse_args()
    if torch.cuda.is_available():
        device = torch.device("cuda", 0)
    elif args.rehearse:
        device = torch.device("cpu")
    else:
        sys.exit("bench_input.py measures on a GPU and found none "
                 "(--rehearse checks the plumbing without one)")
    init_seeds(1)
    cfg = TrainConfig(arch=args.arch, batch_size=args.batch_size,
                      amp=args.amp, channels_last=args.channels_last,
                      sync_bn=False, synthetic=True,
                      num_workers=args.num_workers,
                      # one loss materialisation per window, at step 0
                      log_interval=1 << 30)
    cfg_dev = cfg.replace(device_data=True)
    cfg_mix = cfg_dev.replace(cutmix_alpha=args.cutmix_alpha,
                              cutmix_prob=args.cutmix_prob)
    base = {"arch": cfg.arch, "amp": cfg.amp, "batch": cfg.batch_size,
            "channels_last": cfg.channels_last,
            "num_workers": cfg.num_workers, "device": device.type}
    if device.type != "cuda":
        base["rehearsal"] = True

    def emit(**row):
        print(json.dumps({**row, **base}), flush=True)

    old_loader, _, _ = build_loaders(cfg, 1, 0, distributed=False)
    new_loader, _, _ = build_loaders(cfg_dev, 1, 0, distributed=False,
                                     device=device)
    mix_loader, _, _ = build_loaders(cfg_mix, 1, 0, distributed=False,
                                     device=device)

    gen = torch.Generator().manual_seed(123)
    static = []
    for _ in range(8):
        img = torch.randn(cfg.batch_size, 3, cfg.image_size, cfg.image_size,
                          generator=gen)
        lbl = torch.randint(0, cfg.num_classes, (cfg.batch_size,),
                            generator=gen)
        if device.type == "cuda":
            img, lbl = img.pin_memory(), lbl.pin_memory()
        static.append((img, lbl))

    # ---- input path alone -------------------------------------------------
    for r in range(args.repeats):
        ips, n = input_only_loader(old_loader, cfg, device,
                                   args.loader_batches, args.discard)
        emit(row="input_only", path="loader", repeat=r, batches=n,
             images_per_sec=round(ips, 1))
        ips, n = input_only_device(new_loader, cfg, device,
                                   args.device_epochs,
                                   r * args.device_epochs)
        emit(row="input_only", path="device", repeat=r, batches=n,
             images_per_sec=round(ips, 1))
        ips, n = input_only_device(mix_loader, cfg, device,
                                   args.device_epochs,
                                   r * args.device_epochs)
        emit(row="input_only", path="device+cutmix", repeat=r, batches=n,
             images_per_sec=round(ips, 1), cutmix_alpha=cfg_mix.cutmix_alpha,
             cutmix_prob=cfg_mix.cutmix_prob)

    # ---- the training loop fed four ways ----------------------------------
    model, crit, opt, sched, scaler = build_training(
        cfg, device, 1, 0, distributed=True, wrap="flat")
    sources = (("static", static, cfg), ("loader", old_loader, cfg),
               ("device", new_loader, cfg_dev),
               ("device+cutmix", mix_loader, cfg_mix))
    # every path once untimed: kernel selection, code objects, workers
    for name, source, run_cfg in sources:
        train_window(source, model, crit, opt, run_cfg, device,
                     args.discard + 2, args.discard)
    for r in range(args.repeats):
        for name, source, run_cfg in sources:
            sps, n = train_window(source, model, crit, opt, run_cfg, device,
                                  args.steps, args.discard)
            emit(row="train_epoch", path=name, repeat=r, steps=n,
                 steps_per_sec=round(sps, 2),
                 ms_per_step=round(1000.0 / sps, 3),
                 images_per_sec=round(sps * cfg.batch_size, 1))
    del old_loader   # shuts the persistent workers down


if __name__ == "__main__":
    main()
