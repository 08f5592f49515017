#!/usr/bin/env python3
"""What one evaluation batch costs, with the fused evaluation forward and
without it.

Times the loop body of `engine.validate` on one GPU: forward under autocast,
loss, top-1/top-5 accuracy, on random images, model in eval mode with
randomized BatchNorm statistics. Two variants run in ONE process on the same
model and batch and alternate window by window:

  unfused   the forward as it runs without --fused_eval
  fused     the same forward inside core.inference.fused_inference

Configurations (--configs picks by name):

  r18-bf16, r18-fp16, r50-bf16, r50-fp16   ResNet-18/50, CIFAR shapes
                                           (32 px), batch 256, channels_last
  r50i-bf16                                resnet50_imagenet, 224 px, batch 64

Every configuration is warmed first (which also runs the per-shape autotune of
both variants), then gets --repeats windows of --steps batches per variant
between two device events. One JSON line per configuration: all windows in ms
per batch (so the spread shows), the medians, their ratio, and what one pass
over --eval_batches such batches costs relative to --epoch_s seconds of
training. The per-layer choices of the tuner (`tune_report`) go to stderr.

Usage: python tools/bench_eval.py [--configs r18-bf16,r50-bf16] [--steps 20]
           [--warmup 5] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

CONFIGS = {
    # name: (arch, image size, batch, autocast dtype)
    "r18-bf16": ("resnet18", 32, 256, "bf16"),
    "r18-fp16": ("resnet18", 32, 256, "fp16"),
    "r50-bf16": ("resnet50", 32, 256, "bf16"),
    "r50-fp16": ("resnet50", 32, 256, "fp16"),
    "r50i-bf16": ("resnet50_imagenet", 224, 64, "bf16"),
}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--steps", type=int, default=20,
                   help="batches per timed window")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--eval_batches", type=int, default=40,
                   help="batches of one evaluation pass (CIFAR test set at "
                        "batch 256)")
    p.add_argument("--epoch_s", type=float, default=0.9,
                   help="seconds of one training epoch, for the ratio")
    p.add_argument("--label", default="",
                   help="copied into every line (which tree was measured)")
    args = p.parse_args(argv)
    args.configs = args.configs.split(",")
    unknown = [c for c in args.configs if c not in CONFIGS]
    if unknown:
        p.error(f"unknown configs {unknown}; choose from {sorted(CONFIGS)}")
    return args


def randomize_bn(model, seed=1):
    """A fresh model's BatchNorm folds to the identity; give every layer
    statistics and affine parameters of its own."""
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                dev = m.weight.device
                m.running_mean.copy_((torch.randn(c, generator=g) * 0.1).to(dev))
                m.running_var.copy_((0.5 + torch.rand(c, generator=g)).to(dev))
                m.weight.copy_((0.5 + 0.5 * torch.rand(c, generator=g)).to(dev))
                m.bias.copy_((torch.randn(c, generator=g) * 0.1).to(dev))


def build(arch, device):
    from mi355x_ddp.models import build_model
    from mi355x_ddp.ops import MI355Conv2d
    from mi355x_ddp.ops.pool import MI355MaxPool2d

    torch.manual_seed(0)
    model = build_model(arch, 100).to(device)
    model = MI355MaxPool2d.convert(MI355Conv2d.convert(model))
    model = model.to(memory_format=torch.channels_last)
    randomize_bn(model)
    return model.eval()


def measure(name, args, device):
    from mi355x_ddp.core.amp import autocast_ctx
    from mi355x_ddp.core.inference import fused_inference
    from mi355x_ddp.core.metrics import accuracy
    from mi355x_ddp.ops import fused_eval
    from mi355x_ddp.ops.xent import SoftmaxCrossEntropy

    arch, size, batch, amp = CONFIGS[name]
    model = build(arch, device)
    crit = SoftmaxCrossEntropy(0.0).to(device)
    g = torch.Generator().manual_seed(2)
    images = torch.randn(batch, 3, size, size, generator=g).to(device) \
        .contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, 100, (batch,), generator=g).to(device)

    def batch_step():
        with autocast_ctx(amp, "cuda"):
            out = model(images)
            loss = crit(out, labels)
        return loss, accuracy(out.float(), labels, topk=(1, 5))

    def window(fused, steps):
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        ctx = fused_inference(model) if fused else torch.no_grad()
        with torch.no_grad(), ctx:
            start.record()
            for _ in range(steps):
                batch_step()
            stop.record()
            stop.synchronize()
        return start.elapsed_time(stop) / steps

    fused_eval.calls.reset()
    for fused in (False, True):
        window(fused, args.warmup)
    counts = (fused_eval.calls.fused, fused_eval.calls.unfused,
              fused_eval.calls.fallback)
    times = {False: [], True: []}
    for _ in range(args.repeats):
        for fused in (False, True):
            times[fused].append(window(fused, args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    per_batch = max(1, args.warmup)
    row = {"config": name, "arch": arch, "image_size": size, "batch": batch,
           "amp": amp,
           "unfused_ms_per_batch": [round(t, 4) for t in times[False]],
           "fused_ms_per_batch": [round(t, 4) for t in times[True]],
           "unfused_ms_median": round(med[False], 4),
           "fused_ms_median": round(med[True], 4),
           "fused_over_unfused": round(med[True] / med[False], 4),
           "layers_fused_kernel": counts[0] // per_batch,
           "layers_unfused_candidate": counts[1] // per_batch,
           "layers_fallback": counts[2] // per_batch,
           "eval_pass_ms_unfused": round(med[False] * args.eval_batches, 2),
           "eval_pass_ms_fused": round(med[True] * args.eval_batches, 2),
           "eval_pass_over_epoch_unfused":
               round(med[False] * args.eval_batches / (args.epoch_s * 1e3), 4),
           "eval_pass_over_epoch_fused":
               round(med[True] * args.eval_batches / (args.epoch_s * 1e3), 4),
           "steps": args.steps, "repeats": args.repeats}
    if args.label:
        row["label"] = args.label
    print(json.dumps(row), flush=True)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_eval.py measures on a GPU and found none")
    from mi355x_ddp.ops.conv import clear_autotune_cache, tune_report

    device = torch.device("cuda", 0)
    for name in args.configs:
        clear_autotune_cache()
        measure(name, args, device)
        print(f"--- tuner choices, {name}\n{tune_report()}", file=sys.stderr,
              flush=True)


if __name__ == "__main__":
    main()
