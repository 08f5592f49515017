#!/usr/bin/env python3
"""What LARS, gradient-norm clipping and the weight EMA cost in the optimizer
step.

Times FusedSGD.step() alone, on one GPU, on the parameter sets of ResNet-18
and ResNet-50 (fp32, channels_last, momentum 0.9, weight decay 1e-4) with
random gradients. Variants:

  plain   both features off: the step as it has always been
  clip    clip_grad_norm on
  lars    LARS on
  both    both on
  ema          the weight average fused into the step (ema_decay 0.999)
  ema_foreach  the plain step, then torch._foreach_lerp_ over the same
               tensors: what the fused average replaces, and its yardstick

each also with bf16 conv weight shadows live ("+shadows": the step then
stores the rounded weights and rotates them, as it does under --amp bf16).
The shadows come from one forward of the model under bf16 autocast.

A window is --steps steps between two device events, after --warmup steps;
every variant gets --repeats windows, the variants alternating. One JSON line
per variant: the windows' microseconds per step (all of them, so the spread
shows, and their median), and the kernel launches of one step as the
profiler counts them. --variants plain runs on a tree from before the
features existed, for a baseline from the same session.

The learning rate is 1e-9 so that hundreds of steps on the same gradients
leave the weights where they are; the arithmetic does not depend on it.

Usage: python tools/bench_optimizer.py [--archs resnet18,resnet50]
           [--variants plain,clip,lars,both,ema,ema_foreach] [--steps 200]
           [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from mi355x_ddp.models import build_model
from mi355x_ddp.ops import FusedSGD, MI355Conv2d
from mi355x_ddp.ops.conv import shadow_of
from mi355x_ddp.ops.pool import MI355MaxPool2d

FEATURES = {
    "plain": {},
    "clip": dict(clip_grad_norm=1.0),
    "lars": dict(lars=True),
    "both": dict(lars=True, clip_grad_norm=1.0),
    "ema": dict(ema_decay=0.999),
    "ema_foreach": {},
}
EMA_DECAY = 0.999


class StepThenLerp:
    """The plain fused step followed by the per-tensor average in torch."""

    def __init__(self, opt, params):
        self.opt = opt
        self.params = [p.detach() for p in params]
        self.emas = [p.detach().clone() for p in params]

    def step(self):
        self.opt.step()
        torch._foreach_lerp_(self.emas, self.params, 1.0 - EMA_DECAY)


def parse_args():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--archs", default="resnet18,resnet50")
    p.add_argument("--variants",
                   default="plain,clip,lars,both,ema,ema_foreach")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--label", default="",
                   help="copied into every line (which tree was measured)")
    return p.parse_args()


def build(arch, device, shadows):
    """(model, number of live shadows) with a random gradient on every
    parameter."""
    torch.manual_seed(0)
    model = build_model(arch, 100).to(device)
    model = MI355MaxPool2d.convert(MI355Conv2d.convert(model))
    model = model.to(memory_format=torch.channels_last)
    model.train()
    if shadows:
        x = torch.randn(8, 3, 32, 32, device=device) \
            .to(memory_format=torch.channels_last)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            model(x)
    for p in model.parameters():
        p.grad = torch.randn_like(p) * 0.01
    live = sum(shadow_of(p) is not None for p in model.parameters())
    assert (live > 0) == shadows, live
    return model, live


def launches(opt):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    # the optimizer's own "Optimizer.step#..." span shows up on the device
    # side as well and is not a launch
    return sum(e.device_type == torch.autograd.DeviceType.CUDA and
               not e.name.startswith("Optimizer.step#")
               for e in prof.events())


def window(opt, steps):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        opt.step()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / steps


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optimizer.py measures on a GPU and found none")
    device = torch.device("cuda", 0)
    for arch in args.archs.split(","):
        for shadows in (False, True):
            model, live = build(arch, device, shadows)
            params = list(model.parameters())
            opts = {}
            for name in args.variants.split(","):
                # every variant steps the same parameters; each has its own
                # momentum buffers
                opts[name] = FusedSGD(params, lr=1e-9, momentum=0.9,
                                      weight_decay=1e-4, **FEATURES[name])
                if name == "ema_foreach":
                    opts[name] = StepThenLerp(opts[name], params)
            counts = {}
            for name, opt in opts.items():
                for _ in range(args.warmup):
                    opt.step()
                counts[name] = launches(opt)
            times = {name: [] for name in opts}
            for _ in range(args.repeats):
                for name, opt in opts.items():
                    times[name].append(window(opt, args.steps))
            for name in opts:
                row = {"arch": arch,
                       "variant": name + ("+shadows" if shadows else ""),
                       "tensors": len(params),
                       "elements": sum(p.numel() for p in params),
                       "shadows": live,
                       "launches_per_step": counts[name],
                       "us_per_step_median":
                           round(statistics.median(times[name]), 2),
                       "us_per_step": [round(t, 2) for t in times[name]],
                       "steps": args.steps, "repeats": args.repeats}
                if args.label:
                    row["label"] = args.label
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
