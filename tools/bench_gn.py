#!/usr/bin/env python3
"""Time `gn_add_relu` (forward + backward) on the kernels of
csrc/group_norm.hip at the distinct norm-layer shapes of resnet50 (32 px,
batch 256) and resnet50_imagenet (224 px, batch 64), 32 groups, against

  - the same kernels streaming from global memory (`MI355X_GN_RESIDENT=0`),
  - the torch definition (`MI355X_NATIVE_GN=0`),
  - `bn_add_relu` (training BatchNorm) on the same tensors.

    python tools/bench_gn.py [--dtype bf16|fp16] [--iters 30] [--set cifar|imagenet|all]

The four alternate in one process and are timed with device events around
`--iters` forward+backward calls; the best of three windows is printed. `MB`
is what the resident kernels must move, from the shapes: the forward reads x
and the residual and writes y, the backward reads dy, y and x and writes dx
and d_residual (8 activations). `fwd`/`bwd` name the variant the host picks:
r<CAP> resident with that capacity, s streaming, /32 the 32-channel chunk.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn as nn

from mi355x_ddp.ops import bn_add_relu, gn_add_relu

# (N, C, px) of every distinct conv output that a norm layer reads
CIFAR = [(256, c, px) for c, px in [
    (64, 32), (256, 32), (128, 32), (128, 16), (512, 16), (256, 16), (256, 8),
    (1024, 8), (512, 8), (512, 4), (2048, 4)]]
IMAGENET = [(64, c, px) for c, px in [
    (64, 112), (64, 56), (256, 56), (128, 56), (128, 28), (512, 28),
    (256, 28), (256, 14), (1024, 14), (512, 14), (512, 7), (2048, 7)]]
VARIANTS = ["native", "streaming", "torch", "bn"]


def variants_of(C, hw, groups):
    """The (fwd, bwd) kernel variants launch_fwd / launch_bwd pick."""
    cap = lambda caps: next((f"r{c}" for c in caps if hw <= c), None)
    fwd = cap((64, 256, 1024)) or "s"
    bwd = cap((64, 256, 576))
    if bwd is None:
        bwd = "r1152/32" if hw <= 1152 and C // groups <= 32 else "s"
    return fwd, bwd


def run(x, idn, gn, bn, dout, variant):
    os.environ["MI355X_NATIVE_GN"] = "0" if variant == "torch" else "1"
    os.environ["MI355X_GN_RESIDENT"] = "0" if variant == "streaming" else "1"
    x.grad = idn.grad = None
    if variant == "bn":
        bn_add_relu(x, idn, bn).backward(dout)
    else:
        gn_add_relu(x, idn, gn).backward(dout)


def timed(args, variant, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        run(*args, variant)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--groups", type=int, default=32)
    p.add_argument("--set", default="all", choices=["cifar", "imagenet", "all"])
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_gn.py needs a GPU"
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    shapes = {"cifar": CIFAR, "imagenet": IMAGENET,
              "all": CIFAR + IMAGENET}[a.set]
    print(f"| {'N x C x HW':>18} | {'fwd':>5} | {'bwd':>8} | "
          + " | ".join(f"{v + ' us':>12}" for v in VARIANTS)
          + f" | {'MB':>7} | {'native GB/s':>11} |")
    print("|" + "---|" * (5 + len(VARIANTS)))
    for N, C, px in shapes:
        torch.manual_seed(0)
        gn = nn.GroupNorm(min(a.groups, C // 2), C).cuda()
        bn = nn.BatchNorm2d(C).cuda().train()
        act = lambda: torch.randn(N, C, px, px, device="cuda", dtype=dt) \
            .contiguous(memory_format=torch.channels_last)
        args = (act().requires_grad_(True), act().requires_grad_(True), gn,
                bn, act())
        for v in VARIANTS:
            timed(args, v, 3)
        t = {v: [] for v in VARIANTS}
        for _ in range(3):
            for v in VARIANTS:
                t[v].append(timed(args, v, a.iters))
        best = {v: min(t[v]) for v in VARIANTS}
        mb = 8 * args[0].numel() * 2 / 1e6
        fwd, bwd = variants_of(C, px * px, gn.num_groups)
        print(f"| {f'{N} x {C} x {px}^2':>18} | {fwd:>5} | {bwd:>8} | "
              + " | ".join(f"{best[v]:12.1f}" for v in VARIANTS)
              + f" | {mb:7.1f} | {mb / best['native'] * 1e3:11.0f} |",
              flush=True)
        del args


if __name__ == "__main__":
    main()
