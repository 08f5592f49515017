#!/usr/bin/env python3
"""Time `se_add_relu` on the native kernels against its torch definition
(`MI355X_NATIVE_SE=0`) at the four SE-ResNet-50 CIFAR stage shapes, batch 256.

    python tools/bench_se.py [--dtype bf16|fp16] [--iters 200] [--once]

The two paths alternate in one process and are timed with device events around
`--iters` forward+backward calls. The last columns are the bytes the four
activation-sized kernels must move, from the shapes: squeeze reads u;
scale_add_relu reads u and identity and writes out; bwd_reduce reads dout, out
and u; bwd_apply reads dout and out and writes du and d_identity. Divide by
the kernel times of a kernel trace (`--once` runs each shape three times per
path, which is what to trace).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from mi355x_ddp.ops import SqueezeExcite, se_add_relu

SHAPES = [(256, 256, 32), (256, 512, 16), (256, 1024, 8), (256, 2048, 4)]


def run(u, idn, se, dout, native):
    os.environ["MI355X_NATIVE_SE"] = "1" if native else "0"
    u.grad = idn.grad = None
    se_add_relu(u, idn, se).backward(dout)


def timed(args, native, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(iters):
        run(*args, native)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--once", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "bench_se.py needs a GPU"
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    print(f"{'N x C x HW':>18} {'native us':>10} {'torch us':>10} {'ratio':>6}"
          f" {'squeeze MB':>11} {'scale MB':>9} {'reduce MB':>10}"
          f" {'apply MB':>9}")
    for N, C, px in SHAPES:
        torch.manual_seed(0)
        se = SqueezeExcite(C).cuda()
        act = lambda: torch.randn(N, C, px, px, device="cuda", dtype=dt) \
            .contiguous(memory_format=torch.channels_last)
        args = (act().requires_grad_(True), act().requires_grad_(True), se,
                act())
        if a.once:
            for native in (True, True, True, False, False, False):
                run(*args, native)
            torch.cuda.synchronize()
            continue
        for native in (True, False):
            timed(args, native, 20)
        t = {True: [], False: []}
        for _ in range(3):
            for native in (True, False):
                t[native].append(timed(args, native, a.iters))
        nat, ref = min(t[True]), min(t[False])
        mb = args[0].numel() * 2 / 1e6
        print(f"{f'{N} x {C} x {px}^2':>18} {nat:10.1f} {ref:10.1f} "
              f"{ref / nat:6.2f} {mb:11.1f} {3 * mb:9.1f} {3 * mb:10.1f} "
              f"{4 * mb:9.1f}")


if __name__ == "__main__":
    main()
