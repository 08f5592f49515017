#!/usr/bin/env python3
"""Conv fwd / dgrad time with a cache-hot vs a cache-cold weight operand.

With per-call casts the bf16 weight (forward) and the rotated filter (dgrad)
are written by a small kernel right before the conv that reads them; a
persistent weight shadow (ops/conv.py) was written at the optimizer step and
comes from HBM. For every ResNet18 body shape at batch 256 this times the
conv alone (hip events, median of 12, 1 GiB cache flush before each sample,
activation operand rewritten after the flush) in both situations and prints
the per-step totals weighted by how many convs have that shape. Run on an
MI355X box; output goes to stdout.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from mi355x_ddp.ops import _backend

C = _backend.C()
DEV = "cuda"
CL = torch.channels_last
# (Cin, H, K, stride) 3x3 pad 1 at batch 256, the ResNet18 body shapes + 1x1 downsamples
SHAPES = [(64, 32, 64, 1, 3), (64, 32, 128, 2, 3), (128, 16, 128, 1, 3),
          (128, 16, 256, 2, 3), (256, 8, 256, 1, 3), (256, 8, 512, 2, 3),
          (512, 4, 512, 1, 3), (256, 8, 512, 2, 1)]
COUNT = {0: 4, 1: 1, 2: 3, 3: 1, 4: 3, 5: 1, 6: 3, 7: 1}   # convs of that shape per step
flush_buf = torch.empty(1 << 28, dtype=torch.float32, device=DEV)   # 1 GiB


def timed(fn, prep, iters=12):
    ts = []
    for _ in range(iters):
        flush_buf.fill_(1.0)
        args = prep()
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn(*args)
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


tot = {"fwd_hot": 0.0, "fwd_cold": 0.0, "dg_hot": 0.0, "dg_cold": 0.0}
for si, (cin, h, k, stride, r) in enumerate(SHAPES):
    pad = r // 2
    x = torch.randn(256, cin, h, h, device=DEV).bfloat16().contiguous(memory_format=CL)
    w32 = torch.randn(k, cin, r, r, device=DEV).contiguous(memory_format=CL)
    w16p = w32.to(torch.bfloat16)
    wTp = C.conv_build_wT(w16p)
    p = (h + 2 * pad - r) // stride + 1
    dy = torch.randn(256, k, p, p, device=DEV).bfloat16().contiguous(memory_format=CL)

    fwd = lambda xx, ww: C.conv_fwd_igemm(xx, ww, stride, pad, 0)
    dg = lambda dd, ww: C.conv_dgrad_igemm(dd, ww, h, h, stride, pad, 0)
    f_hot = timed(fwd, lambda: (x.clone(memory_format=torch.preserve_format), w32.to(torch.bfloat16)))
    f_cold = timed(fwd, lambda: (x.clone(memory_format=torch.preserve_format), w16p))
    d_hot = timed(dg, lambda: (dy.clone(memory_format=torch.preserve_format), C.conv_build_wT(w16p)))
    d_cold = timed(dg, lambda: (dy.clone(memory_format=torch.preserve_format), wTp))
    n = COUNT[si]
    tot["fwd_hot"] += n * f_hot
    tot["fwd_cold"] += n * f_cold
    tot["dg_hot"] += n * d_hot
    tot["dg_cold"] += n * d_cold
    print(f"C{cin} H{h} K{k} s{stride} r{r} x{n}: fwd hot {f_hot:6.1f} cold {f_cold:6.1f} us | "
          f"dgrad hot {d_hot:6.1f} cold {d_cold:6.1f} us", flush=True)
print("per step (weighted by conv count): " +
      ", ".join(f"{k} {v:.1f} us" for k, v in tot.items()))
