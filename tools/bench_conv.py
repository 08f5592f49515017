#!/usr/bin/env python3
"""Per-shape micro-benchmark: native implicit-GEMM conv vs MIOpen (F.conv2d).

Times fwd / dgrad / wgrad for every conv shape of a model config at the bench
batch size, channels_last in bf16 or fp16 (--dtype), and prints a table with
speedups. Run on an
MI355X box; output goes to stdout (redirect into gpurun_out/).

Default: the ResNet18 CIFAR table (round-1 baseline format). --arch/--image-
size collects the shape set from the actual model with forward hooks, e.g.
`--arch resnet50 --image-size 224 --batch 64` for BASELINE config 5.

The fwd / dgrad `best` column also sweeps the split-K candidates of the
128x128 tile that the tuner would offer for the shape (cfg `(228, s)`); for
each one it runs, a `# splitk` line gives its time and its relative error
norm(a-b)/norm(b) against the unsplit tile=228 output of the same operands.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn as nn
import torch.nn.functional as F


def timeit(fn, warmup=5, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


R18_CIFAR_SHAPES = [
    # (name, C, H, W, K, R, stride, pad)
    ("stem 3x3", 3, 32, 32, 64, 3, 1, 1),
    ("s1 3x3", 64, 32, 32, 64, 3, 1, 1),
    ("s2 3x3/2", 64, 32, 32, 128, 3, 2, 1),
    ("s2 1x1/2", 64, 32, 32, 128, 1, 2, 0),
    ("s2 3x3", 128, 16, 16, 128, 3, 1, 1),
    ("s3 3x3/2", 128, 16, 16, 256, 3, 2, 1),
    ("s3 3x3", 256, 8, 8, 256, 3, 1, 1),
    ("s4 3x3/2", 256, 8, 8, 512, 3, 2, 1),
    ("s4 3x3", 512, 4, 4, 512, 3, 1, 1),
]


def collect_model_shapes(arch: str, image_size: int):
    """Unique conv shapes (with multiplicities) of a model at this input
    size, discovered by a CPU forward pass with hooks."""
    from mi355x_ddp.models import build_model
    model = build_model(arch)
    shapes = {}  # (C,H,W,K,R,stride,pad) -> count

    def hook(mod, inp, out):
        x = inp[0]
        key = (x.shape[1], x.shape[2], x.shape[3], mod.out_channels,
               mod.kernel_size[0], mod.stride[0], mod.padding[0])
        shapes[key] = shapes.get(key, 0) + 1

    handles = [m.register_forward_hook(hook) for m in model.modules()
               if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        model(torch.zeros(1, 3, image_size, image_size))
    for h in handles:
        h.remove()
    out = []
    for (c, h, w, k, r, s, p), cnt in shapes.items():
        tag = f"{r}x{r}" + (f"/{s}" if s > 1 else "")
        out.append((f"{c}->{k} {tag}@{h}", c, h, w, k, r, s, p, cnt))
    return out


# The grouped 3x3 layers of ResNeXt-50 32x4d on CIFAR input (32 groups), in
# their stride-1 and stride-2 forms: (name, C, H = W of the input, stride)
RESNEXT50_GROUPED_SHAPES = [
    ("s1 128g32", 128, 32, 1),
    ("s2 256g32/2", 256, 32, 2),
    ("s2 256g32", 256, 16, 1),
    ("s3 512g32/2", 512, 16, 2),
    ("s3 512g32", 512, 8, 1),
    ("s4 1024g32/2", 1024, 8, 2),
    ("s4 1024g32", 1024, 4, 1),
]


def bench_grouped(args, dtype):
    """Native grouped kernels against MIOpen, per pass. Each cell is the
    median of `--windows` timeit windows, with the spread (max - min) / median
    of the native windows; GB/s is the pass's compulsory traffic (x read and y
    written once for fwd / dgrad, x and dy read once for wgrad) over the
    native time."""
    from mi355x_ddp import _C
    N, groups = args.batch, 32
    kw = dict(warmup=args.warmup, iters=args.iters)

    def windows(fn):
        ts = sorted(timeit(fn, **kw) for _ in range(args.windows))
        return ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[len(ts) // 2]

    print(f"{'shape':>14} {'pass':>6} {'MIOpen us':>10} {'native us':>10} "
          f"{'spread':>7} {'cfg':>10} {'x':>6} {'GB/s':>7}")
    for name, c, h, stride in RESNEXT50_GROUPED_SHAPES:
        x = torch.randn(N, c, h, h, device="cuda", dtype=dtype) \
            .to(memory_format=torch.channels_last)
        wt = (torch.randn(c, c // groups, 3, 3, device="cuda", dtype=dtype)
              / (9 * c // groups) ** 0.5).to(memory_format=torch.channels_last)
        y = F.conv2d(x, wt, None, stride, 1, 1, groups)
        dy = torch.randn_like(y).to(memory_format=torch.channels_last)
        wp, wpT = _C.conv_grouped_prep(wt, groups)
        act_bytes = 2.0 * (x.numel() + y.numel())

        def miopen_bwd(mask):
            return torch.ops.aten.convolution_backward(
                dy, x, wt, None, [stride, stride], [1, 1], [1, 1], False,
                [0, 0], groups, mask)

        def row(pss, tm, tn, spread, cfg):
            print(f"{name:>14} {pss:>6} {tm:10.1f} {tn:10.1f} {spread:7.1%} "
                  f"{cfg:>10} {tm/tn:6.2f} {act_bytes/tn/1e3:7.1f}",
                  flush=True)

        # the forward includes the per-call prep, as _ConvGrouped runs it
        tm, _ = windows(lambda: F.conv2d(x, wt, None, stride, 1, 1, groups))
        tn, sp = windows(lambda: _C.conv_grouped_fwd(
            x, _C.conv_grouped_prep(wt, groups)[0], stride))
        row("fwd", tm, tn, sp, "prep+fwd")
        tm, _ = windows(lambda: miopen_bwd([True, False, False]))
        tn, sp = windows(lambda: _C.conv_grouped_dgrad(dy, wpT, h, h, stride))
        row("dgrad", tm, tn, sp, "")
        tm, _ = windows(lambda: miopen_bwd([False, True, False]))
        best = min((windows(lambda: _C.conv_grouped_wgrad(
            dy, x, groups, stride, s)) + (f"splits {s}",) for s in (0, 1, 32)))
        row("wgrad", tm, best[0], best[1], best[2])
        del x, wt, y, dy, wp, wpT


# The 13 depthwise layers of MobileNet-v1: (C, stride, multiplicity), in model
# order; the input extent is --image-size (after the stem) divided by the
# strides before the layer. --depthwise times every layer at both strides.
MOBILENET_DW_LAYERS = [(32, 1, 1), (64, 2, 1), (128, 1, 1), (128, 2, 1),
                       (256, 1, 1), (256, 2, 1), (512, 1, 5), (512, 2, 1),
                       (1024, 1, 1)]


def bench_depthwise(args, dtype):
    """Native depthwise kernels against MIOpen, per pass, on the MobileNet-v1
    depthwise shapes, each at stride 1 and 2 (`*` marks the stride the model
    uses). The two sides alternate window by window; a cell is the median of
    `--windows` windows and `spread` is (max - min) / median of the native
    ones. GB/s is the compulsory traffic over the native time. Then the
    mobilenet_v1 training step with MI355X_NATIVE_DEPTHWISE=1 against =0,
    alternating in the same way."""
    from mi355x_ddp import _C
    N = args.batch
    kw = dict(warmup=args.warmup, iters=args.iters)

    def alternate(fa, fb):
        ta, tb = [], []
        for _ in range(args.windows):
            ta.append(timeit(fa, **kw))
            tb.append(timeit(fb, **kw))
        ta.sort(), tb.sort()
        m = len(ta) // 2
        return ta[m], tb[m], (tb[-1] - tb[0]) / tb[m]

    print(f"{'shape':>16} {'pass':>6} {'MIOpen us':>10} {'native us':>10} "
          f"{'spread':>7} {'cfg':>10} {'x':>6} {'GB/s':>7}")
    used, h = {}, args.image_size   # (C, extent) -> the strides the model has
    for c, model_stride, _ in MOBILENET_DW_LAYERS:
        used.setdefault((c, h), set()).add(model_stride)
        h = (h - 1) // model_stride + 1
    for (c, h), model_strides in used.items():
        for stride in (1, 2):
            mark = "*" if stride in model_strides else ""
            name = f"{c}@{h}" + ("/2" if stride == 2 else "") + mark
            x = torch.randn(N, c, h, h, device="cuda", dtype=dtype) \
                .to(memory_format=torch.channels_last)
            wt = (torch.randn(c, 1, 3, 3, device="cuda", dtype=dtype) / 3)
            y = F.conv2d(x, wt, None, stride, 1, 1, c)
            dy = torch.randn_like(y).to(memory_format=torch.channels_last)
            act_bytes = 2.0 * (x.numel() + y.numel())

            def miopen_bwd(mask):
                return torch.ops.aten.convolution_backward(
                    dy, x, wt, None, [stride, stride], [1, 1], [1, 1], False,
                    [0, 0], c, mask)

            def row(pss, tm, tn, spread, cfg=""):
                print(f"{name:>16} {pss:>6} {tm:10.1f} {tn:10.1f} "
                      f"{spread:7.1%} {cfg:>10} {tm/tn:6.2f} "
                      f"{act_bytes/tn/1e3:7.1f}", flush=True)

            row("fwd", *alternate(
                lambda: F.conv2d(x, wt, None, stride, 1, 1, c),
                lambda: _C.conv_dw_fwd(x, wt, stride)))
            row("dgrad", *alternate(
                lambda: miopen_bwd([True, False, False]),
                lambda: _C.conv_dw_dgrad(dy, wt, h, h, stride)))
            cells = []   # (native, MIOpen, spread, cfg), the fastest first
            for s in (0, 8, 64):
                tm, tn, sp = alternate(
                    lambda: miopen_bwd([False, True, False]),
                    lambda: _C.conv_dw_wgrad(dy, x, stride, s))
                cells.append((tn, tm, sp, f"splits {s}"))
            tn, tm, sp, cfg = min(cells)
            row("wgrad", tm, tn, sp, cfg)
            del x, wt, y, dy

    # the training step, forward + backward + SGD, tuner off on both sides
    from mi355x_ddp.models import build_model
    from mi355x_ddp.ops.conv import MI355Conv2d
    os.environ["MI355X_AUTOTUNE"] = "0"
    model = MI355Conv2d.convert(build_model("mobilenet_v1", 100).cuda()) \
        .to(memory_format=torch.channels_last).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    xb = torch.randn(N, 3, args.image_size, args.image_size, device="cuda") \
        .to(memory_format=torch.channels_last)
    lb = torch.randint(0, 100, (N,), device="cuda")

    def step(native):
        os.environ["MI355X_NATIVE_DEPTHWISE"] = native
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype):
            loss = F.cross_entropy(model(xb).float(), lb)
        loss.backward()
        opt.step()

    t0, t1, sp = alternate(lambda: step("0"), lambda: step("1"))
    print(f"# mobilenet_v1 step, batch {N}, {args.image_size} px: "
          f"MI355X_NATIVE_DEPTHWISE=0 {t0/1e3:.2f} ms, =1 {t1/1e3:.2f} ms "
          f"(spread {sp:.1%}), x{t0/t1:.2f}")


# The depthwise K x K layers of the ConvMixer models: (name, N, C, H, K).
CONVMIXER_DW_LAYERS = [("256_8", 256, 256, 16, 5), ("256_16", 256, 256, 32, 9),
                       ("768_32", 64, 768, 32, 7)]


def bench_depthwise_large(args, dtype):
    """Native depthwise K x K kernels against MIOpen, per pass, at the
    ConvMixer layer shapes (each at its own batch), alternating window by
    window as `bench_depthwise` does. GF/s is 2 K^2 flops per element and GB/s
    the compulsory traffic (one read and one write of an activation), both
    over the native time. Then the convmixer_256_8 training step at --batch
    with MI355X_NATIVE_DEPTHWISE=1 against =0."""
    from mi355x_ddp import _C
    kw = dict(warmup=args.warmup, iters=args.iters)

    def alternate(fa, fb):
        ta, tb = [], []
        for _ in range(args.windows):
            ta.append(timeit(fa, **kw))
            tb.append(timeit(fb, **kw))
        ta.sort(), tb.sort()
        m = len(ta) // 2
        return ta[m], tb[m], (tb[-1] - tb[0]) / tb[m]

    print(f"{'shape':>22} {'pass':>6} {'MIOpen us':>10} {'native us':>10} "
          f"{'spread':>7} {'cfg':>10} {'x':>6} {'GF/s':>8} {'GB/s':>7}")
    for name, n, c, h, k in CONVMIXER_DW_LAYERS:
        x = torch.randn(n, c, h, h, device="cuda", dtype=dtype) \
            .to(memory_format=torch.channels_last)
        wt = torch.randn(c, 1, k, k, device="cuda", dtype=dtype) / k
        dy = torch.randn_like(x)
        flops, nbytes = 2.0 * k * k * x.numel(), 4.0 * x.numel()

        def miopen_bwd(mask):
            return torch.ops.aten.convolution_backward(
                dy, x, wt, None, [1, 1], [k // 2, k // 2], [1, 1], False,
                [0, 0], c, mask)

        def row(pss, tm, tn, spread, cfg=""):
            print(f"{f'{name} {n}x{c}x{h}x{h} k{k}':>22} {pss:>6} {tm:10.1f} "
                  f"{tn:10.1f} {spread:7.1%} {cfg:>10} {tm/tn:6.2f} "
                  f"{flops/tn/1e3:8.0f} {nbytes/tn/1e3:7.1f}", flush=True)

        row("fwd", *alternate(
            lambda: F.conv2d(x, wt, None, 1, k // 2, 1, c),
            lambda: _C.conv_dwk_fwd(x, wt)))
        row("dgrad", *alternate(lambda: miopen_bwd([True, False, False]),
                                lambda: _C.conv_dwk_dgrad(dy, wt)))
        cells = []   # (native, MIOpen, spread, cfg), the fastest first
        for s in (0, 64, 512):
            tm, tn, sp = alternate(lambda: miopen_bwd([False, True, False]),
                                   lambda: _C.conv_dwk_wgrad(dy, x, k, s))
            cells.append((tn, tm, sp, f"splits {s}"))
        tn, tm, sp, cfg = min(cells)
        row("wgrad", tm, tn, sp, cfg)
        del x, wt, dy

    # the training step, forward + backward + SGD, tuner off on both sides
    from mi355x_ddp.models import build_model
    from mi355x_ddp.ops.conv import MI355Conv2d
    os.environ["MI355X_AUTOTUNE"] = "0"
    N = args.batch
    model = MI355Conv2d.convert(build_model("convmixer_256_8", 100).cuda()) \
        .to(memory_format=torch.channels_last).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    xb = torch.randn(N, 3, 32, 32, device="cuda") \
        .to(memory_format=torch.channels_last)
    lb = torch.randint(0, 100, (N,), device="cuda")

    def step(native):
        os.environ["MI355X_NATIVE_DEPTHWISE"] = native
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype):
            loss = F.cross_entropy(model(xb).float(), lb)
        loss.backward()
        opt.step()

    t0, t1, sp = alternate(lambda: step("0"), lambda: step("1"))
    print(f"# convmixer_256_8 step, batch {N}, 32 px: "
          f"MI355X_NATIVE_DEPTHWISE=0 {t0/1e3:.2f} ms, =1 {t1/1e3:.2f} ms "
          f"(spread {sp:.1%}), x{t0/t1:.2f}")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depthwise-large", action="store_true",
                   help="time the depthwise 5x5 / 7x7 / 9x9 layers of the "
                        "ConvMixer models (native depthwise KxK kernels vs "
                        "MIOpen) and the convmixer_256_8 step with the "
                        "kernels on and off instead")
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--depthwise", action="store_true",
                   help="time the depthwise 3x3 layers of MobileNet-v1 at "
                        "both strides (native depthwise kernels vs MIOpen) "
                        "and the mobilenet_v1 step with the kernels on and "
                        "off instead")
    p.add_argument("--grouped", action="store_true",
                   help="time the grouped 3x3 layers of ResNeXt-50 32x4d "
                        "(native grouped kernels vs MIOpen) instead")
    p.add_argument("--windows", type=int, default=5,
                   help="timing windows per cell of the --grouped table")
    p.add_argument("--arch", type=str, default=None,
                   help="collect shapes from this model instead of the "
                        "static ResNet18 CIFAR table")
    p.add_argument("--image-size", type=int, default=32)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16",
                   help="16-bit format of the operands, for the native "
                        "kernels and the MIOpen column alike")
    args = p.parse_args()
    from mi355x_ddp import _C
    from mi355x_ddp.ops.conv import splitk_candidates
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    print(f"# dtype {args.dtype}, batch {args.batch}")
    if args.grouped:
        return bench_grouped(args, dtype)
    if args.depthwise:
        return bench_depthwise(args, dtype)
    if args.depthwise_large:
        return bench_depthwise_large(args, dtype)
    N = args.batch
    if args.arch:
        rows = collect_model_shapes(args.arch, args.image_size)
    else:
        rows = [(name, c, h, w, k, r, s, p, 1)
                for (name, c, h, w, k, r, s, p) in R18_CIFAR_SHAPES]

    print(f"{'shape':>18} {'pass':>6} {'n':>3} {'MIOpen us':>10} "
          f"{'igemm us':>9} {'best us':>9} {'cfg':>9} {'x':>6} {'TF/s':>7}")
    tot_m = tot_i = tot_b = 0.0  # weighted by multiplicity
    for name, c, h, w, k, r, stride, pad, cnt in rows:
        x = torch.randn(N, c, h, w, device="cuda", dtype=dtype) \
            .to(memory_format=torch.channels_last)
        wt = (torch.randn(k, c, r, r, device="cuda", dtype=dtype)
              / (c * r * r) ** 0.5).to(memory_format=torch.channels_last)
        ph = ((h + 2 * pad - r) // stride + 1)
        pw = ((w + 2 * pad - r) // stride + 1)
        y = F.conv2d(x, wt, None, stride, pad)
        dy = torch.randn_like(y).to(memory_format=torch.channels_last)
        wT = wt.flip(2, 3).permute(1, 2, 3, 0).contiguous()
        flops = 2.0 * N * ph * pw * k * r * r * c

        def row(pss, tm, ti, tb, cfg):
            nonlocal tot_m, tot_i, tot_b
            tot_m += tm * cnt
            tot_i += ti * cnt
            tot_b += tb * cnt
            print(f"{name:>18} {pss:>6} {cnt:>3} {tm:10.1f} {ti:9.1f} "
                  f"{tb:9.1f} {cfg:>9} {tm/tb:6.2f} {flops/tb/1e6:7.1f}",
                  flush=True)

        def sweep(cands, run):
            best, bcfg = float("inf"), None
            for cand in cands:
                t = timeit(lambda: run(cand), warmup=2, iters=args.iters)
                if t < best:
                    best, bcfg = t, cand
            return best, str(bcfg)

        def split_sweep(pss, run):
            """Time the shape's split-K candidates; report each one's error
            against the unsplit 128x128 tile."""
            best, bcfg = float("inf"), None
            base = None
            for cand in splitk_candidates(pss, x.shape, wt.shape, stride, pad,
                                          cus):
                if base is None:
                    base = run(228, 1).float()
                t = timeit(lambda: run(*cand), warmup=2, iters=args.iters)
                err = ((run(*cand).float() - base).norm() / base.norm()).item()
                print(f"# splitk {name:>10} {pss:>6} {str(cand):>9} "
                      f"{t:9.1f} us  rel err vs 228: {err:.3e}", flush=True)
                if t < best:
                    best, bcfg = t, cand
            return best, str(bcfg)

        kw = dict(warmup=args.warmup, iters=args.iters)
        # fwd
        tm = timeit(lambda: F.conv2d(x, wt, None, stride, pad), **kw)
        ti = timeit(lambda: _C.conv_fwd_igemm(x, wt, stride, pad), **kw)
        tb, cfg = sweep((64, 128, 228),
                        lambda t: _C.conv_fwd_igemm(x, wt, stride, pad, t))
        tb, cfg = min((tb, cfg), split_sweep(
            "fwd", lambda t, s: _C.conv_fwd_igemm(x, wt, stride, pad, t, s)))
        row("fwd", tm, ti, tb, cfg)
        # dgrad (skip stem: input grad never needed there)
        if c != 3:
            xg = x.detach().requires_grad_(True)
            tm = timeit(lambda: torch.ops.aten.convolution_backward(
                dy, xg, wt, None, [stride, stride], [pad, pad], [1, 1], False,
                [0, 0], 1, [True, False, False]), **kw)
            ti = timeit(lambda: _C.conv_dgrad_igemm(dy, wT, h, w, stride, pad),
                        **kw)
            tb, cfg = sweep((64, 128, 228), lambda t: _C.conv_dgrad_igemm(
                dy, wT, h, w, stride, pad, t))
            tb, cfg = min((tb, cfg), split_sweep(
                "dgrad", lambda t, s: _C.conv_dgrad_igemm(
                    dy, wT, h, w, stride, pad, t, s)))
            row("dgrad", tm, ti, tb, cfg)
        # wgrad: sweep tile variants x split factors
        tm = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, wt, None, [stride, stride], [pad, pad], [1, 1], False,
            [0, 0], 1, [False, True, False]), **kw)
        ti = timeit(lambda: _C.conv_wgrad_igemm(dy, x, r, r, stride, pad), **kw)
        wcands = [(t, s) for t in (1, 2, 3, 4, 5, 6)
                  for s in (0, 1, 32, 128)] \
            if c != 3 else [(t, s) for t in (1, 4)
                            for s in (0, 32, 128, 512)]
        tb, cfg = sweep(wcands, lambda ts: _C.conv_wgrad_igemm(
            dy, x, r, r, stride, pad, ts[1], ts[0]))
        row("wgrad", tm, ti, tb, cfg)
        del x, wt, y, dy, wT
    print(f"{'TOTAL':>18} {'':>6} {'':>3} {tot_m:10.1f} {tot_i:9.1f} "
          f"{tot_b:9.1f} {'':>9} {tot_m/tot_b:6.2f}")


if __name__ == "__main__":
    main()
