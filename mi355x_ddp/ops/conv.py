"""Native implicit-GEMM convolution (NHWC bf16 or fp16, MFMA) with torch
fallback.

MI355X-native replacement for the reference's cuDNN conv dependency
(every nn.Conv2d in reference utils/model.py — 3x3 s1/s2
and 1x1 convs of the CIFAR ResNet). The HIP kernels (csrc/conv_igemm.hip)
run when input and weight are channels_last CUDA tensors of one 16-bit
dtype, bf16 or fp16 (``--amp bf16`` / ``--amp fp16``: the autocast dtype);
anything else (CPU tests, fp32 mode, exotic shapes) runs torch's conv so the
same module is testable everywhere. ``MI355X_NATIVE_CONV=0`` forces the torch
path for parity A/B; ``MI355X_NATIVE_CONV_FP16=0`` does so for fp16 only
(bf16 keeps the native kernels): the A/B switch for the fp16 kernels.

Autotune (the ``cudnn.benchmark=True`` equivalent the reference relies on,
distributed.py:48): per conv shape, the GEMM-M tile (64 vs 128) for
fwd/dgrad and the split-K factor for wgrad are measured once at first use
with hip events and cached for the rest of the process. ``MI355X_AUTOTUNE=0``
falls back to the static size heuristic inside the kernels. For the late
small-M stages, where 128x128 tiles alone leave most CUs without a block, the
fwd/dgrad candidates include that tile with the reduction split in 2 or 4
slices (``splitk_candidates``); ``MI355X_CONV_SPLITK=0`` removes them (the
A/B switch for the split-K kernels). The heuristic never picks a split.

Weight shadows. Under 16-bit autocast an fp32 conv weight is needed in two
other forms: its copy in the autocast dtype (forward, wgrad) and the
180-degree-rotated transposed filter in that dtype (dgrad). A shadow records
its dtype; a weight used under the other 16-bit dtype gets a new shadow.
Both forms change only when the weight changes,
i.e. once per optimizer step, so ``MI355Conv2d`` keeps them as persistent
tensors (``WeightShadow``: ``w16``, ``wT``) instead of casting per forward
and rotating per backward. ``FusedSGD`` rewrites them in the step that
produces the new weight; any other writer is caught at the next forward by a
``(weight._version, weight.data_ptr())`` stamp and triggers one
``conv_prep_weight`` launch. A writer the version counter cannot see
(``p.data.<op>_()``, raw-pointer kernels) MUST call
``invalidate_weight_shadows``. The weight gradient comes back from the wgrad
epilogue as fp32 (the 16-bit-rounded value, widened), so autograd inserts no
cast node in either direction and results are bit-equal to the cast path.
``MI355X_WEIGHT_SHADOWS=0`` restores the per-call casts (A/B switch);
``MI355X_CHECK_SHADOWS=1`` verifies the shadows against a fresh cast and
rotate at every forward (tests only: it synchronises with the host).
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _backend


def native_conv_wanted() -> bool:
    return os.environ.get("MI355X_NATIVE_CONV", "1") == "1"


def native_conv_fp16_wanted() -> bool:
    return os.environ.get("MI355X_NATIVE_CONV_FP16", "1") == "1"


_NATIVE_DTYPES = (torch.bfloat16, torch.float16)


def autotune_wanted() -> bool:
    return os.environ.get("MI355X_AUTOTUNE", "1") == "1"


def conv_splitk_wanted() -> bool:
    return os.environ.get("MI355X_CONV_SPLITK", "1") == "1"


def weight_shadows_wanted() -> bool:
    return os.environ.get("MI355X_WEIGHT_SHADOWS", "1") == "1"


def check_shadows_wanted() -> bool:
    return os.environ.get("MI355X_CHECK_SHADOWS", "0") == "1"


def _native_ok(x: torch.Tensor, weight: torch.Tensor, stride, padding,
               dilation, groups, weight_dtype=None) -> bool:
    """`weight_dtype` overrides weight.dtype: the dtype the kernels will see
    when a 16-bit shadow stands in for an fp32 weight. x and weight must
    share one 16-bit dtype, bf16 or fp16."""
    if not native_conv_wanted() or not _backend.native_enabled(x):
        return False
    if weight_dtype is None:
        weight_dtype = weight.dtype
    if x.dtype not in _NATIVE_DTYPES or weight_dtype != x.dtype:
        return False
    if x.dtype == torch.float16 and not native_conv_fp16_wanted():
        return False
    if groups != 1 or dilation[0] != 1 or dilation[1] != 1:
        return False
    if stride[0] != stride[1] or padding[0] != padding[1]:
        return False
    # only take over when the tensors are already NHWC — in NCHW mode the
    # MIOpen path stays (no per-call layout conversions)
    if not x.is_contiguous(memory_format=torch.channels_last):
        return False
    # square filters only (the ResNet zoo is 3x3 / 1x1)
    return weight.shape[2] == weight.shape[3]


# --------------------------------------------------------------------------
# Per-shape launch-config cache (kernel-selection cache a la cudnn.benchmark)
# --------------------------------------------------------------------------

_TUNE_CACHE: Dict[Tuple, int] = {}


def _measure_ms(fn: Callable[[], None], iters: int = 4,
                abort_above_ms: Optional[float] = None) -> float:
    """Event-timed mean; one probe run first, and if that alone exceeds
    `abort_above_ms` the candidate is hopeless (e.g. MIOpen immediate mode
    falling back to a naive kernel at 50+ ms) — skip the refinement runs
    instead of paying 5x a pathological time."""
    fn()  # allocator warm-up
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    probe = start.elapsed_time(stop)
    if abort_above_ms is not None and probe > abort_above_ms:
        return probe
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def _tuned_choice(key: Tuple,
                  candidates: Union[Sequence, Callable[[], Sequence]],
                  run: Callable, default=None):
    """Cached fastest candidate for this shape key.

    `default` (first candidate unless given) is returned without measuring
    when autotune is off or a hipGraph capture is in flight — for the native
    kernels that is the launch-config heuristic, never MIOpen. `candidates`
    may be a callable that returns them: it runs on a cache miss only.
    """
    if key in _TUNE_CACHE:
        return _TUNE_CACHE[key]
    # NB: is_current_stream_capturing() raises on CPU-only machines — check
    # the cheap conditions first (the tuner is only reached from GPU paths,
    # but keep it robust for direct callers/tests)
    off = (not autotune_wanted() or not torch.cuda.is_available() or
           torch.cuda.is_current_stream_capturing())
    if off and default is not None:
        return default
    if callable(candidates):
        candidates = candidates()
    if off:
        return candidates[0]
    best, best_ms = candidates[0], float("inf")
    for c in candidates:
        # a candidate already 2x slower than the best can't win — one
        # probe run suffices (bounds the cost of pathological candidates)
        cutoff = 2.0 * best_ms if best_ms < float("inf") else None
        ms = _measure_ms(lambda: run(c), abort_above_ms=cutoff)
        if ms < best_ms:
            best, best_ms = c, ms
    _TUNE_CACHE[key] = best
    return best


TILE_128X128 = 228   # the kernels' name for the 128x128 fwd/dgrad tile
_SPLITK_COUNTS = (2, 4)
_SPLITK_MIN_KTILES = 4    # reduction tiles (of 64) a slice must keep


def splitk_candidates(kind: str, x_shape, w_shape, stride: int, padding: int,
                      cus: int) -> Tuple[Tuple[int, int], ...]:
    """The (tile, splits) candidates the tuner adds for one fwd or dgrad pass:
    a plain function of the shapes, so it can be tested without a GPU.

    `x_shape` is the conv input (N, C, H, W) and `w_shape` the filter
    (K, C, R, S), for both kinds. Split-K is offered only where it can pay:
    - the pass takes the pipelined 128x128 kernel: gathered channels a
      multiple of 64 and at least 96 GEMM columns; a stride-2 input-grad
      with even H, W runs the parity kernels, which have no split form;
    - the 128x128 tiles alone do not fill the chip: their count is at most
      `cus`, the device's CU count;
    - every slice keeps at least 4 reduction tiles of 64.
    """
    if not conv_splitk_wanted() or kind not in ("fwd", "dgrad"):
        return ()
    n, c, h, w = (int(v) for v in x_shape)
    k, r, s = int(w_shape[0]), int(w_shape[2]), int(w_shape[3])
    if kind == "fwd":
        p = (h + 2 * padding - r) // stride + 1
        q = (w + 2 * padding - s) // stride + 1
        gm, gn, gathered = n * p * q, k, c
    else:
        if stride == 2 and h % 2 == 0 and w % 2 == 0:
            return ()
        gm, gn, gathered = n * h * w, c, k
    if gathered % 64 != 0 or gn < 96:
        return ()
    tiles = -(-gm // 128) * -(-gn // 128)
    if tiles > cus:
        return ()
    ktiles = r * s * gathered // 64
    return tuple((TILE_128X128, z) for z in _SPLITK_COUNTS
                 if ktiles // z >= _SPLITK_MIN_KTILES)


def _cu_count(t: torch.Tensor) -> int:
    return torch.cuda.get_device_properties(t.device).multi_processor_count


def _choice_label(choice) -> str:
    if choice == MIOPEN:
        return "MIOpen"
    if isinstance(choice, tuple) and len(choice) == 2 and \
            choice[0] == TILE_128X128:
        return f"128x128 tile, split-K x{choice[1]}"
    return str(choice)


def _tune_key(kind: str, dtype: torch.dtype, *shape) -> Tuple:
    """Cache key of one pass: the operands' dtype comes right after the pass
    name, so bf16 and fp16 runs of one shape are tuned separately."""
    return (kind, dtype) + tuple(shape)


def clear_autotune_cache() -> None:
    _TUNE_CACHE.clear()


def tune_report() -> str:
    """Human-readable dump of the per-shape choices the tuner made
    (``MI355X_TUNE_REPORT=1`` makes bench.py print it to stderr at exit)."""
    lines = []
    for key in sorted(_TUNE_CACHE, key=str):
        choice = _TUNE_CACHE[key]
        # wgrad choices are (wtile, splits) pairs too, printed as they are
        if key[0] == "fwd_bn":   # ops/fused_eval.py: conv + eval BN
            if choice == UNFUSED:
                label = "unfused: conv2d, then bn_fwd_apply"
            elif choice == TILE_128X128:
                label = "fused BN epilogue, 128x128 tile"
            elif isinstance(choice, tuple):
                label = f"fused BN epilogue, {_choice_label(choice)}"
            else:
                label = f"fused BN epilogue, tile {choice}"
        else:
            label = _choice_label(choice) if key[0] in ("fwd", "dgrad") \
                else ("MIOpen" if choice == MIOPEN else str(choice))
        # _ConvIGEMM's keys carry the dtype of the pass's operands at [1]
        if len(key) > 1 and isinstance(key[1], torch.dtype):
            dt, rest = str(key[1]).replace("torch.", ""), key[2:]
        else:
            dt, rest = "", key[1:]
        lines.append(f"{key[0]:>12} {dt:>8} {str(rest):<70} -> {label}")
    return "\n".join(lines) if lines else "(autotune cache empty)"


MIOPEN = -1  # tuner sentinel: this pass is fastest on the MIOpen kernel
UNFUSED = -2  # "fwd_bn" sentinel: the plain conv2d, then bn_fwd_apply


# --------------------------------------------------------------------------
# Persistent bf16 / rotated copies of an fp32 conv weight
# --------------------------------------------------------------------------

def rotate_wT(w16: torch.Tensor) -> torch.Tensor:
    """Torch form of conv_build_wT: wT[c][i][j][k] = w[k][c][R-1-i][S-1-j],
    (C, R, S, K) contiguous."""
    return w16.flip(2, 3).permute(1, 2, 3, 0).contiguous()


class WeightShadow:
    """`w16` (the weight's shape and strides) and `wT` ((C,R,S,K) contiguous)
    of one fp32 (K,C,R,S) weight, both in `dtype` (bf16 or fp16: the autocast
    dtype the weight is used under). Both are allocated once and only ever
    rewritten in place, so a hipGraph-captured step that reads or writes them
    stays replayable. `stamp` is (weight._version, weight.data_ptr()) at the
    time they were last written, None when known stale."""

    __slots__ = ("w16", "wT", "dtype", "stamp", "refreshes")

    def __init__(self, weight: torch.Tensor,
                 dtype: torch.dtype = torch.bfloat16):
        if dtype not in _NATIVE_DTYPES:
            raise ValueError(f"a weight shadow is bf16 or fp16, not {dtype}")
        K, C, R, S = weight.shape
        self.dtype = dtype
        # empty_like keeps the strides of a dense tensor
        self.w16 = torch.empty_like(weight.detach(), dtype=dtype)
        self.wT = torch.empty((C, R, S, K), dtype=dtype,
                              device=weight.device)
        self.stamp = None
        self.refreshes = 0

    def matches(self, weight: torch.Tensor) -> bool:
        """These buffers can shadow `weight` (same shape, layout, device)."""
        return (weight.dtype == torch.float32 and
                weight.device == self.w16.device and
                weight.shape == self.w16.shape and
                weight.stride() == self.w16.stride())

    def fresh(self, weight: torch.Tensor) -> bool:
        return self.stamp == (weight._version, weight.data_ptr())

    def mark_fresh(self, weight: torch.Tensor) -> None:
        self.stamp = (weight._version, weight.data_ptr())

    def invalidate(self) -> None:
        self.stamp = None

    def refresh(self, weight: torch.Tensor) -> None:
        """Cast + rotate into the existing buffers (one launch natively)."""
        w = weight.detach()
        if _backend.native_enabled(w):
            _backend.C().conv_prep_weight(w, self.w16, self.wT)
        else:
            with torch.no_grad():
                self.w16.copy_(w)
                self.wT.copy_(rotate_wT(self.w16))
        self.refreshes += 1
        self.mark_fresh(weight)

    def ensure(self, weight: torch.Tensor) -> None:
        if not self.fresh(weight):
            self.refresh(weight)

    def check(self, weight: torch.Tensor) -> None:
        """Raise if the shadows differ from a fresh cast + rotate."""
        w16 = weight.detach().to(self.dtype)
        if not torch.equal(self.w16, w16):
            raise RuntimeError(f"stale {self.dtype} weight shadow (w16) for a "
                               f"weight of shape {tuple(weight.shape)}")
        if not torch.equal(self.wT, rotate_wT(w16)):
            raise RuntimeError("stale rotated weight shadow (wT) for a weight "
                               f"of shape {tuple(weight.shape)}")


def shadow_of(weight: torch.Tensor) -> Optional[WeightShadow]:
    """The shadow attached to this parameter, if any (fresh or not)."""
    return getattr(weight, "_mi355x_shadow", None)


def _shadow_for(weight: torch.Tensor,
                dtype: torch.dtype = torch.bfloat16) -> WeightShadow:
    """Fresh shadow of `weight` in `dtype`, created at first use; a shadow of
    the other 16-bit dtype (the model ran under the other autocast mode
    before) is replaced."""
    sh = shadow_of(weight)
    if sh is None or sh.dtype != dtype or not sh.matches(weight):
        sh = WeightShadow(weight, dtype)
        weight._mi355x_shadow = sh
    sh.ensure(weight)
    if check_shadows_wanted():
        sh.check(weight)
    return sh


def invalidate_weight_shadows(
        target: Union[nn.Module, torch.Tensor, Iterable[torch.Tensor]]) -> None:
    """Mark the weight shadows of a module's (or the given) parameters stale;
    the next forward rebuilds them. Needed after any parameter write that does
    not bump the tensor's version counter: `p.data.<op>_()`, a collective on
    `p.data`, a kernel writing through the raw pointer."""
    if isinstance(target, nn.Module):
        params = target.parameters()
    elif isinstance(target, torch.Tensor):
        params = (target,)
    else:
        params = target
    for p in params:
        sh = shadow_of(p)
        if sh is not None:
            sh.invalidate()


class _ConvIGEMM(torch.autograd.Function):
    """Per-pass dispatch between the native igemm kernels (with their tile /
    split-K launch knobs) and MIOpen, chosen by the per-shape autotune cache.
    The heuristic default (autotune off) is always the native kernel.

    `weight` is the differentiable input. With `w16`/`wT` given (a
    WeightShadow's tensors) it is an fp32 parameter: the passes run on the
    shadows and backward returns an fp32 gradient. The shadows are kept on
    ctx, not in save_for_backward: they are rewritten in place by design, and
    backward reads whatever they hold then (the weight must not change
    between a forward and its backward)."""

    @staticmethod
    def forward(ctx, x, weight, stride: int, padding: int, w16=None, wT=None):
        x = x.contiguous(memory_format=torch.channels_last)
        ctx.shadowed = w16 is not None
        if ctx.shadowed:
            weight = w16
            ctx.save_for_backward(x)
            ctx.w16, ctx.wT = w16, wT
        else:
            weight = weight.contiguous(memory_format=torch.channels_last)
            ctx.save_for_backward(x, weight)
        ctx.stride, ctx.padding = stride, padding
        C = _backend.C()

        def run(t):
            if t == MIOPEN:
                return F.conv2d(x, weight, None, stride, padding)
            if isinstance(t, tuple):     # (tile, split-K slices)
                return C.conv_fwd_igemm(x, weight, stride, padding, *t)
            return C.conv_fwd_igemm(x, weight, stride, padding, t)

        # the dtype is part of every key: a choice measured for bf16 is never
        # replayed for fp16 in the same process
        key = _tune_key("fwd", x.dtype, x.shape, weight.shape, stride,
                        padding)
        def cands():
            return (64, 128, TILE_128X128) + splitk_candidates(
                "fwd", x.shape, weight.shape, stride, padding,
                _cu_count(x)) + (MIOPEN,)

        return run(_tuned_choice(key, cands, run, default=0))

    @staticmethod
    def backward(ctx, dy):
        if ctx.shadowed:
            (x,), weight = ctx.saved_tensors, ctx.w16
        else:
            x, weight = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        C = _backend.C()
        if ctx.needs_input_grad[0]:
            # 180°-rotated, (C,R,S,K)-transposed filter for the dgrad GEMM
            wT = ctx.wT if ctx.shadowed else C.conv_build_wT(weight)

            def run_dx(t):
                if t == MIOPEN:
                    return torch.ops.aten.convolution_backward(
                        dy, x, weight, None,
                        [ctx.stride, ctx.stride], [ctx.padding, ctx.padding],
                        [1, 1], False, [0, 0], 1, [True, False, False])[0]
                tile, nz = t if isinstance(t, tuple) else (t, 1)
                return C.conv_dgrad_igemm(dy, wT, x.shape[2], x.shape[3],
                                          ctx.stride, ctx.padding, tile, nz)

            key = _tune_key("dgrad", x.dtype, dy.shape, wT.shape,
                            ctx.stride, ctx.padding)
            def cands_dx():
                return (64, 128, TILE_128X128) + splitk_candidates(
                    "dgrad", x.shape, weight.shape, ctx.stride, ctx.padding,
                    _cu_count(x)) + (MIOPEN,)

            dx = run_dx(_tuned_choice(key, cands_dx, run_dx, default=0))
        if ctx.needs_input_grad[1]:
            R = weight.shape[2]

            def run_dw(c):
                if c == MIOPEN:
                    g = torch.ops.aten.convolution_backward(
                        dy, x, weight, None,
                        [ctx.stride, ctx.stride], [ctx.padding, ctx.padding],
                        [1, 1], False, [0, 0], 1, [False, True, False])[1]
                    g = g.contiguous(memory_format=torch.channels_last)
                    return g.float() if ctx.shadowed else g
                wtile, splits = c
                # kernel emits (K,C,R,S) channels_last directly — no
                # fp32->bf16 permute/copy pass; for an fp32 weight the
                # bf16-rounded values come out as fp32, no widening pass
                return C.conv_wgrad_igemm(dy, x, R, R, ctx.stride,
                                          ctx.padding, splits, wtile,
                                          ctx.shadowed)

            # two-phase: pick the tile (v1/v2 variants vs MIOpen), then the
            # split-K factor for the winning native tile
            kt = _tune_key("wgrad_tile", x.dtype, dy.shape, x.shape, R,
                           ctx.stride, ctx.padding)
            tile = _tuned_choice(
                kt, ((0, 0), (1, -1), (2, -1), (3, -1), (4, 0), (5, -1),
                     (6, -1), MIOPEN),
                run_dw, default=(0, 0))
            if tile == MIOPEN:
                choice = MIOPEN
            else:
                ks = _tune_key("wgrad_splits", x.dtype, dy.shape, x.shape,
                               R, ctx.stride, ctx.padding, tile[0])
                # 0 = the kernel's default (~1024 blocks, the bit-stable
                # count), -1 = one resident set of blocks (3..200 slices on
                # the ResNet shapes); the explicit counts bracket both
                choice = _tuned_choice(
                    ks, tuple((tile[0], s) for s in (0, -1, 1, 32, 128)),
                    run_dw, default=tile)
            dw = run_dw(choice)
        return dx, dw, None, None, None, None


def conv2d(x: torch.Tensor, weight: torch.Tensor, stride=(1, 1),
           padding=(0, 0), dilation=(1, 1), groups: int = 1) -> torch.Tensor:
    if _native_ok(x, weight, stride, padding, dilation, groups):
        return _ConvIGEMM.apply(x, weight, stride[0], padding[0])
    return F.conv2d(x, weight, None, stride, padding, dilation, groups)


class MI355Conv2d(nn.Conv2d):
    """nn.Conv2d whose hot path is the implicit-GEMM HIP kernel.

    Under bf16 or fp16 autocast the input is cast explicitly to the autocast
    dtype (custom autograd Functions are invisible to autocast's casting). An
    fp32 channels_last weight headed for the native kernels is not cast per
    call: its WeightShadow (see the module docstring) supplies the 16-bit and
    rotated forms in that dtype. Every other fp32 weight is cast per call as
    before, and a weight that already is bf16 (`bf16_o2`) needs neither.
    Outside autocast the native path runs only when the tensors already share
    one 16-bit dtype.
    """

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        weight = self.weight
        dt = torch.get_autocast_dtype("cuda") \
            if torch.is_autocast_enabled() and x.is_cuda else None
        # MI355X_NATIVE_CONV_FP16=0: fp16 autocast is left to torch's conv,
        # casts included, as before the fp16 kernels existed
        if dt == torch.float16 and not native_conv_fp16_wanted():
            dt = None
        if dt in _NATIVE_DTYPES:
            x = x.to(dt)
            if self._shadow_ok(x, weight):
                sh = _shadow_for(weight, dt)
                return _ConvIGEMM.apply(x, weight, self.stride[0],
                                        self.padding[0], sh.w16, sh.wT)
            weight = weight.to(dt)
        return conv2d(x, weight, self.stride, self.padding, self.dilation,
                      self.groups)

    def native_operands(self, x: torch.Tensor
                        ) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(input, filter) as `forward` would hand them to the forward igemm
        kernel, or None where `forward` would not run that kernel for `x`
        (torch's conv instead). The filter is the WeightShadow's `w16` where
        `forward` would use the shadow, so a changed weight is picked up by
        the same stamp. For callers that replace the forward kernel by a
        sibling of it (ops/fused_eval.py)."""
        weight = self.weight
        dt = torch.get_autocast_dtype("cuda") \
            if torch.is_autocast_enabled() and x.is_cuda else None
        if dt == torch.float16 and not native_conv_fp16_wanted():
            dt = None
        if dt in _NATIVE_DTYPES:
            x = x.to(dt)
            if self._shadow_ok(x, weight):
                return x, _shadow_for(weight, dt).w16
            weight = weight.to(dt)
        if not _native_ok(x, weight, self.stride, self.padding, self.dilation,
                          self.groups):
            return None
        return (x.contiguous(memory_format=torch.channels_last),
                weight.detach().contiguous(memory_format=torch.channels_last))

    def _shadow_ok(self, x: torch.Tensor, weight: torch.Tensor) -> bool:
        return (weight_shadows_wanted() and
                weight.dtype == torch.float32 and weight.is_cuda and
                weight.dim() == 4 and
                weight.is_contiguous(memory_format=torch.channels_last) and
                _native_ok(x, weight, self.stride, self.padding,
                           self.dilation, self.groups,
                           weight_dtype=x.dtype))

    @classmethod
    def convert(cls, module: nn.Module) -> nn.Module:
        """Swap every plain nn.Conv2d (bias-free, as the ResNet zoo builds
        them) for MI355Conv2d, preserving parameters."""
        if type(module) is nn.Conv2d and module.bias is None:
            new = cls(module.in_channels, module.out_channels,
                      module.kernel_size, module.stride, module.padding,
                      module.dilation, module.groups, bias=False)
            new.weight = module.weight
            return new
        for name, child in module.named_children():
            setattr(module, name, cls.convert(child))
        return module
