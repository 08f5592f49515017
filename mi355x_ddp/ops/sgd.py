"""Fused multi-tensor SGD with momentum + weight decay.

MI355X-native replacement for the per-parameter ATen SGD step the reference
runs (optimizer at distributed.py:63; SURVEY.md §2.2 N9 calls this the
BASELINE north-star): ONE HIP kernel launch updates every parameter of the
model — ResNet18 has ~62 tensors, so the eager step's ~180 kernel launches
collapse to 1. Math matches torch.optim.SGD exactly:

    m <- mu*m + g + wd*p      (momentum buffer, damping 0)
    p <- p - lr*m

bf16 parameters (the apex-O2-equivalent ``amp="bf16_o2"`` mode, where the
MODEL lives in bf16 and no per-step autocast weight casts exist) get an
fp32 MASTER copy in the optimizer state: the update runs in fp32 against
the master and the bf16 parameter is its rounded copy —

    m <- mu*m + g + wd*master ; master <- master - lr*m ; p <- bf16(master)

Mixed models (some fp32, some bf16 tensors) split into the two paths.

Conv weight shadows (ops/conv.py): an fp32 conv weight used under 16-bit
autocast carries persistent copies in the autocast dtype, bf16 or fp16:
`w16` and the rotated `wT`. The native kernels here write parameters through
raw pointers, which the tensor's version counter does not see, so for every
parameter it updates that carries a shadow the step either rewrites the
shadow itself — the SGD kernel stores p_new rounded to the shadow's dtype
into `w16` next to `p` (per tensor: one step may carry bf16 and fp16
shadows), and one batched `multi_tensor_build_wT` launch rotates every `w16`
into its `wT` — or marks it stale. Never neither.

LARS and clipping by the global gradient norm (``lars=True``,
``clip_grad_norm=x``; both off by default, and then the step is exactly the
one above). With w the fp32 weight (the parameter, or the O2 master), over the
T tensors that are stepped:

    norm    = sqrt(sum_t |g_t|^2)                       the pre-clip global norm
    c       = min(1, x / (norm + 1e-6))                 1 when clipping is off
    ratio_t = eta*|w_t| / (c*|g_t| + wd*|w_t| + 1e-8)   1 when LARS is off
    d       = ratio_t * (c*g + wd*w) ; m <- mu*m + d ; w <- w - lr*m

c is ``torch.nn.utils.clip_grad_norm_``'s coefficient, but the gradient
tensors are NOT modified: clipping happens inside the update. ratio_t is 1 for
tensors with ``ndim <= 1`` (BatchNorm affine, biases; their weight decay stays
as the group says) and when |w_t| or |g_t| is 0. Parameters without a gradient
are skipped and do not enter the norm. On the native path the norms, c and the
ratios are computed on the device (`multi_tensor_sqnorm`, `sgd_coeffs`: fixed
summation order, no atomics) into buffers that the optimizer keeps, and the
update kernels read them there: after the first step a step does no host
sync, no host-to-device copy and no allocation, so it captures into a
hipGraph. The norm is global over all param groups; max_norm, eta and wd are
each group's own. The effect of either feature on accuracy has not been
measured in this project.

Weight EMA (``ema_decay=d``, 0 < d < 1; 0, the default, is off, and then the
step is exactly the one above, same code path and same launches). Every
stepped tensor keeps an fp32 average ``state[p]["ema"]`` of its fp32 weight w
(the parameter, or the O2 master), created at the first step as a copy of w
before that step's update (timm's ``ModelEmaV2`` initialisation) and then, in
the same kernel that produces the new weight,

    e <- d*e + (1 - d)*w_new          fmaf(d, e, omd*w_new), omd = 1.f - d

with d and omd rounded to fp32 once on the host. Tensors the optimizer does
not step (the BatchNorm running statistics) are averaged by the same formula
when handed over with `track_buffers`: one `multi_tensor_ema` launch per 32
tensors at the end of `step()`, so a skipped fp16 step skips the averages too
and a captured step holds them. core/ema.py (`WeightEMA`) swaps the averages
in for evaluation. Out of scope: decay warm-up or schedules, updating every N
steps, evaluating both weight sets per epoch. The effect on accuracy has not
been measured in this project.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

from . import _backend
from .conv import WeightShadow, shadow_of, weight_shadows_wanted

# The extension exports its values under the same names (_C.MT_CHUNK for the
# last); these serve the CPU fallback, which runs with no extension built.
LARS_EPS = 1e-8   # in the trust ratio's denominator
CLIP_EPS = 1e-6   # torch.nn.utils.clip_grad_norm_'s
_MT_CHUNK = 1 << 13   # elements per block


class _NormBuffers:
    """Device buffers of the scaled step, kept while the list of stepped
    tensors is unchanged."""

    def __init__(self, key, ws: List[torch.Tensor], excluded: List[bool],
                 ngroups: int):
        dev = ws[0].device
        chunks = sum((w.numel() + _MT_CHUNK - 1) // _MT_CHUNK for w in ws)
        n = len(ws)
        self.key = key
        self.partials = torch.empty(2, max(chunks, 1), device=dev)
        self.sq = torch.zeros(2, n, device=dev)
        self.gscale = torch.ones(ngroups, device=dev)
        self.ratio = torch.ones(n, device=dev)
        self.gnorm = torch.zeros((), device=dev)
        self.excluded = torch.tensor(excluded, dtype=torch.uint8).to(dev)


def ema_coeffs(decay: float):
    """(d, omd) as the kernels take them: d rounded to fp32, omd = 1 - d formed
    in fp32, both returned as Python floats that fp32 holds exactly."""
    d = torch.tensor(float(decay), dtype=torch.float32)
    return float(d), float(torch.ones((), dtype=torch.float32) - d)


def ema_update_torch(emas, ws, decay: float) -> None:
    """e <- d*e + (1 - d)*w in torch for every pair, fp32; a None average is
    skipped. The kernels' formula (they fuse the multiply-add)."""
    d, omd = ema_coeffs(decay)
    for e, w in zip(emas, ws):
        if e is not None:
            e.mul_(d).add_(w, alpha=omd)


def multi_tensor_ema(srcs: List[torch.Tensor], emas: List[torch.Tensor],
                     decay: float) -> None:
    """emas[i] <- decay*emas[i] + (1 - decay)*srcs[i], fp32: one native launch
    per 32 tensors on the GPU, torch on the CPU."""
    if not srcs:
        return
    if _backend.native_enabled(srcs[0]):
        _backend.C().multi_tensor_ema(srcs, emas, decay)
    else:
        ema_update_torch(emas, srcs, decay)


def _group_scaled(group) -> bool:
    return bool(group.get("lars", False)) or \
        group.get("clip_grad_norm", 0.0) > 0


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, lars: bool = False,
                 lars_eta: float = 1e-3, clip_grad_norm: float = 0.0,
                 ema_decay: float = 0.0):
        if not 0 <= ema_decay < 1:
            raise ValueError("ema_decay must be in [0, 1) (0 turns the weight "
                             f"average off), got {ema_decay}")
        if lars_eta <= 0:
            raise ValueError(f"lars_eta must be > 0, got {lars_eta}")
        if clip_grad_norm < 0:
            raise ValueError("clip_grad_norm must be >= 0 (0 turns clipping "
                             f"off), got {clip_grad_norm}")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                        lars=bool(lars), lars_eta=lars_eta,
                        clip_grad_norm=clip_grad_norm,
                        ema_decay=float(ema_decay))
        super().__init__(params, defaults)
        self._norm: Optional[_NormBuffers] = None
        self._grad_norm: Optional[torch.Tensor] = None
        self._ema_buffers = ([], [])

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_ema_buffers", ([], []))
        # a state dict saved before ema_decay existed has no such key in its
        # groups: the run's own setting holds, so its averages start from the
        # loaded weights
        for group in self.param_groups:
            group.setdefault("ema_decay", self.defaults.get("ema_decay", 0.0))

    def load_state_dict(self, state_dict) -> None:
        """torch's, with two differences.

        `ema_decay` stays this run's own in every group, whatever the saved
        groups hold (0, another value, or no such key): whether a run averages
        is its `--ema_decay`, and a `WeightEMA` built for the run relies on it.
        The saved averages are restored either way; a run with averages that
        loads a state without them starts them, at its next step, from the
        loaded weights.

        The fp32 state of a bf16 (O2) parameter stays fp32: torch casts every
        floating-point state tensor to the parameter's dtype, which would
        round `master`, `momentum_buffer` and `ema` to bf16."""
        own = [g.get("ema_decay", 0.0) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, decay in zip(self.param_groups, own):
            group["ema_decay"] = decay
        saved = state_dict["state"]
        for group, sgroup in zip(self.param_groups,
                                 state_dict["param_groups"]):
            for p, pid in zip(group["params"], sgroup["params"]):
                if p.dtype != torch.bfloat16 or pid not in saved:
                    continue
                for key in ("master", "momentum_buffer", "ema"):
                    if key in saved[pid]:
                        self.state[p][key] = saved[pid][key].detach().to(
                            device=p.device, dtype=torch.float32, copy=True)

    def _buffer_decay(self) -> float:
        """The decay of the tracked buffers: the one every group has."""
        decays = {g.get("ema_decay", 0.0) for g in self.param_groups}
        if len(decays) != 1 or min(decays) <= 0:
            raise RuntimeError(
                "track_buffers needs one ema_decay > 0 shared by every param "
                f"group, got {sorted(decays)}")
        return decays.pop()

    def track_buffers(self, pairs) -> None:
        """`pairs`: (buffer, ema_buffer) fp32 tensors that no group steps (the
        BatchNorm running statistics). Every `step()` that runs averages them
        after the parameter update, with the groups' `ema_decay`, which has to
        be one positive value for all groups (checked here and at every step
        that has buffers to average); replaces any earlier list."""
        srcs, emas = [], []
        for src, ema in pairs:
            if src.dtype != torch.float32 or ema.dtype != torch.float32 or \
                    src.shape != ema.shape or src.device != ema.device:
                raise ValueError("track_buffers takes (buffer, ema_buffer) "
                                 "pairs of fp32 tensors of one shape")
            srcs.append(src)
            emas.append(ema)
        if srcs:
            self._buffer_decay()
        self._ema_buffers = (srcs, emas)

    def grad_norm(self) -> Optional[torch.Tensor]:
        """0-dim tensor on the parameters' device: the global gradient norm of
        the last step, before clipping. None when LARS and clipping are both
        off (and before the first step). Reading it is a host sync."""
        if not any(_group_scaled(g) for g in self.param_groups):
            return None
        return getattr(self, "_grad_norm", None)

    def _gather(self, group) -> "_Gathered":
        """The group's tensors that have a gradient, split into the fp32 and
        the bf16 (O2) path; creates masters and momentum buffers."""
        # plain local lists: this loop is host time of every step
        p32, g32, m32, s32 = [], [], [], []
        p16, g16, w16, m16 = [], [], [], []
        has_momentum = group["momentum"] != 0
        for p in group["params"]:
            if p.grad is None:
                continue
            state = self.state[p]
            if p.dtype == torch.bfloat16:
                if "master" not in state:
                    state["master"] = p.detach().float()
                w, ms = state["master"], m16
                p16.append(p)
                g16.append(p.grad)
                w16.append(w)
            else:
                w, ms = p, m32
                p32.append(p)
                g32.append(p.grad)
                s32.append(shadow_of(p))
            if has_momentum:
                if "momentum_buffer" not in state:
                    state["momentum_buffer"] = torch.zeros_like(w)
                ms.append(state["momentum_buffer"])
        if not has_momentum:
            m32 = m16 = None
        # a pass of its own, so that the loop above costs a step without
        # averages nothing
        e32 = e16 = None
        if group.get("ema_decay", 0.0) > 0:
            e32 = [self._ema_of(p, p) for p in p32]
            e16 = [self._ema_of(p, w) for p, w in zip(p16, w16)]
        return _Gathered(p32, g32, m32, s32, p16, g16, w16, m16, e32, e16)

    def _ema_of(self, p, w) -> torch.Tensor:
        """The average of parameter p's fp32 weight w; at first use a copy of
        w, which `_gather` sees before the step's update."""
        state = self.state[p]
        if "ema" not in state:
            state["ema"] = w.detach().clone()
        return state["ema"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if any(_group_scaled(g) for g in self.param_groups):
            self._step_scaled()
        else:
            for group in self.param_groups:
                _step_group(group, self._gather(group))
        srcs, emas = self._ema_buffers
        if srcs:
            multi_tensor_ema(srcs, emas, self._buffer_decay())
        return loss

    def _step_scaled(self) -> None:
        """The step with LARS and/or clipping on in at least one group."""
        gathered = [self._gather(g) for g in self.param_groups]
        # the order of the norm's tensor list: group by group, a group's fp32
        # tensors before its bf16 ones, so each path's ratios are one slice
        ws, gs, excluded, ranges = [], [], [], []
        for got in gathered:
            lo = len(ws)
            ws += got.p32 + got.w16
            gs += got.g32 + got.g16
            excluded += [p.ndim <= 1 for p in got.p32 + got.p16]
            ranges.append((lo, lo + len(got.p32), len(ws)))
        if not ws:
            return
        native = _backend.native_enabled(ws[0])
        if native:
            # all that the buffers' sizes and contents depend on
            key = (tuple(w.numel() for w in ws), tuple(excluded),
                   len(self.param_groups), ws[0].device)
            nb = getattr(self, "_norm", None)
            if nb is None or nb.key != key:
                nb = self._norm = _NormBuffers(key, ws, excluded,
                                               len(self.param_groups))
            _backend.C().multi_tensor_sqnorm(ws, gs, nb.partials, nb.sq)
            self._grad_norm = nb.gnorm
        else:
            sq_w = torch.stack([w.float().pow(2).sum() for w in ws])
            sq_g = torch.stack([g.float().pow(2).sum() for g in gs])
        for gi, (group, got, (lo, mid, hi)) in enumerate(
                zip(self.param_groups, gathered, ranges)):
            if lo == hi:
                continue
            wd = group["weight_decay"]
            max_norm = group.get("clip_grad_norm", 0.0)
            lars = bool(group.get("lars", False))
            eta = group.get("lars_eta", 1e-3)
            if native:
                gscale = nb.gscale[gi:gi + 1]
                ratio = nb.ratio
                _backend.C().sgd_coeffs(nb.sq, nb.excluded, gscale, ratio,
                                        nb.gnorm, max_norm, lars, eta, wd,
                                        lo, hi)
            else:
                gscale, ratio, self._grad_norm = sgd_coeffs_torch(
                    sq_w, sq_g, excluded, max_norm, lars, eta, wd)
            _step_group(group, got, gscale, ratio[lo:mid], ratio[mid:hi])


class _Gathered(NamedTuple):
    """One group's tensors that have a gradient, by path. The momentum lists
    are None when the group has no momentum."""
    # fp32 path: params, grads, momentum buffers, weight shadows (None where
    # a param has none)
    p32: list
    g32: list
    m32: Optional[list]
    s32: list
    # O2 path: bf16 params, bf16 grads, fp32 masters, fp32 momentum buffers
    p16: list
    g16: list
    w16: list
    m16: Optional[list]
    # fp32 averages of p32 and of the masters w16; None when the group's
    # ema_decay is 0
    e32: Optional[list] = None
    e16: Optional[list] = None


def _step_group(group, got: _Gathered, gscale=None, ratio32=None,
                ratio16=None) -> None:
    """Steps one group; without `gscale` and the ratios, the plain step."""
    lr, momentum = group["lr"], group["momentum"]
    wd = group["weight_decay"]
    decay = group.get("ema_decay", 0.0)
    if got.p32:
        fused_sgd_step(got.p32, got.g32, got.m32, lr, momentum, wd, got.s32,
                       gscale, ratio32, got.e32, decay)
    if got.p16:
        fused_sgd_o2_step(got.p16, got.g16, got.w16, got.m16, lr, momentum,
                          wd, gscale, ratio16, got.e16, decay)


def sgd_coeffs_torch(sq_w: torch.Tensor, sq_g: torch.Tensor,
                     excluded: List[bool], max_norm: float, lars: bool,
                     eta: float, weight_decay: float):
    """The `sgd_coeffs` kernel's math in torch, in its order: per-tensor sums
    of squares (fp32 [n] each) -> (gscale [1], ratio [n], global norm)."""
    total = sq_g[0]
    for t in range(1, sq_g.numel()):   # index order, as the kernel
        total = total + sq_g[t]
    norm = total.sqrt()
    if max_norm > 0:
        c = (max_norm / (norm + CLIP_EPS)).clamp(max=1.0)
    else:
        c = torch.ones_like(norm)
    ratio = torch.ones_like(sq_w)
    if lars:
        wn, gn = sq_w.sqrt(), sq_g.sqrt()
        adapt = (wn > 0) & (gn > 0) & ~torch.tensor(
            excluded, dtype=torch.bool, device=sq_w.device)
        trust = eta * wn / (c * gn + weight_decay * wn + LARS_EPS)
        ratio = torch.where(adapt, trust, ratio)
    return c.reshape(1), ratio, norm


def _update_torch(ws, grads, momentum_bufs, lr, momentum, weight_decay,
                  gscale, ratio, params16=None, emas=None,
                  ema_decay: float = 0.0) -> None:
    """The update in torch, same math (used on CPU and for parity tests), on
    the fp32 weights `ws`. With `params16` (the O2 path) `ws` are the masters
    of bf16 parameters, which get the rounded copy. With `emas` (one fp32
    average or None per weight) the new weights are averaged into them."""
    for i, (w, g) in enumerate(zip(ws, grads)):
        if params16 is not None:
            g = g.float()
        if gscale is not None:
            g = ratio[i] * (gscale[0] * g + weight_decay * w)
        elif weight_decay != 0:
            g = g.add(w, alpha=weight_decay)
        if momentum_bufs is not None:
            buf = momentum_bufs[i]
            buf.mul_(momentum).add_(g)
            g = buf
        w.add_(g, alpha=-lr)
        if params16 is not None:
            params16[i].copy_(w)
    if emas:
        ema_update_torch(emas, ws, ema_decay)


def fused_sgd_step(params: List[torch.Tensor], grads: List[torch.Tensor],
                   momentum_bufs: Optional[List[torch.Tensor]],
                   lr: float, momentum: float, weight_decay: float,
                   shadows: Optional[List[Optional[WeightShadow]]] = None,
                   gscale: Optional[torch.Tensor] = None,
                   ratio: Optional[torch.Tensor] = None,
                   emas: Optional[List[Optional[torch.Tensor]]] = None,
                   ema_decay: float = 0.0) -> None:
    """`shadows[i]` is params[i]'s WeightShadow or None. Each one is either
    rewritten with the new weight here (native path) or invalidated.

    With `gscale` ([1]) and `ratio` ([len(params)]) the update is the scaled
    one, d = ratio[i]*(gscale*g + wd*p); the gradients are not modified.

    With `emas` (one fp32 average or None per param) the same launch does
    emas[i] <- ema_decay*emas[i] + (1 - ema_decay)*p_new."""
    live = []
    for p, sh in zip(params, shadows or ()):
        if sh is None:
            continue
        if weight_shadows_wanted() and sh.matches(p):
            live.append((p, sh))
        else:
            sh.invalidate()
    if not (params and _backend.native_enabled(params[0])):
        for _, sh in live:
            sh.invalidate()
        _update_torch(params, grads, momentum_bufs, lr, momentum,
                      weight_decay, gscale, ratio, emas=emas,
                      ema_decay=ema_decay)
        return
    w16s = []
    if live:
        keep = {id(sh) for _, sh in live}
        w16s = [sh.w16 if sh is not None and id(sh) in keep else None
                for sh in shadows]
    bufs = momentum_bufs if momentum_bufs is not None else []
    # no averages: the call, and so the kernel, of a step without them
    ema_kw = dict(emas=emas, ema_decay=ema_decay) if emas else {}
    if gscale is None:
        _backend.C().multi_tensor_sgd(params, grads, bufs,
                                      lr, momentum, weight_decay, w16s,
                                      **ema_kw)
    else:
        _backend.C().multi_tensor_sgd_scaled(params, grads, bufs,
                                             lr, momentum, weight_decay,
                                             gscale, ratio, w16s, **ema_kw)
    if live:
        _backend.C().multi_tensor_build_wT([sh.w16 for _, sh in live],
                                           [sh.wT for _, sh in live])
        for p, sh in live:
            sh.mark_fresh(p)


def fused_sgd_o2_step(params: List[torch.Tensor], grads: List[torch.Tensor],
                      masters: List[torch.Tensor],
                      momentum_bufs: Optional[List[torch.Tensor]],
                      lr: float, momentum: float, weight_decay: float,
                      gscale: Optional[torch.Tensor] = None,
                      ratio: Optional[torch.Tensor] = None,
                      emas: Optional[List[Optional[torch.Tensor]]] = None,
                      ema_decay: float = 0.0) -> None:
    """bf16 params/grads, fp32 master + momentum (apex-O2 update); scaled as
    in fused_sgd_step when `gscale` and `ratio` are given. `emas` average the
    new masters."""
    if not (params and _backend.native_enabled(params[0])):
        _update_torch(masters, grads, momentum_bufs, lr, momentum,
                      weight_decay, gscale, ratio, params16=params,
                      emas=emas, ema_decay=ema_decay)
        return
    bufs = momentum_bufs if momentum_bufs is not None else []
    ema_kw = dict(emas=emas, ema_decay=ema_decay) if emas else {}
    if gscale is None:
        _backend.C().multi_tensor_sgd_o2(
            params, grads, masters, bufs, lr, momentum, weight_decay,
            **ema_kw)
    else:
        _backend.C().multi_tensor_sgd_o2_scaled(
            params, grads, masters, bufs, lr, momentum, weight_decay,
            gscale, ratio, **ema_kw)
