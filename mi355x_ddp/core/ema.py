"""Weight EMA for evaluation and deployment (`--ema_decay`).

The averages themselves are kept by `FusedSGD` (ops/sgd.py): one fp32 average
per stepped parameter in ``optimizer.state[p]["ema"]``, written by the kernel
that produces the new weight, and the averages of the tensors handed to
`FusedSGD.track_buffers`, written by one more launch at the end of `step()`.
`WeightEMA` owns the second kind for a model's floating-point buffers (the
BatchNorm running statistics; `num_batches_tracked` is a counter and is
neither averaged nor swapped), and puts the averaged model in the live model's
place:

    ema = WeightEMA(model, optimizer)
    with ema.swapped():
        validate(model, ...)          # the averaged weights and statistics
    torch.save(ema.state_dict(), f)   # loads into build_model(arch)

The swap is in place (`copy_`), so every pointer stays what it was: FlatDDP's
views, the static memory of a captured step and the conv weight shadows keep
working, and after the context every tensor is bit for bit what it was before.
It runs twice per evaluation and is plain torch.

Not here: decay warm-up or schedules, averaging every N steps, evaluating both
weight sets per epoch.
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from typing import Dict, Iterator, List, Tuple

import torch

from ..ops.conv import shadow_of, weight_shadows_wanted


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


class WeightEMA:
    def __init__(self, model, optimizer):
        self.module = _unwrap(model)
        self.optimizer = optimizer
        self._depth = 0   # nesting of swapped()
        # name -> (buffer, its average), in the module's order
        self.buffers: "OrderedDict[str, Tuple[torch.Tensor, torch.Tensor]]" \
            = OrderedDict()
        for name, buf in self.module.named_buffers():
            if buf.is_floating_point():
                self.buffers[name] = (buf, buf.detach().clone())
        optimizer.track_buffers(list(self.buffers.values()))

    # ---- the pairs ----------------------------------------------------------

    def _param_pairs(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor,
                                             torch.Tensor]]:
        """(parameter, its fp32 weight, that weight's average) of every
        parameter that has an average. The fp32 weight is the parameter
        itself, or the O2 master of a bf16 parameter."""
        for group in self.optimizer.param_groups:
            for p in group["params"]:
                state = self.optimizer.state.get(p)
                if not state or "ema" not in state:
                    continue
                yield p, state.get("master", p), state["ema"]

    @torch.no_grad()
    def _exchange(self) -> None:
        for p, w, e in self._param_pairs():
            tmp = w.detach().clone()
            w.copy_(e)        # bumps p._version for an fp32 parameter
            e.copy_(tmp)
            if w is not p:
                p.copy_(w)    # O2: the bf16 parameter is the rounded master
        for buf, avg in self.buffers.values():
            tmp = buf.clone()
            buf.copy_(avg)
            avg.copy_(tmp)

    @torch.no_grad()
    def _refresh_shadows(self) -> None:
        """Rewrites, in place, the conv weight shadows that the evaluation
        forward filled with the averaged weights. The next eager forward would
        do it by the version stamp; a captured step does not look at stamps."""
        if not weight_shadows_wanted():
            return
        for p, _, _ in self._param_pairs():
            sh = shadow_of(p)
            if sh is not None and sh.matches(p):
                sh.ensure(p)

    @contextlib.contextmanager
    def swapped(self):
        """The model holds the averages inside the context and its own
        weights, bit for bit, after it. Nested uses are one swap; an exception
        in the body still restores. Parameters without an average yet (before
        the first optimizer step) are left alone."""
        if self._depth == 0:
            self._exchange()
        self._depth += 1
        try:
            yield self
        finally:
            self._depth -= 1
            if self._depth == 0:
                self._exchange()
                self._refresh_shadows()

    # ---- the averaged model ---------------------------------------------------

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The averaged model under the model's own keys: averaged fp32
        weights (the live weight where there is no average yet), averaged
        running statistics, the live `num_batches_tracked`. Copies."""
        inside = self._depth > 0   # then the live tensors hold the averages
        avg_of = {}
        for p, w, e in self._param_pairs():
            avg_of[id(p)] = w if inside else e
        for buf, avg in self.buffers.values():
            avg_of[id(buf)] = buf if inside else avg
        out = OrderedDict()
        for key, v in self.module.state_dict(keep_vars=True).items():
            out[key] = avg_of.get(id(v), v).detach().clone()
        return out

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Restores the buffer averages from a `state_dict()`. The parameter
        averages are optimizer state and come back with it."""
        if self._depth > 0:
            raise RuntimeError("WeightEMA.load_state_dict inside swapped()")
        missing: List[str] = [k for k in self.buffers if k not in sd]
        if missing:
            raise KeyError(f"WeightEMA state lacks buffer averages: {missing}")
        for key, (_, avg) in self.buffers.items():
            avg.copy_(sd[key])

    @torch.no_grad()
    def reset_buffers(self) -> None:
        """Starts the buffer averages again from the model's current
        statistics (after loading a checkpoint that has no averages)."""
        for buf, avg in self.buffers.values():
            avg.copy_(buf)
