"""Exponential moving average of the weights (``trainer.ema_decay``), as its own launch behind the optimizer step.

    ema = ModelEMA(model, decay=0.9998)         # a deep copy of the bare module, kept in eval mode
    optimizer.step(); ema.update(optimizer)     # e += w * (p - e) for every parameter the optimizer can move
    ema.sync_untracked(); evaluate(ema.module)  # frozen parameters and buffers are copied from the live model, not averaged

Per element three float32 roundings, in this order: ``d = p - e``, ``t = w * d``, ``e' = e + t`` with ``w = float32(1 - d_t)``,
``d_t = min(decay, (1 + t) / (10 + t))`` under warm-up (``t`` = earlier ``update`` calls), else ``decay``.  On the GPU all tracked tensors
go through ONE ``mono_ema_update_f32`` launch (include/monosowa_pointwise.h) over a chunk table that is shipped once -- both address
columns are fixed, unlike the gradient tables -- and the launch consults the optimizer's guard record, so a step the guard skipped on
the device leaves the average untouched as well.  Anything else (CPU tensors, other dtypes or layouts) takes the same three roundings
through torch's ``sub`` / ``mul`` / ``add``.  ``t`` advances on a skipped step too: the host does not know about a device-side skip
(the deviation ``state["step"]`` of the guarded AdamW has)."""
import copy

import numpy as np
import torch

from .helpers.save_helper import unwrap


def _invalidate_derived():
    """The raw-pointer launch does not move the tensors' version counters: what the eval forward derives from parameters (folded
    convolution weights in backbone.py, the captured graphs of inference.py) is keyed on the module-level optimizer epoch."""
    from .monodetr import backbone
    if backbone._PARAM_EPOCH is not None:
        backbone._bump_param_epoch()


def ema_decay_at(decay, updates, warmup=True):
    """``d_t`` of update number ``updates`` (0-based), in Python floats."""
    return min(decay, (1 + updates) / (10 + updates)) if warmup else decay


def ema_weight(decay, updates, warmup=True):
    """``w = float32(1 - d_t)``: what multiplies ``p - e``."""
    return np.float32(1.0 - ema_decay_at(decay, updates, warmup))


def ema_fallback_(avgs, params, w):
    """``e += w * (p - e)`` through torch operations, each rounded to float32 on its own (no ``lerp``, no ``addcmul``): the bits of the
    kernel and of numpy in float32."""
    w = float(np.float32(w))
    with torch.no_grad():
        d = torch._foreach_sub(list(params), list(avgs))
        torch._foreach_mul_(d, w)
        torch._foreach_add_(list(avgs), d)


class EMAPlan:
    """Chunk table of ``mono_ema_update_f32`` over all tracked tensors: {average address, parameter address, count} per chunk of at most
    ``ADAM_CHUNK`` elements, written and copied to the device ONCE -- neither column moves between steps (``matches`` tells when one
    did)."""

    def __init__(self, avgs, params):
        from .pointwise import ADAM_CHUNK
        sizes = np.array([p.numel() for p in params], dtype=np.int64)
        per = (sizes + ADAM_CHUNK - 1) // ADAM_CHUNK
        tensor = np.repeat(np.arange(len(params)), per)
        first = np.cumsum(per) - per
        offset = (np.arange(per.sum()) - np.repeat(first, per)) * ADAM_CHUNK               # elements
        self.n_chunks = int(per.sum())
        self.device = params[0].device
        self.keys = (self._ptr(avgs), self._ptr(params), sizes)
        table = np.empty(self.n_chunks * (2 * 8 + 4), dtype=np.uint8)
        cols = table[:self.n_chunks * 16].view(np.uint64).reshape(2, self.n_chunks)
        cols[0] = self.keys[0][tensor] + (offset * 4).astype(np.uint64)
        cols[1] = self.keys[1][tensor] + (offset * 4).astype(np.uint64)
        table[self.n_chunks * 16:].view(np.int32)[:] = np.minimum(sizes[tensor] - offset, ADAM_CHUNK)
        # a pageable source: the copy has left the host buffer when copy_ returns, and it happens once
        self.dev = torch.from_numpy(table).to(self.device)
        self.launches = 0

    @staticmethod
    def _ptr(ts):
        return np.array([t.data_ptr() for t in ts], dtype=np.uint64)

    def matches(self, avgs, params):
        return len(params) == len(self.keys[2]) and np.array_equal(self.keys[0], self._ptr(avgs)) \
            and np.array_equal(self.keys[1], self._ptr(params)) and all(p.numel() == n for p, n in zip(params, self.keys[2]))

    def launch(self, w, record=None):
        from ._lib import on_device, raw_stream
        from .pointwise import load
        with on_device(self.device):
            code = load().mono_ema_update_f32(self.dev.data_ptr(), self.n_chunks, float(w), record, raw_stream())
        if code:
            raise RuntimeError("mono_ema_update_f32 failed with code %d" % code)
        self.launches += 1


class ModelEMA:
    def __init__(self, model, decay, warmup=True):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("ModelEMA: decay must lie in (0, 1), got %r" % decay)
        self.source = unwrap(model)
        # Parameter.__deepcopy__ clones with preserve_format: every averaged tensor has its parameter's strides
        self.module = copy.deepcopy(self.source).eval()
        self.decay, self.warmup, self.updates = decay, bool(warmup), 0
        self.plan = None
        self._flags = None
        self._pairs()

    def _pairs(self):
        """(averages, parameters) of the tracked tensors: the live parameters with ``requires_grad`` -- what the optimizer can move."""
        live = list(self.source.parameters())
        flags = tuple(p.requires_grad for p in live)
        if flags != self._flags:
            mine = list(self.module.parameters())
            assert len(mine) == len(live)
            self._flags = flags
            self._avgs = [e for e, f in zip(mine, flags) if f]
            self._params = [p for p, f in zip(live, flags) if f]
            self._frozen = [(e, p) for e, p, f in zip(mine, live, flags) if not f]
        return self._avgs, self._params

    def tracked(self):
        """{name: averaged tensor} of the tracked parameters."""
        return {n: e for (n, e), p in zip(self.module.named_parameters(), self.source.parameters()) if p.requires_grad}

    @torch.no_grad()
    def sync_untracked(self):
        """Frozen parameters and buffers of the copy := the live model's (they are not averaged).  Called whenever the module is handed
        out: for evaluation and for saving."""
        self._pairs()
        for e, p in self._frozen:
            e.copy_(p)
        for e, p in zip(self.module.buffers(), self.source.buffers()):
            e.copy_(p)
        self.module.eval()
        return self.module

    def weight(self):
        """``w`` of the next update."""
        return ema_weight(self.decay, self.updates, self.warmup)

    def update(self, optimizer=None):
        """One averaging step behind ``optimizer.step()``.  ``optimizer`` (the guarded AdamW): its guard record is handed to the kernel
        when the guard ran on the device this step, and under the guard's host fallback its own skip decision is honoured."""
        from .pointwise import accumulate_supported
        w = self.weight()
        self.updates += 1                                   # on a skipped step too: the host does not know about a device-side skip
        if optimizer is not None and getattr(optimizer, "last_step_skipped", lambda: False)():
            return
        avgs, params = self._pairs()
        if not avgs:
            return
        if accumulate_supported(avgs, params):              # dense float32 on one GPU, the parameters' strides
            if self.plan is None or not self.plan.matches(avgs, params):
                self.plan = EMAPlan(avgs, params)
            record = getattr(optimizer, "guard_record_address", lambda: None)() if optimizer is not None else None
            self.plan.launch(w, record)
        else:
            ema_fallback_(avgs, params, w)
        _invalidate_derived()

    def state_dict(self):
        self.sync_untracked()
        return {"module": self.module.state_dict(), "updates": self.updates, "decay": self.decay, "warmup": self.warmup}

    def load_state_dict(self, state):
        """In place: the averaged tensors keep their addresses, the chunk table stays valid."""
        self.module.load_state_dict(state["module"])
        self.updates, self.decay, self.warmup = int(state["updates"]), float(state["decay"]), bool(state["warmup"])
        _invalidate_derived()

    @torch.no_grad()
    def reset(self):
        """The average starts over from the live model's current weights (a checkpoint without an average): ``updates = 0``."""
        for e, p in zip(self.module.parameters(), self.source.parameters()):
            e.copy_(p)
        for e, p in zip(self.module.buffers(), self.source.buffers()):
            e.copy_(p)
        self.updates = 0
        _invalidate_derived()
