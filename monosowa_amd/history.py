"""Per-step training record kept on the device (``trainer.history``): the loss terms, per module group the gradient norm, the parameter
norm and the number of non-finite gradient elements, and the guard's verdict -- one row per optimizer step, no host synchronisation
in the step.

    hist = StepHistory(model, weight_dict, capacity)            # capacity: optimizer steps kept before a drain
    hist.add_losses(loss_dict, total, scale=1.0)                # once per micro-batch; scale = 1 / K under accumulation
    optimizer.step()
    hist.commit(optimizer, epoch=e, step=s, lr=lr, micro_batches=K)      # right behind the step, in front of ema.update()
    rows = hist.drain()                                         # the only call that waits for the device; oldest row first

The ring is a ``[capacity, F]`` float64 device tensor, zeroed at allocation and after every drain.  The columns of a row:

* one per key of ``weight_dict`` that the first ``loss_dict`` holds, in ``weight_dict`` order: the raw, unweighted term, and one more,
  ``loss_detr``, for the ``total`` handed in.  ``add_losses`` does ``row[j] += float64(term_j) * scale`` on the device (one stack of
  the terms, one mixed-precision in-place add); with ``scale = 1`` the stored value is exactly ``float64(term)``.  ``scale`` applies to
  the term columns alone: ``total`` is added as handed in, because under accumulation the Trainer's total already carries its 1 / K.
* three per module group: ``grad_sumsq``, ``param_sumsq`` (both sums of exact float64 products) and ``grad_nonfinite``, over the tensors
  as the optimizer saw them -- after accumulation and DDP's all-reduce, before any clipping -- and the parameters after the step (the
  untouched ones when the guard skipped it).  Only parameters with a gradient in the step enter; a group without one reports zeros.
* ``guard_norm``, ``guard_coef``, ``guard_skip``: the guard record of the step when the guard ran on the device, else zeros (and left out
  of the drained row).

On the GPU the group columns come from ``mono_step_stats_f32`` (include/monosowa_pointwise.h): two launches over the chunk tables the
fused AdamW step has just used (``AdamW.last_fused_plans()``), so no second per-step table is shipped; the group id of every chunk is a
device array built once per table.  When the optimizer's last step was not fully fused (CPU tensors, ``amsgrad``, ``sgd`` / ``adam``,
non-dense layouts) the same columns are computed through torch operations in float64 (``_fallback``); that path may synchronise.

``epoch``, ``step``, ``lr`` and ``micro_batches`` never travel to the device: they wait in a host list and are joined at ``drain()``.
A ``commit`` (or ``add_losses``) on a full ring first drains it into a host backlog -- a synchronisation; size ``capacity`` to the steps
between two drains and it never happens."""
import json
import math
import re

import numpy as np
import torch

from .helpers.save_helper import unwrap

MAX_GROUPS = 64
_LAYER = re.compile(r"^backbone\.0\.body\.(layer\d+)\.")


def default_group(name):
    """``backbone.0.body.layerN.*`` -> ``backbone.layerN``; ``depthaware_transformer.X.*`` -> ``depthaware_transformer.X``; everything
    else by its first dotted component."""
    m = _LAYER.match(name)
    if m:
        return "backbone." + m.group(1)
    parts = name.split(".")
    if parts[0] == "depthaware_transformer" and len(parts) > 2:
        return "depthaware_transformer." + parts[1]
    return parts[0]


def jsonable(value):
    """``value`` with every non-finite float replaced by the string ``"nan"``, ``"inf"`` or ``"-inf"``: what ``json.dumps`` writes as
    valid JSON."""
    if isinstance(value, dict):
        return {k: jsonable(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [jsonable(v) for v in value]
    if isinstance(value, (float, np.floating)):
        value = float(value)
        if math.isnan(value):
            return "nan"
        if math.isinf(value):
            return "inf" if value > 0 else "-inf"
        return value
    if isinstance(value, np.integer):
        return int(value)
    return value


def to_json(row):
    """One drained row as one line of valid JSON."""
    return json.dumps(jsonable(row), allow_nan=False)


class StepHistory:
    def __init__(self, model, weight_dict, capacity, group_of=None):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("StepHistory: capacity must be at least 1, got %r" % capacity)
        self.module = unwrap(model)
        self.weight_keys = list(weight_dict)
        self.capacity = capacity
        names, self._group_of_param = [], {}
        for name, p in self.module.named_parameters():
            g = (group_of or default_group)(name)
            if g not in names:
                names.append(g)
            self._group_of_param[id(p)] = names.index(g)
        if not names:
            raise ValueError("StepHistory: the model has no parameters")
        if len(names) > MAX_GROUPS:
            raise ValueError("StepHistory: %d module groups, at most %d are kept (pass a coarser group_of)" % (len(names), MAX_GROUPS))
        self.groups = names
        self.device = next(self.module.parameters()).device
        self.loss_keys = None            # fixed by the first loss_dict
        self.ring = None                 # allocated with it: [capacity, F] float64
        self._meta = []                  # host side of the rows in the ring: (epoch, step, lr, micro_batches, guard on the device?)
        self._backlog = []               # rows drained early by a commit on a full ring
        self._arrays = {}                # id(FusedAdamWPlan) -> (plan, device int32 group id per chunk)
        self._partials = None
        self.kernel_commits = 0          # commits served by mono_step_stats_f32

    # ------------------------------------------------------------------------------------------------------------------ losses
    def _begin(self, loss_dict):
        self.loss_keys = [k for k in self.weight_keys if k in loss_dict]
        self._key_set = set(loss_dict.keys())
        self.n_loss = len(self.loss_keys) + 1
        self.width = self.n_loss + 3 * len(self.groups) + 3
        self.ring = torch.zeros(self.capacity, self.width, dtype=torch.float64, device=self.device)

    def _make_room(self):
        if len(self._meta) >= self.capacity:
            self._backlog.extend(self._collect())

    def add_losses(self, loss_dict, total, scale=1.0):
        """``row[j] += float64(term_j) * scale`` for the term columns of the open row and ``row[loss_detr] += float64(total)``:
        ``scale`` is for the raw terms alone, ``total`` enters as it is handed in (under accumulation the caller's total already
        carries its 1 / K).  One stack of the values and one in-place add that widens to float64 as it reads -- two launches; with
        ``scale != 1`` the total's column takes an add of its own, three.  Nothing waits for the device."""
        if self.loss_keys is None:
            self._begin(loss_dict)
        elif set(loss_dict.keys()) != self._key_set:
            raise ValueError("StepHistory.add_losses: the keys of this loss_dict differ from the first one's in %r"
                             % sorted(set(loss_dict.keys()) ^ self._key_set))
        self._make_room()
        peek = getattr(loss_dict, "peek", loss_dict.__getitem__)
        with torch.no_grad():
            terms = [torch.as_tensor(peek(k)).detach().reshape(()) for k in self.loss_keys] + [torch.as_tensor(total).detach().reshape(())]
            vals = torch.stack([t if t.device == self.device else t.to(self.device) for t in terms])
            row = self.ring[len(self._meta)]
            if float(scale) == 1.0:
                row[:self.n_loss].add_(vals)
            else:
                row[:self.n_loss - 1].add_(vals[:-1], alpha=float(scale))
                row[self.n_loss - 1:self.n_loss].add_(vals[-1:])

    # ------------------------------------------------------------------------------------------------------------------ commit
    def _group_array(self, plan):
        """Device int32 group id of every chunk of ``plan``, built once per plan (and again when the optimizer re-makes the plan)."""
        hit = self._arrays.get(id(plan))
        if hit is not None and hit[0] is plan:
            return hit[1]
        by_ptr = {p.data_ptr(): self._group_of_param[id(p)] for p in self.module.parameters() if id(p) in self._group_of_param}
        try:
            per_tensor = np.array([by_ptr[int(ptr)] for ptr in plan.keys[0]], dtype=np.int32)
        except KeyError:
            raise ValueError("StepHistory.commit: the optimizer steps a parameter that is not one of the model's") from None
        arr = torch.from_numpy(per_tensor[plan.tensor]).to(plan.device)
        self._arrays = {k: v for k, v in self._arrays.items() if k == id(plan) or v[0] is not plan}
        self._arrays[id(plan)] = (plan, arr)
        return arr

    def _fallback(self, optimizer, out):
        """The group columns through torch operations in float64, over every parameter of the optimizer that has a gradient.  May
        synchronise (and does on a GPU)."""
        idx, stats = [], []
        for group in optimizer.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if id(p) not in self._group_of_param:
                    raise ValueError("StepHistory.commit: the optimizer steps a parameter that is not one of the model's")
                g = p.grad.detach()
                g64, p64 = g.to(torch.float64), p.detach().to(torch.float64)
                stats.append(torch.stack([(g64 * g64).sum(), (p64 * p64).sum(), (~torch.isfinite(g)).sum().to(torch.float64)]).to(self.device))
                idx.append(self._group_of_param[id(p)])
        if not stats:
            return
        table = torch.zeros(len(self.groups), 3, dtype=torch.float64, device=self.device)
        table.index_add_(0, torch.tensor(idx, dtype=torch.long).to(self.device), torch.stack(stats))
        out[:3 * len(self.groups)].copy_(table.reshape(-1))

    def commit(self, optimizer, epoch=0, step=0, lr=None, micro_batches=1):
        """Closes the open row behind ``optimizer.step()``: the group columns and the guard record are written on the device, the
        host values wait in a list.  No synchronisation on the kernel path (after the first call, which ships the group ids)."""
        if self.loss_keys is None:
            self._begin({})
        self._make_room()
        row = len(self._meta)
        plans = getattr(optimizer, "last_fused_plans", lambda: None)()
        record = None
        if plans is not None and all(p.device == self.device for p in plans) and len(plans) <= 8:
            record = getattr(optimizer, "guard_record_address", lambda: None)()
            if plans:
                from .pointwise import step_stats
                arrays = [self._group_array(p) for p in plans]
                need = 3 * sum(p.n_chunks for p in plans)
                if self._partials is None or self._partials.numel() < need:
                    self._partials = torch.empty(need, dtype=torch.float64, device=self.device)
                out = self.ring.data_ptr() + 8 * (row * self.width + self.n_loss)
                step_stats(plans, arrays, len(self.groups), record, self._partials, out)
                self.kernel_commits += 1
            else:
                record = None
        else:
            with torch.no_grad():
                self._fallback(optimizer, self.ring[row, self.n_loss:])
        self._meta.append((int(epoch), int(step), None if lr is None else float(lr), int(micro_batches), record is not None))

    # ------------------------------------------------------------------------------------------------------------------ drain
    def _collect(self):
        """The committed rows of the ring as dicts; the ring is zeroed.  Waits for the device.  Under ``torch.distributed`` with more
        than one rank the loss columns are averaged over the ranks first, by one all-reduce (every rank has to call this)."""
        n = len(self._meta)
        if n == 0:
            return []
        from .monodetr import misc
        if misc.is_dist_avail_and_initialized() and misc.get_world_size() > 1:
            losses = self.ring[:n, :self.n_loss].contiguous()
            torch.distributed.all_reduce(losses)
            self.ring[:n, :self.n_loss] = losses / misc.get_world_size()
        host = self.ring[:n].to("cpu", copy=True).numpy()             # a copy on the CPU too: the ring is zeroed next
        self.ring.zero_()
        rows, G = [], len(self.groups)
        for (epoch, step, lr, micro, guarded), r in zip(self._meta, host):
            stats = r[self.n_loss:self.n_loss + 3 * G].reshape(G, 3)
            with np.errstate(invalid="ignore"):
                norms = np.sqrt(stats[:, :2])
            row = {"epoch": epoch, "step": step, "lr": lr, "micro_batches": micro,
                   "losses": {k: float(v) for k, v in zip(self.loss_keys, r)},
                   "loss_detr": float(r[self.n_loss - 1]),
                   "grad_norm": {g: float(v) for g, v in zip(self.groups, norms[:, 0])},
                   "param_norm": {g: float(v) for g, v in zip(self.groups, norms[:, 1])},
                   "grad_nonfinite": {g: int(v) for g, v in zip(self.groups, stats[:, 2])}}
            if guarded:
                norm, coef, skip = r[self.n_loss + 3 * G:]
                row["guard"] = {"norm": float(norm), "coef": float(coef), "skip": int(skip)}
            rows.append(row)
        self._meta = []
        return rows

    def drain(self):
        """Every row since the last drain, oldest first, as a list of dicts; the ring starts over.  The only call that is meant to
        wait for the device."""
        if self.ring is None:
            return []
        rows, self._backlog = self._backlog + self._collect(), []
        return rows
