"""Optimizer construction and the reference's AdamW variant, evaluated with multi-tensor kernels.

Reference: lib/helpers/optimizer_helper.py -- ``build_optimizer`` :7-27 (biases get weight_decay 0),
``AdamW.step`` :69-129.  The update is NOT torch.optim.AdamW: eps is added to sqrt(v) before the bias
correction and the decay term is scaled by the bias-corrected step size:

    m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  denom = sqrt(v) + eps
    step_size = lr * sqrt(1-b2^t) / (1-b1^t)
    p = p - step_size * (wd*p + m/denom)

The reference loops over ~580 parameters in Python (about six tiny launches each); here the same
element-wise operations, in the same order, are issued through ``torch._foreach_*`` so a step is a
handful of launches.  State keys ('step','exp_avg','exp_avg_sq') match for checkpoint exchange.

Guarded step (``clip_max_norm`` / ``skip_nonfinite``, off by default, not in the reference): the global L2 norm of all
gradients is taken on the device, every gradient enters the update times ``min(max_norm / (norm + 1e-6), 1)`` and a step
whose gradients are not finite leaves parameters and moments untouched -- without a host synchronisation, see
``AdamW._guarded_step``.  Two stated deviations: ``p.grad`` is NOT rewritten (``clip_grad_norm_`` scales it in place), and
``state['step']`` advances on a skipped step too (the host does not know about the skip; only the bias correction sees it).
"""
import math

import torch
import torch.optim as optim
from torch.optim.optimizer import Optimizer


def build_optimizer(cfg_optimizer, model):
    weights, biases = [], []
    for name, param in model.named_parameters():
        (biases if "bias" in name else weights).append(param)
    parameters = [{"params": biases, "weight_decay": 0},
                  {"params": weights, "weight_decay": cfg_optimizer["weight_decay"]}]
    kind = cfg_optimizer["type"]
    clip = cfg_optimizer.get("clip_max_norm") or None          # absent, None or 0: off
    skip = bool(cfg_optimizer.get("skip_nonfinite", False))
    if (clip is not None or skip) and kind in ("sgd", "adam"):
        raise ValueError("optimizer.clip_max_norm / optimizer.skip_nonfinite apply to type 'adamw' only, not to '%s'" % kind)
    if kind == "sgd":
        return optim.SGD(parameters, lr=cfg_optimizer["lr"], momentum=0.9)
    if kind == "adam":
        return optim.Adam(parameters, lr=cfg_optimizer["lr"])
    if kind == "adamw":
        return AdamW(parameters, lr=cfg_optimizer["lr"], clip_max_norm=clip, skip_nonfinite=skip)
    raise NotImplementedError("%s optimizer is not supported" % kind)


class AdamW(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, clip_max_norm=None,
                 skip_nonfinite=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: {}".format(betas))
        if clip_max_norm is not None and not float(clip_max_norm) >= 0.0:
            raise ValueError("Invalid clip_max_norm: {}".format(clip_max_norm))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))
        # the guard belongs to the optimizer, not to a group (the norm is global) and not to the checkpoint
        self.clip_max_norm = float(clip_max_norm) if clip_max_norm else None
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard = None                      # pointwise.GradGuard once the device path has run
        self._guard_host = None                 # the fallback path's record
        self._step_record = None                # device address of the guard record when THIS step's guard ran on the device
        self._step_skipped = False              # the fallback path left THIS step out
        self._step_plans = None                 # the FusedAdamWPlans THIS step launched, in launch order; None: some bucket went through foreach

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
        for name in ("clip_max_norm", "_guard", "_guard_host", "_step_record", "_step_plans"):
            self.__dict__.setdefault(name, None)
        self.__dict__.setdefault("skip_nonfinite", False)
        self.__dict__.setdefault("_step_skipped", False)

    @property
    def guard_enabled(self):
        return self.clip_max_norm is not None or self.skip_nonfinite

    def _fused_plan(self, group, params, grads, exp_avgs, exp_avg_sqs):
        """The chunk table for one HIP launch over all parameters of the group (monosowa_amd/csrc/pointwise.hip adamw_kernel) when
        they are dense contiguous float32 GPU tensors, else None."""
        # element-wise over storage order: any dense layout works (channels_last convolution weights included) as long
        # as the parameter, its gradient and both moments share it
        def dense(t):
            return t.is_cuda and t.dtype == torch.float32 and (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)))
        if group["amsgrad"] or not params or not all(
                dense(p) and p.stride() == g.stride() == m.stride() == v.stride() and g.dtype == torch.float32 and g.is_cuda
                for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs)):
            return None
        from ..pointwise import FusedAdamWPlan
        plans = self.__dict__.setdefault("_fused_plans", {})
        key = id(group["params"])
        plan = plans.get(key)
        if plan is None or len(plan.keys[0]) != len(params) or not plan.matches(params, exp_avgs, exp_avg_sqs):
            plan = plans[key] = FusedAdamWPlan(params, exp_avgs, exp_avg_sqs, group["weight_decay"])
        return plan

    @staticmethod
    def _step_size(group, step):
        beta1, beta2 = group["betas"]
        return group["lr"] * math.sqrt(1 - beta2 ** step) / (1 - beta1 ** step)

    def _fused_step(self, group, step, params, grads, exp_avgs, exp_avg_sqs):
        """All parameters of the group in one HIP launch; same operations in the same order as the foreach formulation below."""
        plan = self._fused_plan(group, params, grads, exp_avgs, exp_avg_sqs)
        if plan is None:
            return False
        beta1, beta2 = group["betas"]
        plan.step(grads, beta1, beta2, group["eps"], self._step_size(group, step))
        if self._step_plans is not None:
            self._step_plans.append(plan)
        return True

    def _foreach_step(self, group, step, params, grads, exp_avgs, exp_avg_sqs, max_sqs):
        self._step_plans = None
        beta1, beta2 = group["betas"]
        torch._foreach_mul_(exp_avgs, beta1)
        torch._foreach_add_(exp_avgs, grads, alpha=1 - beta1)
        torch._foreach_mul_(exp_avg_sqs, beta2)
        torch._foreach_addcmul_(exp_avg_sqs, grads, grads, value=1 - beta2)
        if group["amsgrad"]:
            torch._foreach_maximum_(max_sqs, exp_avg_sqs)
            denom = torch._foreach_sqrt(max_sqs)
        else:
            denom = torch._foreach_sqrt(exp_avg_sqs)
        torch._foreach_add_(denom, group["eps"])
        update = torch._foreach_mul(params, group["weight_decay"])
        torch._foreach_addcdiv_(update, exp_avgs, denom, value=1)
        torch._foreach_add_(params, update, alpha=-self._step_size(group, step))

    def _guarded_step(self, work):
        """The step under the guard for ``work`` = [(group, step, params, grads, exp_avgs, exp_avg_sqs, max_sqs)] of ALL groups.
        Device path (every bucket served by the fused kernel, one device, at most 8 tables): the tables of all groups are refreshed,
        ``mono_grad_guard_f32`` runs once over all of them, then one guarded AdamW launch per table consults its record -- nothing
        here waits for the device.  Anything else (CPU tensors, non-dense layouts, amsgrad) takes the same semantics through torch
        operations, which may synchronise."""
        from ..pointwise import GUARD_MAX_GROUPS, GradGuard
        plans = [self._fused_plan(w[0], *w[2:6]) for w in work]
        if all(p is not None for p in plans) and len(plans) <= GUARD_MAX_GROUPS and len({p.device for p in plans}) == 1:
            for plan, w in zip(plans, work):
                plan.refresh(w[3])
            if self._guard is None or self._guard.device != plans[0].device:
                self._guard = GradGuard(plans[0].device)
            self._guard_host = None
            self._guard.run(plans, self.clip_max_norm, self.skip_nonfinite)
            record = self._step_record = self._guard.record.data_ptr()
            for plan, (group, step) in zip(plans, (w[:2] for w in work)):
                plan.launch(group["betas"][0], group["betas"][1], group["eps"], self._step_size(group, step), record)
            self._step_plans = plans
            return
        self._step_plans = None                            # a skipped step launches nothing at all: not a fused one either
        grads = [g for w in work for g in w[3]]
        sumsq = torch.stack([g.detach().double().pow(2).sum().to(grads[0].device) for g in grads]).sum()
        norm = sumsq.sqrt().float()
        if self.clip_max_norm is not None:                 # clip_grad_norm_'s f32 arithmetic; fmin like the kernel's fminf
            coef = torch.fmin(self.clip_max_norm / (norm + 1e-6), torch.ones_like(norm))
        else:
            coef = torch.ones_like(norm)
        host = self._guard_host or {"skipped_total": self._guard.report()["skipped_total"] if self._guard is not None else 0}
        self._guard, self._guard_host = None, host
        host["grad_norm"], host["coef"] = norm, coef
        if self.skip_nonfinite and not bool(torch.isfinite(sumsq)):
            host["skipped_total"] += 1
            self._step_skipped = True
            return
        for group, step, params, grads, exp_avgs, exp_avg_sqs, max_sqs in work:
            if self.clip_max_norm is not None:
                grads = [g * coef.to(g.device) for g in grads]
            self._foreach_step(group, step, params, grads, exp_avgs, exp_avg_sqs, max_sqs)

    def guard_report(self):
        """``{"grad_norm", "coef", "skipped_total"}`` of the last guarded step (None before the first one or with the guard off).
        Reads the device record: a host synchronisation, for the places that wait for the device anyway."""
        if self._guard_host is not None:
            h = self._guard_host
            return {"grad_norm": float(h["grad_norm"]), "coef": float(h["coef"]), "skipped_total": int(h["skipped_total"])}
        if self._guard is None:
            return None
        r = self._guard.report()
        return {"grad_norm": r["grad_norm"], "coef": r["coef"], "skipped_total": r["skipped_total"]}

    def guard_record_address(self):
        """Device address of the guard record the LAST step's kernels consulted (``mono_grad_guard_f32`` ran on the device in that
        step), else None: what a launch behind the step -- the weight average -- hands to its kernel so that it skips with the step."""
        return self._step_record

    def last_fused_plans(self):
        """The ``FusedAdamWPlan``s the LAST step launched, in launch order, their tables refreshed for that step's gradients -- what a
        launch behind the step reads the step's parameter, gradient and count columns from.  None when any bucket of that step took
        the foreach path (CPU tensors, ``amsgrad``, non-dense layouts) or no step has run; an empty list when no parameter had a
        gradient."""
        return None if self._step_plans is None else list(self._step_plans)

    def last_step_skipped(self):
        """True when the guard's host fallback left the LAST step out.  A skip decided on the device is not known here (False): there
        ``guard_record_address()`` is what follows it."""
        return self._step_skipped

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        self._step_record, self._step_skipped, self._step_plans = None, False, []
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []         # under the guard: the buckets of ALL groups (the norm is global), stepped together at the end
        for group in self.param_groups:
            buckets = {}      # step count -> lists (all equal in practice: one bucket)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                    if group["amsgrad"]:
                        state["max_exp_avg_sq"] = torch.zeros_like(p)
                state["step"] += 1
                b = buckets.setdefault(int(state["step"]), ([], [], [], [], []))
                b[0].append(p)
                b[1].append(p.grad)
                b[2].append(state["exp_avg"])
                b[3].append(state["exp_avg_sq"])
                if group["amsgrad"]:
                    b[4].append(state["max_exp_avg_sq"])
            for step, (params, grads, exp_avgs, exp_avg_sqs, max_sqs) in buckets.items():
                if self.guard_enabled:
                    work.append((group, step, params, grads, exp_avgs, exp_avg_sqs, max_sqs))
                elif not self._fused_step(group, step, params, grads, exp_avgs, exp_avg_sqs):
                    self._foreach_step(group, step, params, grads, exp_avgs, exp_avg_sqs, max_sqs)
        if work:
            self._guarded_step(work)
        return loss
