"""The guarded AdamW step (``clip_max_norm`` / ``skip_nonfinite``) where it needs no GPU: the configuration keys, and the torch
fallback path of ``AdamW._guarded_step`` -- the same semantics as the device path (tests/test_guarded_step_gpu.py): the global
gradient norm from exact float64 squares, ``clip_grad_norm_``'s float32 coefficient, the reference's AdamW update on the scaled
gradients, and a step with non-finite gradients left out whole."""
import math

import numpy as np
import pytest
import torch

from monosowa_amd.helpers.optimizer_helper import AdamW, build_optimizer

SHAPES = [(7, 5), (5,), (3, 4, 2), (1,), (33,)]
LR, WD = 2e-4, 1e-4


def _reference_adamw_step(params, grads, states, lr, wd, step, b1=0.9, b2=0.999, eps=1e-8):
    """lib/helpers/optimizer_helper.py:69-129 of the reference, per parameter (tests/test_helpers.py restates it the same way)."""
    for p, g, st in zip(params, grads, states):
        st["m"].mul_(b1).add_(g, alpha=1 - b1)
        st["v"].mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = st["v"].sqrt().add_(eps)
        step_size = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        p.add_(torch.mul(p, wd).addcdiv_(st["m"], denom, value=1), alpha=-step_size)


def _clip_f64(grads, max_norm):
    """(norm, coef) as float32: the norm from a correctly rounded float64 sum of the exact squares, the coefficient by
    ``clip_grad_norm_``'s arithmetic in float32."""
    squares = np.concatenate([g.numpy().astype(np.float64).ravel() for g in grads]) ** 2        # exact: 24-bit factors
    norm = np.float32(math.sqrt(math.fsum(squares)))
    coef = np.minimum(np.float32(max_norm) / (norm + np.float32(1e-6)), np.float32(1.0))
    return norm, np.float32(coef)


def _setup(**guard):
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    opt = AdamW([{"params": ps[:2], "weight_decay": 0}, {"params": ps[2:], "weight_decay": WD}], lr=LR, **guard)
    ref = [p.detach().clone() for p in ps]
    st = [{"m": torch.zeros_like(p), "v": torch.zeros_like(p)} for p in ref]
    return ps, opt, ref, st


def test_build_optimizer_reads_the_guard_keys():
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.LayerNorm(4))
    base = {"type": "adamw", "lr": 1e-3, "weight_decay": 0.1}
    opt = build_optimizer(base, m)
    assert opt.clip_max_norm is None and opt.skip_nonfinite is False and not opt.guard_enabled and opt.guard_report() is None
    for off in (None, 0, 0.0):
        opt = build_optimizer(dict(base, clip_max_norm=off), m)
        assert opt.clip_max_norm is None and not opt.guard_enabled
    opt = build_optimizer(dict(base, clip_max_norm=0.1), m)
    assert opt.clip_max_norm == 0.1 and opt.skip_nonfinite is False and opt.guard_enabled
    opt = build_optimizer(dict(base, skip_nonfinite=True), m)
    assert opt.clip_max_norm is None and opt.skip_nonfinite is True and opt.guard_enabled
    opt = build_optimizer(dict(base, clip_max_norm=35, skip_nonfinite=True), m)
    assert opt.clip_max_norm == 35.0 and opt.skip_nonfinite is True
    assert set(opt.state_dict()["param_groups"][0]) == set(build_optimizer(base, m).state_dict()["param_groups"][0])   # checkpoint format
    with pytest.raises(ValueError):
        AdamW(m.parameters(), clip_max_norm=-1.0)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("key", [{"clip_max_norm": 0.1}, {"skip_nonfinite": True}])
def test_guard_keys_are_refused_for_other_optimizers(kind, key):
    m = torch.nn.Linear(3, 4)
    base = {"type": kind, "lr": 1e-3, "weight_decay": 0.1}
    build_optimizer(base, m)
    build_optimizer(dict(base, clip_max_norm=None, skip_nonfinite=False), m)          # switched off: as absent
    with pytest.raises(ValueError):
        build_optimizer(dict(base, **key), m)


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_fallback_clips_like_float64_then_reference_adamw(max_norm):
    ps, opt, ref, st = _setup(clip_max_norm=max_norm, skip_nonfinite=True)
    for step in range(1, 4):
        gs = [torch.randn_like(p) * step for p in ps]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        norm, coef = _clip_f64(gs, max_norm)
        assert (coef < 1.0) == (max_norm == 0.5)
        report = opt.guard_report()
        assert np.float32(report["grad_norm"]) == norm and np.float32(report["coef"]) == coef and report["skipped_total"] == 0
        scaled = [torch.from_numpy(g.numpy() * coef) for g in gs]
        _reference_adamw_step(ref[:2], scaled[:2], st[:2], LR, 0, step)
        _reference_adamw_step(ref[2:], scaled[2:], st[2:], LR, WD, step)
        for p, g, r in zip(ps, gs, ref):
            assert torch.equal(p.detach(), r)
            assert torch.equal(p.grad, g)                 # the gradients themselves are not rewritten
    for p, s in zip(ps, st):
        assert torch.equal(opt.state[p]["exp_avg"], s["m"]) and torch.equal(opt.state[p]["exp_avg_sq"], s["v"])
    assert set(opt.state_dict()["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_fallback_skips_a_non_finite_step(bad):
    ps, opt, ref, st = _setup(clip_max_norm=0.5, skip_nonfinite=True)
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    for p in ps:
        p.grad = torch.randn_like(p)
    ps[-1].grad[-1] = bad
    opt.step()
    for p, (p0, m0, v0) in zip(ps, before):
        assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]["exp_avg"], m0) and torch.equal(opt.state[p]["exp_avg_sq"], v0)
    assert opt.guard_report()["skipped_total"] == 1
    assert opt.state[ps[0]]["step"] == 2                  # the stated deviation: the count advances on a skipped step too
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()
    assert opt.guard_report()["skipped_total"] == 1 and math.isfinite(opt.guard_report()["grad_norm"])
    assert all(not torch.equal(p.detach(), p0) and torch.isfinite(p).all() for p, (p0, _, _) in zip(ps, before))


def test_skip_alone_does_not_scale():
    ps, opt, ref, st = _setup(skip_nonfinite=True)
    for step in range(1, 3):
        gs = [torch.randn_like(p) * 100 for p in ps]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        _reference_adamw_step(ref[:2], gs[:2], st[:2], LR, 0, step)
        _reference_adamw_step(ref[2:], gs[2:], st[2:], LR, WD, step)
        assert all(torch.equal(p.detach(), r) for p, r in zip(ps, ref))
        assert opt.guard_report()["coef"] == 1.0


def test_without_the_keys_the_step_is_the_foreach_formulation_bitwise():
    ps, opt, ref, st = _setup()
    for step in range(1, 4):
        gs = [torch.randn_like(p) for p in ps]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        for lo, hi, wd in ((0, 2, 0), (2, len(ps), WD)):              # AdamW.step's foreach operations, restated
            P, G = ref[lo:hi], gs[lo:hi]
            M, V = [s["m"] for s in st[lo:hi]], [s["v"] for s in st[lo:hi]]
            torch._foreach_mul_(M, 0.9)
            torch._foreach_add_(M, G, alpha=1 - 0.9)
            torch._foreach_mul_(V, 0.999)
            torch._foreach_addcmul_(V, G, G, value=1 - 0.999)
            denom = torch._foreach_sqrt(V)
            torch._foreach_add_(denom, 1e-8)
            step_size = LR * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
            update = torch._foreach_mul(P, wd)
            torch._foreach_addcdiv_(update, M, denom, value=1)
            torch._foreach_add_(P, update, alpha=-step_size)
        for p, r, s in zip(ps, ref, st):
            assert torch.equal(p.detach(), r)
            assert torch.equal(opt.state[p]["exp_avg"], s["m"]) and torch.equal(opt.state[p]["exp_avg_sq"], s["v"])
    assert opt.guard_report() is None


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _bare_trainer(optimizer):
    from monosowa_amd.helpers.trainer_helper import Trainer
    t = object.__new__(Trainer)
    t.optimizer, t.logger, t._guard_skipped = optimizer, _Log(), 0
    return t


def test_trainer_counts_skipped_steps_and_refuses_a_dead_epoch():
    ps, opt, _, _ = _setup(skip_nonfinite=True)
    t = _bare_trainer(opt)

    def steps(bad):
        for b in bad:
            for p in ps:
                p.grad = torch.randn_like(p)
            if b:
                ps[0].grad[0, 0] = float("nan")
            opt.step()

    steps([False, True, False])
    t._check_guard(0, 3)
    assert t.logger.lines == ["Epoch 0: 1 of 3 steps skipped (non-finite gradients)"]
    steps([True, True])
    with pytest.raises(RuntimeError, match="every step of epoch 1"):
        t._check_guard(1, 2)                             # the epoch's own count, not the running total
    steps([False, False])
    t._check_guard(2, 2)
    assert t.logger.lines[-1] == "Epoch 2: 0 of 2 steps skipped (non-finite gradients)"


def test_trainer_says_nothing_about_the_guard_without_the_keys():
    ps, opt, _, _ = _setup()
    t = _bare_trainer(opt)
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()
    assert t._guard_report() is None
    t._check_guard(0, 1)
    assert t.logger.lines == []
    t.optimizer = torch.optim.SGD(ps, lr=0.1)            # an optimizer that has no guard at all
    assert t._guard_report() is None
