"""``trainer.global_batch`` on the GPU: the accumulation kernel alone (``mono_grad_accumulate_f32``), and cycles of K = 2 of the shipped
architecture (dropout 0) at 640 x 192, per-GPU batch 2 -- linear in the micro-batch gradients to the last bit under the deterministic
flag, the cycle-wide normaliser against each micro-batch's own, the guard on the accumulated gradient, no host synchronisation, and
nothing changed with the key at K = 1.

The depth predictor keeps a hard-coded dropout of 0.1: a forward pre-hook seeds torch's generator (and the native kernels' seed
counters) with 100 + micro-step index on both sides of every comparison."""
import copy
import logging
import os
import warnings

import numpy as np
import pytest
import torch
import yaml

from test_train_step_grads_gpu import BOUND_BACKBONE, BOUND_HEADS, _group, _mode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (640, 192)
CHUNK = 32768


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------------------- 5. kernel alone
SENTINEL = 12345.0
# (acc, g) pairs whose sum is special: signed zeros, Inf - Inf, Inf, NaN operands, overflow, subnormal results, cancellation to zero
SPECIAL = [(0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (np.inf, -np.inf), (np.inf, 1.0), (-np.inf, -np.inf), (np.nan, 1.0), (1.0, np.nan),
           (1e38, 1e38), (-1e38, -1e38), (1e-45, 1e-45), (1e-39, -3e-40), (1.17549435e-38, -1e-45), (3e-39, 3e-39), (1.5, -1.5),
           (16777216.0, 1.0)]


def _kernel_layout():
    """[(shape, first element in the accumulator buffer, first element in the gradient buffer, channels_last)] and the buffer length:
    tensors start on 16-byte boundaries (or, where asked, one element past one) with at least one sentinel element between them."""
    spec = [((n,), 0, 0, False) for n in (1, 3, 4, 5, 255, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)]
    spec += [((1031,), 1, 1, False), ((1031,), 1, 0, False), ((1031,), 0, 1, False), ((8, 3, 3, 5), 0, 0, True)]
    out, cursor = [], 1
    for shape, sa, sg, cl in spec:
        start = (cursor + 1 + 3) // 4 * 4
        out.append((shape, start + sa, start + sg, cl))
        cursor = start + 1 + int(np.prod(shape))
    for _ in range(600):                                   # 7 elements every 9: every alignment, one or two sentinels between
        out.append(((7,), cursor + 1, cursor + 1, False))
        cursor += 9
    return out, cursor + 8


def _view(buf, start, shape, cl):
    n = int(np.prod(shape))
    flat = buf[start:start + n]
    if cl:
        N, C, H, W = shape
        t = flat.view(N, H, W, C).permute(0, 3, 1, 2)
        assert t.shape == shape and t.is_contiguous(memory_format=torch.channels_last)
        return t
    return flat.view(shape)


def test_kernel_adds_exactly_the_tensor_elements_bit_for_bit(dev):
    from monosowa_amd import pointwise
    layout, length = _kernel_layout()
    rng = np.random.default_rng(17)
    acc_h = np.full(length, SENTINEL, dtype=np.float32)
    g_h = np.full(length, -SENTINEL, dtype=np.float32)
    inside = np.zeros(length, dtype=bool)
    for i, (shape, a0, g0, _) in enumerate(layout):
        n = int(np.prod(shape))
        a, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        if n >= 2 * len(SPECIAL):                          # head and tail of the tensor: float4 body and scalar tail both see them
            a[:len(SPECIAL)], g[:len(SPECIAL)] = zip(*SPECIAL)
            a[-len(SPECIAL):], g[-len(SPECIAL):] = zip(*SPECIAL)
        else:
            a[0], g[0] = SPECIAL[i % len(SPECIAL)]
        assert not inside[a0:a0 + n].any()
        acc_h[a0:a0 + n], g_h[g0:g0 + n] = a, g
        inside[a0:a0 + n] = True
    assert not inside[0] and not inside[-1] and all(not inside[a0 - 1] and not inside[a0 + int(np.prod(s))] for s, a0, _, _ in layout)
    acc, g = torch.from_numpy(acc_h).to(dev), torch.from_numpy(g_h).to(dev)
    assert acc.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    accs = [_view(acc, a0, shape, cl) for shape, a0, _, cl in layout]
    grads = [_view(g, g0, shape, cl) for shape, _, g0, cl in layout]
    assert {(a.data_ptr() % 16, b.data_ptr() % 16) for a, b in zip(accs[9:12], grads[9:12])} == {(4, 4), (4, 0), (0, 4)}
    assert len({a.data_ptr() % 16 for a in accs[13:]}) == 4
    assert pointwise.accumulate_supported(accs, grads)
    want = acc.clone()
    for (shape, a0, g0, cl) in layout:
        n = int(np.prod(shape))
        want[a0:a0 + n] = acc[a0:a0 + n] + g[g0:g0 + n]                       # torch's add of the same storage-order elements
    plan = pointwise.GradAccumulatePlan(accs)
    assert plan.n_chunks == sum(-(-a.numel() // CHUNK) for a in accs)
    plan.add(accs, grads)
    torch.cuda.synchronize()
    got_h, want_h = acc.cpu().numpy(), want.cpu().numpy()
    nan = np.isnan(want_h)
    assert nan.sum() >= 3 * 9 and np.array_equal(np.isnan(got_h), nan)
    assert np.array_equal(got_h.view(np.int32)[~nan], want_h.view(np.int32)[~nan])
    assert np.isinf(want_h).any() and (np.abs(want_h[~nan]) < 1e-38).any()
    assert np.array_equal(got_h.view(np.int32)[~inside], acc_h.view(np.int32)[~inside])          # every sentinel unchanged
    assert np.array_equal(g.cpu().numpy().view(np.int32), g_h.view(np.int32))                    # the gradients are read only


# --------------------------------------------------------------------------------------------------------------- the shipped model
class _Loader:
    def __init__(self, seeds, batch_size=2):
        from monosowa_amd.synthetic import make_batch
        self.batch_size = batch_size
        self.batches = [make_batch(batch_size, "cpu", seed=s, resolution=RES) for s in seeds]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)

    def counts(self):
        return [int(b[2]["mask_2d"].sum()) for b in self.batches]


class _Rig:
    """A Trainer over a fresh copy of the module's model: its own optimizer, loader and seeding hook."""

    def __init__(self, shared, seeds, optimizer=None, **trainer_cfg):
        from monosowa_amd import flash_attn, pointwise
        from monosowa_amd.helpers.optimizer_helper import build_optimizer
        from monosowa_amd.helpers.trainer_helper import Trainer
        cfg, model0, self.crit = shared
        self.model = copy.deepcopy(model0)
        self.k = 0

        def hook(module, args):
            torch.manual_seed(100 + self.k)
            pointwise._seed_counter[0] = flash_attn._seed_counter[0] = 0
            self.k += 1
        self.model.register_forward_pre_hook(hook)
        self.opt = build_optimizer(dict(cfg["optimizer"], **(optimizer or {})), self.model)
        self.loader = _Loader(seeds)
        self.trainer = Trainer(dict({"save_path": "outputs", "max_epoch": 1}, **trainer_cfg), self.model, self.opt, self.loader, None, None,
                               None, logging.getLogger("test_accumulation"), self.crit, "shipped")
        self.trainer.log_interval = 10 ** 9
        self.model.train(), self.crit.train()

    def grads(self):
        return {n: p.grad.detach().clone() for n, p in self.model.named_parameters() if p.grad is not None}

    def plain(self, i, num_boxes=None):
        """Gradients of loader batch i evaluated alone as micro-step i, the way ``train_step`` does up to the optimizer step."""
        from monosowa_amd.helpers.trainer_helper import stage_batch
        from monosowa_amd.monodetr.criterion import weighted_total
        t = self.trainer
        inputs, calibs, targets, info = stage_batch(self.loader.batches[i], t.device)
        tl = t.prepare_targets(targets, inputs.shape[0])
        self.opt.zero_grad(set_to_none=True)
        self.k = i
        outputs = t.model(inputs, calibs, tl, targets["img_size"], dn_args=None)
        weighted_total(t.detr_loss(outputs, tl, None, info, num_boxes=num_boxes), t.detr_loss.weight_dict).backward()
        return self.grads()

    def cycle(self, step=False):
        """One cycle over the loader's batches; ``step=False`` stops in front of ``optimizer.step()``."""
        if not step:
            self.opt.step = lambda *a, **k: None
        try:
            self.k = 0
            self.trainer.train_cycle(list(self.loader))
        finally:
            self.opt.__dict__.pop("step", None)
        return self.grads()

    def state(self):
        out = {}
        for n, p in self.model.named_parameters():
            out["param." + n] = p.detach().clone()
            for key in ("exp_avg", "exp_avg_sq"):
                if key in self.opt.state.get(p, {}):
                    out[key + "." + n] = self.opt.state[p][key].clone()
        return out


@pytest.fixture(scope="module")
def shared(dev):
    from monosowa_amd.helpers.model_helper import build_model
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    torch.manual_seed(444)
    model, crit = build_model(dict(cfg["model"], device="cuda", dropout=0.0, depth_map_size=(RES[0] // 16, RES[1] // 16)))
    return cfg, model.to(dev), crit.to(dev)


@pytest.fixture()
def kernel_calls(monkeypatch):
    """Counts the launches of the accumulation kernel."""
    from monosowa_amd import pointwise
    calls = []
    add = pointwise.GradAccumulatePlan.add
    monkeypatch.setattr(pointwise.GradAccumulatePlan, "add", lambda self, accs, grads, **kw: (calls.append(len(accs)), add(self, accs, grads, **kw))[1])
    return calls


# --------------------------------------------------------------------------------------------------------------- 6. linearity
def test_cycle_is_the_rounded_mean_of_the_micro_gradients_under_the_deterministic_flag(shared, kernel_calls, monkeypatch):
    """|A - (g0 + g1) / 2| <= 2 * 2^-24 * (|g0| + |g1|) / 2 per element: halving is exact, so A is ONE correctly rounded add of the two
    halves -- error at most 2^-24 |g0 / 2 + g1 / 2|; the factor 2 is margin.  Equal box totals, so each micro-batch's own normaliser
    (the untouched path) is the cycle's."""
    from monosowa_amd import pointwise
    with _mode(True):
        rig = _Rig(shared, [3, 7], global_batch=4)
        assert rig.loader.counts() == [12, 12] and rig.trainer.accum_steps == 2
        g0, g1 = rig.plain(0), rig.plain(1)
        assert not kernel_calls
        A = rig.cycle()
        assert len(kernel_calls) == 1 and kernel_calls[0] == len(A) > 300           # one launch for every gradient tensor
        again = rig.cycle()
        monkeypatch.setattr(pointwise, "FUSED_ACCUMULATE", False)
        autograd = rig.cycle()
        assert len(kernel_calls) == 2
    assert set(A) == set(g0) == set(g1) == set(again) == set(autograd)
    worst = 0.0
    for n in sorted(A):
        a, x, y = A[n].double(), g0[n].double(), g1[n].double()
        err, bound = (a - (x + y) / 2).abs(), 2.0 * 2.0 ** -24 * (x.abs() + y.abs()) / 2
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (n, ratio)
        assert torch.equal(A[n], again[n]), "%s differs between two evaluations of the cycle" % n
        assert torch.equal(A[n], autograd[n]), "%s differs between the kernel and autograd's accumulation" % n
    print("\nworst |A - mean| / bound over %d tensors: %.3f" % (len(A), worst))


# --------------------------------------------------------------------------------------------------------------- 7. unequal counts
def _bound(name):
    return BOUND_BACKBONE if name.startswith("backbone.") else _group(name)[1]


def _rel_errors(A, ref):
    """per tensor ||A - ref|| / ||ref||; the key projections' biases (zero gradient in exact arithmetic) against their weight's norm,
    as tests/test_train_step_grads_gpu.py measures them"""
    def scale(n):
        return ref[n.replace("_proj.bias", "_proj.weight")] if n.endswith(("sa_kcontent_proj.bias", "sa_kpos_proj.bias")) else ref[n]
    return {n: float((A[n].double() - ref[n]).norm() / scale(n).norm().clamp_min(1e-300)) for n in A}


def test_cycle_normalises_by_the_cycle_wide_box_count_not_by_each_micro_batchs_own(shared):
    """The class head gets seeded weights of standard deviation 0.25 first (logits spread by 0.25 * sqrt(256) = 4 around the prior's
    -4.6, as a trained head's are).  At initialisation every query sits at the prior probability 0.01: the unmatched queries' focal
    gradient vanishes (~ p^2) and every matched box contributes the same constant, so a class bias's gradient is
    (boxes x constant) / num_boxes -- the SAME number under both definitions, whatever the counts (measured: 2 of the 3 class biases
    within 6e-3).  With spread logits the unmatched queries dominate that gradient; their number does not depend on the box count,
    so the two normalisers (22 | 198 against 110) scale it by 2.8."""
    rig = _Rig(shared, [17, 13], global_batch=4)
    assert rig.loader.counts() == [2, 18]
    gen = torch.Generator().manual_seed(29)
    with torch.no_grad():
        spread = [p for n, p in rig.model.named_parameters() if "class_embed." in n and n.endswith(".weight")]
        assert len(spread) == 3 and all(p.shape[1] == 256 for p in spread)
        for p in spread:
            p.copy_((0.25 * torch.randn(p.shape, generator=gen)).to(p.device))
    n_bar = 20 * rig.crit.group_num / 2.0
    mean = lambda x, y: {n: (x[n].double() + y[n].double()) / 2 for n in x}
    ref = mean(rig.plain(0, num_boxes=n_bar), rig.plain(1, num_boxes=n_bar))
    own = mean(rig.plain(0), rig.plain(1))
    A = rig.cycle()
    assert set(A) == set(ref) == set(own)
    e_ref, e_own = _rel_errors(A, ref), _rel_errors(A, own)
    for title, errs in (("cycle-wide normaliser", e_ref), ("own normaliser", e_own)):
        print("\n%s" % title)
        for name, e in sorted(errs.items(), key=lambda kv: -kv[1] / _bound(kv[0]))[:6]:
            print("  %.3e (bound %.1e)  %s" % (e, _bound(name), name))
    bad = [(n, e, _bound(n)) for n, e in e_ref.items() if e > _bound(n)]
    assert not bad, bad[:12]
    heads = [n for n in A if "class_embed." in n or "bbox_embed." in n]
    assert len(heads) >= 6
    told_apart = [n for n in heads if e_own[n] > BOUND_HEADS]
    assert told_apart == heads, sorted(set(heads) - set(told_apart))


# --------------------------------------------------------------------------------------------------------------- 8. guard
def test_guard_sees_the_accumulated_gradient_and_skips_the_whole_cycle(shared):
    rig = _Rig(shared, [3, 7], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, global_batch=4)
    A = rig.cycle(step=True)
    report = rig.opt.guard_report()
    assert rig.opt._guard is not None and rig.opt._guard_host is None, "the device path must have served the step"
    want = float(torch.stack([(g.double() ** 2).sum() for g in A.values()]).sum().sqrt())
    print("\ngrad_norm %r, float64 of the accumulated gradient %r" % (report["grad_norm"], want))
    assert abs(report["grad_norm"] - want) <= float(np.spacing(np.float32(want)))        # tests/test_guarded_step_gpu.py: one ulp of f32
    assert report["skipped_total"] == 0 and report["coef"] < 1.0
    # a NaN in the LAST micro-batch's image (a NaN cost would be reported by the matcher when the next matching begins)
    before = rig.state()
    assert any(k.startswith("exp_avg_sq.") for k in before)
    rig.loader.batches[1][0][1, 0, 5, 7] = float("nan")
    rig.cycle(step=True)
    assert rig.opt.guard_report()["skipped_total"] == 1
    after = rig.state()
    assert set(after) == set(before) and all(torch.equal(before[k], after[k]) for k in before)
    try:                                   # whatever the shared matcher noted about that micro-batch's costs is taken down here
        rig.crit.matcher.check_device_status(block=True)
    except ValueError:
        pass


# --------------------------------------------------------------------------------------------------------------- 9. no new sync
def test_cycle_does_not_synchronise(shared, kernel_calls):
    rig = _Rig(shared, [3, 7], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, global_batch=4)
    rig.cycle(step=True)                                   # plans, pinned tables and kernel selection belong to the first cycle
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rig.cycle(step=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()] == []
    assert len(kernel_calls) == 2
    assert rig.opt.guard_report()["skipped_total"] == 0


# --------------------------------------------------------------------------------------------------------------- 10. key off
def test_global_batch_of_one_loader_batch_leaves_the_training_bit_identical(shared, kernel_calls):
    with _mode(True):
        states = []
        for cfg in ({}, {"global_batch": 2}):
            rig = _Rig(shared, [3, 7], **cfg)
            assert rig.trainer.accum_steps == 1
            rig.trainer.train_one_epoch(0)
            assert rig.k == 2
            states.append(rig.state())
    assert not kernel_calls
    assert set(states[0]) == set(states[1]) and len(states[0]) > 900
    assert all(torch.equal(states[0][k], states[1][k]) for k in states[0])
    start = dict(shared[1].named_parameters())
    assert any(not torch.equal(states[0]["param." + n], p) for n, p in start.items())      # ... and it did train


# --------------------------------------------------------------------------------------------------------------- fallback inside a cycle
def test_accumulator_goes_over_to_autograd_when_a_later_gradient_is_not_served(dev, kernel_calls):
    """A fresh gradient in another layout than its accumulator at micro-step 1: no exception, the sums are torch's, the accumulators
    are back in ``.grad`` (where autograd adds in place) and the kernel is not launched."""
    from monosowa_amd import pointwise
    gen = torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    ps = [torch.nn.Parameter(torch.zeros(5, 3, device=dev)), torch.nn.Parameter(torch.zeros(7, device=dev)),
          torch.nn.Parameter(torch.zeros(4, device=dev))]
    a0, b0, a1, b1, c1, a2 = rand(5, 3), rand(7), rand(3, 5).t(), rand(7), rand(4), rand(5, 3)
    assert a1.shape == (5, 3) and not a1.is_contiguous()
    acc = pointwise.GradAccumulator(ps)
    acc.begin()
    ps[0].grad, ps[1].grad = a0.clone(), b0.clone()
    acc.collect(0)
    assert acc.acc is not None and all(p.grad is None for p in ps)
    ps[0].grad, ps[1].grad, ps[2].grad = a1, b1.clone(), c1.clone()
    acc.collect(1)
    assert acc.acc is None and not kernel_calls
    assert torch.equal(ps[0].grad, a0 + a1) and torch.equal(ps[1].grad, b0 + b1) and torch.equal(ps[2].grad, c1)
    ps[0].grad.add_(a2)                                    # what autograd's AccumulateGrad does from here on
    acc.collect(2)
    acc.install()
    assert torch.equal(ps[0].grad, (a0 + a1) + a2) and torch.equal(ps[1].grad, b0 + b1)
