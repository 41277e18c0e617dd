"""The guarded AdamW step on the device (``mono_grad_guard_f32`` + ``mono_adamw_step_guarded_f32``): global gradient norm against
float64, ``clip_grad_norm_``'s coefficient, the update bit for bit the plain kernel's on pre-scaled gradients, the skipping of a
non-finite step, no host synchronisation, and bit-identical records from run to run.

The tensor set is the smallest that reaches every branch of the kernels: sizes 1, 3, 5, 32768 (exactly one chunk), 32769 and
65536 + 7, a channels-last convolution weight, a parameter / gradient pair one float off a 16-byte boundary (scalar path), two
parameter groups with different weight decay, and enough 1..7-element tensors that the number of chunks is at least the shipped
model's -- so the one-workgroup fold runs many times past the 256 partials it takes at once."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 32768
LR, WD = 1e-3, 1e-4
BIG = 65536 + 7           # its last chunk has 7 elements: one float4 and a 3-element tail
# (name, kind, shape): group 0 (no decay) gets the first four and half of the small tensors, group 1 the rest; BIG comes last
HEAD = [("one", "plain", (1,)), ("three", "plain", (3,)), ("five", "plain", (5,)), ("offset", "off", (1031,))]
TAIL = [("chunk", "plain", (CHUNK,)), ("chunk+1", "plain", (CHUNK + 1,)), ("conv", "cl", (8, 4, 3, 3)), ("big", "plain", (BIG,))]


@pytest.fixture(scope="module")
def model_chunks():
    """Chunks the shipped model's parameters take in the AdamW tables: sum of ceil(numel / 32768), from the shapes, on the CPU."""
    import yaml
    from monosowa_amd.helpers.model_helper import build_model
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, _ = build_model(dict(cfg["model"], device="cpu"))
    return sum(-(-p.numel() // CHUNK) for p in model.parameters() if p.requires_grad)


@pytest.fixture(scope="module")
def layout(model_chunks):
    """[(name, kind, shape)] per group; the small tensors alone already make as many chunks as the model has."""
    n_small = max(2000, model_chunks)
    sizes = np.random.default_rng(5).integers(1, 8, n_small)
    small = [("s%d" % i, "small", (int(n),)) for i, n in enumerate(sizes)]
    half = n_small // 2
    return [HEAD + small[:half], small[half:] + TAIL]


def _values(layout, seed, scale=None):
    """Seeded float32 arrays for every tensor of the layout; ``scale``: every element about that size (random sign, 1 - 1.5 x)."""
    rng = np.random.default_rng(seed)
    out = []
    for group in layout:
        vals = []
        for _, _, shape in group:
            if scale is None:
                vals.append(rng.standard_normal(shape).astype(np.float32))
            else:
                vals.append((rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 1.5, shape) * scale).astype(np.float32))
        out.append(vals)
    return out


def _place(layout, values, dev):
    """The arrays as device tensors in the layout's kinds (a list per group)."""
    out = []
    for group, vals in zip(layout, values):
        small = [v for (_, kind, _), v in zip(group, vals) if kind == "small"]
        flat = torch.from_numpy(np.concatenate(small)).to(dev)
        parts = iter([t.clone() for t in flat.split([v.size for v in small])])       # one upload, own (aligned) allocations
        ts = []
        for (_, kind, _), v in zip(group, vals):
            if kind == "small":
                t = next(parts)
            elif kind == "cl":
                t = torch.from_numpy(v).to(dev).contiguous(memory_format=torch.channels_last)
            elif kind == "off":
                base = torch.zeros(v.size + 8, dtype=torch.float32, device=dev)
                t = base[1:1 + v.size]
                t.copy_(torch.from_numpy(v))
                assert t.data_ptr() % 16 == 4
            else:
                t = torch.from_numpy(v).to(dev)
            ts.append(t)
        out.append(ts)
    return out


class Rig:
    """The tensor set as parameters of one AdamW (same seeded start values for every rig of a layout)."""

    def __init__(self, layout, dev, **guard):
        from monosowa_amd.helpers.optimizer_helper import AdamW
        self.layout, self.dev = layout, dev
        placed = _place(layout, _values(layout, 11), dev)
        self.groups = [[torch.nn.Parameter(t) for t in ts] for ts in placed]
        self.params = [p for g in self.groups for p in g]
        self.opt = AdamW([{"params": self.groups[0], "weight_decay": 0}, {"params": self.groups[1], "weight_decay": WD}], lr=LR, **guard)

    def set_grads(self, values, times=None):
        """``times``: a float32 factor put on every gradient by a torch multiply (what the guarded kernel does inside)."""
        for p, g in zip(self.params, (t for ts in _place(self.layout, values, self.dev) for t in ts)):
            p.grad = g if times is None else g * times

    def state(self):
        return [(p.detach().clone(), self.opt.state[p]["exp_avg"].clone(), self.opt.state[p]["exp_avg_sq"].clone()) for p in self.params]

    def report(self):
        assert self.opt._guard is not None and self.opt._guard_host is None, "the device path must have served the step"
        return self.opt.guard_report()

    def chunks(self):
        return sum(plan.n_chunks for plan in self.opt._fused_plans.values())


def _assert_same_state(a, b):
    sa, sb = a.state(), b.state()
    for i, (x, y) in enumerate(zip(sa, sb)):
        for name, u, v in zip(("p", "exp_avg", "exp_avg_sq"), x, y):
            assert torch.equal(u, v), (a.params[i].shape, name)


def _norm_f64(values):
    """The L2 norm in float64 from a correctly rounded sum of the exact squares."""
    sq = np.concatenate([v.astype(np.float64).ravel() for vals in values for v in vals]) ** 2
    return math.sqrt(math.fsum(sq))


def _coef_f32(norm, max_norm):
    return np.minimum(np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)), np.float32(1.0))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_set_has_at_least_the_models_chunks(layout, model_chunks, dev):
    rig = Rig(layout, dev, clip_max_norm=0.1, skip_nonfinite=True)
    rig.set_grads(_values(layout, 21))
    rig.opt.step()
    assert model_chunks > 256                          # the fold's width: the model itself needs several rounds
    assert rig.chunks() >= model_chunks
    assert rig.chunks() == sum(-(-int(np.prod(s)) // CHUNK) for g in layout for _, _, s in g)
    assert rig.report()["skipped_total"] == 0


# |reported - true| <= 1 ulp of float32, derived: the squares are exact in f64; a sum of at most 4e7 non-negative terms in any order
# is off by at most 4e7 * 2^-53 = 4.4e-9 relative, its square root by half of that plus 2^-53 -- 1/27 of the 6e-8 half-ulp of f32 --
# so the one rounding to float32 lands on one of the two float32 neighbours of the true norm.
@pytest.mark.parametrize("scale", [None, 1e25, 1e-30])
def test_norm_within_one_ulp_of_float64(layout, dev, scale):
    values = _values(layout, 31, scale)
    want = _norm_f64(values)
    assert float(np.finfo(np.float32).tiny) < want < float(np.finfo(np.float32).max)       # the true norm is a normal float32
    if scale is not None:                              # ... where a float32 sum of squares gives Inf / 0
        with np.errstate(over="ignore", under="ignore"):
            naive = np.float32(sum(np.sum(v * v, dtype=np.float32) for vals in values for v in vals))
        assert naive == (np.inf if scale > 1 else 0.0)
    rig = Rig(layout, dev, clip_max_norm=0.1, skip_nonfinite=True)
    rig.set_grads(values)
    rig.opt.step()
    rep = rig.report()
    got = np.float32(rep["grad_norm"])
    print("scale %s: norm %r, float64 %r, ulp %r" % (scale, got, want, np.spacing(np.float32(want))))
    assert abs(float(got) - want) <= float(np.spacing(np.float32(want)))
    assert rep["skipped_total"] == 0
    assert np.float32(rep["coef"]) == _coef_f32(got, 0.1)


@pytest.mark.parametrize("max_norm", [0.1, 1e6])
def test_coefficient_is_the_f32_formula_of_the_reported_norm(layout, dev, max_norm):
    values = _values(layout, 41)
    rig = Rig(layout, dev, clip_max_norm=max_norm, skip_nonfinite=False)
    rig.set_grads(values)
    rig.opt.step()
    first = rig.report()
    assert np.float32(first["coef"]) == _coef_f32(first["grad_norm"], max_norm)
    assert (first["coef"] == 1.0) == (max_norm == 1e6) and (first["grad_norm"] < max_norm) == (max_norm == 1e6)
    rig.set_grads([[np.zeros_like(v) for v in vals] for vals in values])
    rig.opt.step()
    zero = rig.report()
    assert zero["grad_norm"] == 0.0 and zero["coef"] == 1.0
    off = Rig(layout, dev, skip_nonfinite=True)        # no clipping: the same norm, and the coefficient is 1 whatever it is
    off.set_grads(values)
    off.opt.step()
    assert off.report()["coef"] == 1.0 and off.report()["grad_norm"] == first["grad_norm"]


@pytest.mark.parametrize("max_norm", [0.1, 1e6])
def test_update_is_the_plain_kernel_on_prescaled_gradients(layout, dev, max_norm):
    guarded, plain = Rig(layout, dev, clip_max_norm=max_norm, skip_nonfinite=True), Rig(layout, dev)
    for step in range(3):                               # the moments are zero in the first step only
        values = _values(layout, 50 + step)
        guarded.set_grads(values)
        kept = [p.grad.clone() for p in guarded.params]
        guarded.opt.step()
        coef = guarded.report()["coef"]                 # ONE coefficient for both groups
        assert (coef == 1.0) == (max_norm == 1e6)
        plain.set_grads(values, times=None if coef == 1.0 else coef)
        plain.opt.step()
        assert plain.opt._guard is None and len(plain.opt._fused_plans) == 2       # mono_adamw_step_f32, a launch per group
        _assert_same_state(guarded, plain)
        assert all(torch.equal(p.grad, g) for p, g in zip(guarded.params, kept))   # p.grad is not rewritten
    assert guarded.report()["skipped_total"] == 0


def _poison(values, layout, where):
    """A non-finite value where the reduction could lose it: (group, tensor, flat index, value)."""
    g1 = len(layout[1]) - 1
    assert layout[1][g1][0] == "big" and layout[0][0][0] == "one"
    gi, ti, idx, val = {"nan_last_tail": (1, g1, BIG - 1, np.nan),          # last element of the 3-element tail of the LAST chunk
                        "inf_middle_chunk": (1, g1, CHUNK + CHUNK // 2, np.inf),      # the middle one of the big tensor's three chunks
                        "neg_inf_single": (0, 0, 0, -np.inf)}[where]
    values[gi][ti].reshape(-1)[idx] = val
    return values


@pytest.mark.parametrize("where", ["nan_last_tail", "inf_middle_chunk", "neg_inf_single"])
def test_non_finite_step_is_skipped_whole(layout, dev, where):
    guarded, plain = Rig(layout, dev, clip_max_norm=0.1, skip_nonfinite=True), Rig(layout, dev)

    def finite_step(seed):
        values = _values(layout, seed)
        guarded.set_grads(values)
        guarded.opt.step()
        plain.set_grads(values, times=guarded.report()["coef"])
        plain.opt.step()
        _assert_same_state(guarded, plain)

    finite_step(60)
    before, count = guarded.state(), guarded.report()["skipped_total"]
    guarded.set_grads(_poison(_values(layout, 61), layout, where))
    guarded.opt.step()
    assert guarded.report()["skipped_total"] == count + 1
    for i, (x, y) in enumerate(zip(before, guarded.state())):
        assert all(torch.equal(u, v) for u, v in zip(x, y)), guarded.params[i].shape
    for p in plain.params:                              # the guarded optimizer counted the step (the host does not know of the skip)
        plain.opt.state[p]["step"] += 1
    finite_step(62)                                     # and the next step is a regular one
    assert guarded.report()["skipped_total"] == count + 1


def test_guarded_step_does_not_synchronise(layout, dev):
    rig = Rig(layout, dev, clip_max_norm=0.1, skip_nonfinite=True)
    for i in range(4):
        rig.set_grads(_values(layout, 70 + i))
        if i < 3:
            rig.opt.step()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rig.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert [str(w.message) for w in caught] == []
    assert rig.report()["skipped_total"] == 0


def test_record_is_bit_identical_from_run_to_run(layout, dev):
    records = []
    for _ in range(2):
        rig = Rig(layout, dev, clip_max_norm=0.1, skip_nonfinite=True)
        rig.set_grads(_values(layout, 31))
        rig.opt.step()
        rig.report()
        records.append(rig.opt._guard.record.cpu())
    assert torch.equal(records[0], records[1])
