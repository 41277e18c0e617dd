"""``trainer.history`` on the GPU: ``mono_step_stats_f32`` alone (the layout of tests/test_accumulation_gpu.py over two AdamW chunk tables
and five interleaved module groups plus an empty sixth), under a guard record, and train steps of the shipped architecture (dropout 0,
640 x 192, batch 2, the rig of tests/test_accumulation_gpu.py) with the key on and off.

The reference sums are taken in numpy's extended precision (64-bit mantissa: their own error is far below 2^-53) and rounded to
float64 once.  Tolerance: a sum of n non-negative doubles added in any order -- every addition rounded once, 2^-53 relative, all terms of
one sign -- lies within n * 2^-53 of the exact sum, relative; the products of float32 values are exact in float64.  n is the group's
element count.  A norm is the square root of such a sum: half its relative error plus the two roundings of the roots, n * 2^-53 again
for n >= 2, and exact for n = 1."""
import json
import logging
import math
import os
import warnings

import numpy as np
import pytest
import torch

from test_accumulation_gpu import CHUNK, RES, _Rig, _kernel_layout, _view, dev, shared      # noqa: F401  (fixtures)
from test_ema_cpu import CHECKPOINT_KEYS
from test_ema_gpu import _steps
from test_train_step_grads_gpu import _mode

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
N_GROUPS = 6                       # five interleaved groups (tensor i belongs to group i % 5) and a sixth without chunks
P_SENTINEL, G_SENTINEL, D_SENTINEL = 12345.0, -12345.0, 777.0
PAD = 5                            # sentinel doubles on either side of partials and of the output row


def _sumsq(x):
    """Sum of squares of a float32 array: extended precision, rounded to float64 once."""
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(np.square(x.astype(np.longdouble))))


# --------------------------------------------------------------------------------------------------------------- the kernel alone
class _Case:
    """Parameters and gradients laid out in two buffers with sentinels in between (``_kernel_layout``), the tensors dealt alternately to
    two ``FusedAdamWPlan`` tables, the group id of every chunk on the device, and sentinel-framed partials and output rows."""

    def __init__(self, dev, scale=1.0, poison=()):
        from monosowa_amd.pointwise import FusedAdamWPlan
        layout, length = _kernel_layout()
        self.sizes = [int(np.prod(s)) for s, _, _, _ in layout]
        assert self.sizes[:9] == [1, 3, 4, 5, 255, 32767, 32768, 32769, 65537] and len(layout) == 613
        rng = np.random.default_rng(53)
        self.p_h = np.full(length, P_SENTINEL, dtype=np.float32)
        self.g_h = np.full(length, G_SENTINEL, dtype=np.float32)
        self.p_np, self.g_np = [], []
        for i, ((shape, p0, g0, _), n) in enumerate(zip(layout, self.sizes)):
            p = rng.standard_normal(n).astype(np.float32)
            g = (rng.standard_normal(n) * scale).astype(np.float32)
            for tensor, index, value in poison:
                if tensor == i:
                    g[index] = value
            assert np.isfinite(g).all() or poison
            self.p_h[p0:p0 + n], self.g_h[g0:g0 + n] = p, g
            self.p_np.append(p), self.g_np.append(g)
        self.pbuf, self.gbuf = torch.from_numpy(self.p_h).to(dev), torch.from_numpy(self.g_h).to(dev)
        zeros = torch.zeros(length, dtype=torch.float32, device=dev)                     # the moments: never read by this kernel
        assert self.pbuf.data_ptr() % 16 == 0 and self.gbuf.data_ptr() % 16 == 0 and zeros.data_ptr() % 16 == 0
        params = [_view(self.pbuf, p0, shape, cl) for shape, p0, _, cl in layout]
        grads = [_view(self.gbuf, g0, shape, cl) for shape, _, g0, cl in layout]
        moments = [_view(zeros, p0, shape, cl) for shape, p0, _, cl in layout]
        assert {(a.data_ptr() % 16, b.data_ptr() % 16) for a, b in zip(params[9:12], grads[9:12])} == {(4, 4), (4, 0), (0, 4)}
        assert params[12].is_contiguous(memory_format=torch.channels_last) and len({a.data_ptr() % 16 for a in params[13:]}) == 4
        # every access of the kernel lies inside the two buffers: the tables' counts are the tensors' sizes
        for a, b in zip(params, grads):
            assert self.pbuf.data_ptr() <= a.data_ptr() and a.data_ptr() + 4 * a.numel() <= self.pbuf.data_ptr() + 4 * length
            assert self.gbuf.data_ptr() <= b.data_ptr() and b.data_ptr() + 4 * b.numel() <= self.gbuf.data_ptr() + 4 * length
        self.keep = (params, grads, moments, zeros)
        self.group_of = [i % 5 for i in range(len(layout))]
        self.plans, self.arrays = [], []
        for half in (0, 1):
            ids = list(range(half, len(layout), 2))
            plan = FusedAdamWPlan([params[i] for i in ids], [moments[i] for i in ids], [moments[i] for i in ids], 0.0)
            plan.refresh([grads[i] for i in ids])
            assert plan.n_chunks == sum(-(-self.sizes[i] // CHUNK) for i in ids)
            self.plans.append(plan)
            self.arrays.append(torch.from_numpy(np.array([self.group_of[i] for i in ids], dtype=np.int32)[plan.tensor]).to(dev))
        self.total = sum(p.n_chunks for p in self.plans)
        assert self.total == 613 + 1 + 2                                                 # 32769 -> 2 chunks, 65537 -> 3
        self.width = 3 * N_GROUPS + 3
        self.partials = torch.full((3 * self.total + 2 * PAD,), D_SENTINEL, dtype=torch.float64, device=dev)
        self.rows = torch.full((3, self.width + 2 * PAD), D_SENTINEL, dtype=torch.float64, device=dev)      # three "ring rows"
        self.dev = dev

    def run(self, row=0, record=None):
        from monosowa_amd.pointwise import step_stats
        step_stats(self.plans, self.arrays, N_GROUPS, record, self.partials[PAD:], self.rows[row, PAD:].data_ptr())

    def result(self, row=0):
        torch.cuda.synchronize()
        return self.rows[row].cpu().numpy()[PAD:PAD + self.width]

    def reference(self):
        """[(grad_sumsq, param_sumsq, grad_nonfinite, elements)] per group."""
        out = []
        for q in range(N_GROUPS):
            ids = [i for i, g in enumerate(self.group_of) if g == q]
            g = np.concatenate([self.g_np[i] for i in ids]) if ids else np.zeros(0, dtype=np.float32)
            p = np.concatenate([self.p_np[i] for i in ids]) if ids else np.zeros(0, dtype=np.float32)
            out.append((_sumsq(g), _sumsq(p), int((~np.isfinite(g)).sum()), g.size))
        return out

    def assert_frames_and_inputs_untouched(self, rows_written, guard_columns):
        torch.cuda.synchronize()
        rows, partials = self.rows.cpu().numpy(), self.partials.cpu().numpy()
        assert (partials[:PAD] == D_SENTINEL).all() and (partials[-PAD:] == D_SENTINEL).all()
        assert not (partials[PAD:-PAD] == D_SENTINEL).any()
        for r in range(rows.shape[0]):
            written = self.width if guard_columns else self.width - 3
            assert (rows[r, :PAD] == D_SENTINEL).all() and (rows[r, PAD + (written if r in rows_written else 0):] == D_SENTINEL).all(), r
        assert np.array_equal(self.pbuf.cpu().numpy().view(np.int32), self.p_h.view(np.int32))          # both inputs keep their bits
        assert np.array_equal(self.gbuf.cpu().numpy().view(np.int32), self.g_h.view(np.int32))


def _assert_sums(got, want, what):
    """``got``: the 3 * N_GROUPS doubles of a row; ``want``: ``_Case.reference()``."""
    worst = 0.0
    for q, (gs, ps, bad, n) in enumerate(want):
        ggs, gps, gbad = got[3 * q:3 * q + 3]
        assert gbad == bad, (what, q, gbad, bad)
        assert abs(gps - ps) <= n * U * ps, (what, "param_sumsq", q, gps, ps)
        if math.isnan(gs):
            assert math.isnan(ggs), (what, q, ggs)
        elif math.isinf(gs):
            assert ggs == gs, (what, q, ggs)
        else:
            assert math.isfinite(ggs) and abs(ggs - gs) <= n * U * gs, (what, "grad_sumsq", q, ggs, gs)
            worst = max(worst, abs(ggs - gs) / (n * U * gs) if n else 0.0)
        worst = max(worst, abs(gps - ps) / (n * U * ps) if n else 0.0)
    print("\n%s: worst |sum - reference| / (n * 2^-53 * reference) = %.4f" % (what, worst))


def test_kernel_sums_per_group_within_the_float64_bound_and_writes_nothing_else(dev):
    case = _Case(dev)
    want = case.reference()
    assert [w[3] for w in want][:5] == [sum(n for i, n in enumerate(case.sizes) if i % 5 == q) for q in range(5)] and want[5][3] == 0
    case.run(row=1)
    got = case.result(row=1)
    _assert_sums(got, want, "randn")
    assert got[15] == 0.0 and got[16] == 0.0 and got[17] == 0.0 and not np.signbit(got[15:18]).any()      # the empty group: exactly 0
    assert all(w[2] == 0 for w in want)
    case.assert_frames_and_inputs_untouched(rows_written={1}, guard_columns=False)
    # the same inputs at another ring row: identical bits
    case.run(row=2)
    again = case.result(row=2)
    assert np.array_equal(got[:18].view(np.int64), again[:18].view(np.int64))
    case.assert_frames_and_inputs_untouched(rows_written={1, 2}, guard_columns=False)


@pytest.mark.parametrize("scale", [1e25, 1e-30])
def test_kernel_neither_overflows_nor_loses_scaled_gradients(dev, scale):
    case = _Case(dev, scale=scale)
    want = case.reference()
    assert all(math.isfinite(w[0]) and w[0] > 0 for w in want[:5])
    assert (want[0][0] > 1e50) if scale > 1 else (want[0][0] < 1e-50)      # beyond float32's range as a sum of squares
    case.run()
    _assert_sums(case.result(), want, "gradients x %g" % scale)


def test_kernel_counts_non_finite_gradients_in_their_groups_alone(dev):
    """NaN in the last tail element of the 32769-element tensor (group 2), +Inf in the middle chunk of the 65537-element one (group 3),
    -Inf as the one-element tensor (group 0)."""
    case = _Case(dev, poison=((7, 32768, np.nan), (8, CHUNK + 100, np.inf), (0, 0, -np.inf)))
    want = case.reference()
    assert [w[2] for w in want] == [1, 0, 1, 1, 0, 0]
    assert want[0][0] == math.inf and math.isnan(want[2][0]) and want[3][0] == math.inf
    assert all(math.isfinite(want[q][0]) for q in (1, 4, 5)) and all(math.isfinite(w[1]) for w in want)
    case.run()
    _assert_sums(case.result(), want, "non-finite placements")
    case.assert_frames_and_inputs_untouched(rows_written={0}, guard_columns=False)


def test_kernel_copies_the_guard_record_and_agrees_with_its_norm(dev):
    from monosowa_amd.pointwise import GradGuard
    case = _Case(dev)
    guard = GradGuard(dev)
    guard.run(case.plans, 0.1, True)
    case.run(row=0, record=guard.record.data_ptr())
    got = case.result()
    report = guard.report()
    assert report["skip"] == 0 and report["coef"] < 1.0
    assert got[18] == float(np.float32(report["grad_norm"])) and got[19] == float(np.float32(report["coef"])) and got[20] == 0.0
    total = float(np.float32(math.sqrt(float(np.sum(got[0:18:3])))))
    assert abs(total - report["grad_norm"]) <= float(np.spacing(np.float32(report["grad_norm"])))       # one float32 ulp
    _assert_sums(got, case.reference(), "under a guard record")
    case.assert_frames_and_inputs_untouched(rows_written={0}, guard_columns=True)
    # a NaN gradient: skip = 1 is recorded
    bad = _Case(dev, poison=((7, 32768, np.nan),))
    guard.run(bad.plans, 0.1, True)
    bad.run(row=0, record=guard.record.data_ptr())
    got = bad.result()
    assert got[20] == 1.0 and math.isnan(got[18]) and guard.report()["skip"] == 1
    assert [got[3 * q + 2] for q in range(N_GROUPS)] == [0, 0, 1, 0, 0, 0]


def test_entry_point_with_zero_chunks_leaves_the_row_alone(dev):
    import ctypes
    from monosowa_amd import pointwise
    case = _Case(dev)
    tables = (ctypes.c_void_p * 2)(*[p.dev.data_ptr() for p in case.plans])
    groups = (ctypes.c_void_p * 2)(*[a.data_ptr() for a in case.arrays])
    zero, negative = (ctypes.c_int * 2)(0, 0), (ctypes.c_int * 2)(case.plans[0].n_chunks, -1)
    lib = pointwise.load()
    args = (None, case.partials[PAD:].data_ptr(), case.rows[0, PAD:].data_ptr(), None)
    assert lib.mono_step_stats_f32(tables, zero, groups, 2, N_GROUPS, *args) == 0
    assert lib.mono_step_stats_f32(tables, negative, groups, 2, N_GROUPS, *args) == -2
    assert lib.mono_step_stats_f32(tables, zero, groups, 9, N_GROUPS, *args) == -2
    assert lib.mono_step_stats_f32(tables, zero, groups, 2, 65, *args) == -2
    assert lib.mono_step_stats_f32(None, zero, groups, 2, N_GROUPS, *args) == -1
    assert lib.mono_step_stats_f32(tables, zero, groups, 2, N_GROUPS, None, None, case.rows.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (case.rows.cpu().numpy() == D_SENTINEL).all() and (case.partials.cpu().numpy() == D_SENTINEL).all()


# --------------------------------------------------------------------------------------------------------------- the shipped model
class _Terms:
    """Wraps the criterion's forward: the raw loss terms of every call as Python floats (``.item()``), in ``weight_dict`` order."""

    def __init__(self, crit):
        self.crit, self.calls = crit, []

    def __enter__(self):
        forward = self.crit.forward

        def spy(*a, **k):
            ld = forward(*a, **k)
            self.calls.append({key: ld.peek(key).item() for key in self.crit.weight_dict if key in ld})
            return ld
        self.crit.forward = spy
        return self

    def __exit__(self, *exc):
        self.crit.__dict__.pop("forward", None)


def _param_reference(rig, hist, snapshot):
    """{group: (sum p^2 over the parameters that had a gradient in the last step, their element count)} from a host snapshot."""
    from monosowa_amd.history import default_group
    acc = {g: [np.longdouble(0), 0] for g in hist.groups}
    for n, p in rig.model.named_parameters():
        if p.grad is None:
            continue
        x = snapshot[n].reshape(-1)
        acc[default_group(n)][0] += np.sum(np.square(x.astype(np.longdouble)))
        acc[default_group(n)][1] += x.size
    return {g: (float(s), n) for g, (s, n) in acc.items()}


@pytest.mark.parametrize("K", [1, 2])
def test_steps_with_the_key_on_and_off_train_identically_and_the_rows_hold_what_the_step_saw(shared, K):
    steps = 2
    seeds = [3, 7, 11, 13][:steps * K]
    cfg = {"global_batch": 4} if K == 2 else {}
    with _mode(True):
        off = _Rig(shared, seeds, **cfg)
        assert off.trainer.history is None and off.trainer.accum_steps == K
        _steps(off, K, steps)
        on = _Rig(shared, seeds, history=True, **cfg)
        hist = on.trainer.history
        assert hist is not None and hist.ring is None and hist.capacity == steps
        with _Terms(on.crit) as terms:
            snaps = _steps(on, K, steps)
    a, b = off.state(), on.state()
    assert set(a) == set(b) and len(a) > 900 and any(k.startswith("exp_avg_sq.") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between the runs with the key off and on" % k
    assert hist.kernel_commits == steps and len(terms.calls) == steps * K
    reference = _param_reference(on, hist, snaps[-1])
    rows = hist.drain()
    assert len(rows) == steps and [(r["step"], r["micro_batches"]) for r in rows] == [(s, K) for s in range(steps)]
    assert "guard" not in rows[0] and rows[0]["lr"] == on.opt.param_groups[0]["lr"]
    weight_dict = on.crit.weight_dict
    for s, row in enumerate(rows):
        calls = terms.calls[s * K:(s + 1) * K]
        assert list(row["losses"]) == [k for k in weight_dict if k in calls[0]] and len(row["losses"]) > 20
        for key, got in row["losses"].items():
            if K == 1:
                assert got == float(calls[0][key]), (s, key)                       # exactly float64(term)
            else:
                want = sum(float(c[key]) for c in calls) / K
                assert abs(got - want) <= 4 * np.spacing(abs(want)), (s, key, got, want)
        want = sum(sum(c[k] * weight_dict[k] for k in c) for c in calls) / K
        assert abs(row["loss_detr"] - want) <= 1e-5 * abs(want), (s, row["loss_detr"], want)     # the float32 totals against float64
        assert all(v == 0 for v in row["grad_nonfinite"].values()) and row["grad_norm"]["class_embed"] > 0
    worst = 0.0
    for g, (sumsq, n) in reference.items():
        got, want = rows[-1]["param_norm"][g], math.sqrt(sumsq)
        assert abs(got - want) <= n * U * want, (g, got, want, n)
        worst = max(worst, abs(got - want) / (n * U * want) if n else 0.0)
    assert sum(n for _, n in reference.values()) > 10e6 and sum(1 for _, n in reference.values() if n) > 8
    print("\nK = %d: worst |param_norm - reference| / (n * 2^-53 * reference) over %d groups = %.4f" % (K, len(reference), worst))


def test_train_step_with_the_key_on_does_not_synchronise(shared):
    from monosowa_amd.helpers.trainer_helper import stage_batch
    rig = _Rig(shared, [3, 7, 11], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, history=True)
    hist = rig.trainer.history
    batches = [stage_batch(raw, rig.trainer.device) for raw in rig.loader.batches]
    rig.trainer.train_step(*batches[0])                   # plans, tables, group ids and kernel selection belong to the first step
    arrays = {k: v[1] for k, v in hist._arrays.items()}
    assert hist.kernel_commits == 1 and len(arrays) == 2   # the two parameter groups of build_optimizer
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rig.trainer.train_step(*batches[1])
            rig.trainer.train_step(*batches[2])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()] == []
    assert hist.kernel_commits == 3 and all(hist._arrays[k][1] is v for k, v in arrays.items()) and len(hist._arrays) == 2
    rows = hist.drain()
    report = rig.opt.guard_report()
    assert len(rows) == 3 and all(r["guard"]["skip"] == 0 and r["guard"]["coef"] < 1.0 for r in rows)
    assert rows[-1]["guard"]["norm"] == report["grad_norm"] and rows[-1]["guard"]["coef"] == report["coef"]
    total = float(np.float32(math.sqrt(sum(v * v for v in rows[-1]["grad_norm"].values()))))
    assert abs(total - report["grad_norm"]) <= float(np.spacing(np.float32(report["grad_norm"])))          # one float32 ulp


def test_a_nan_gradient_is_localised_to_its_group_and_the_skipped_step_leaves_the_parameters(shared):
    rig = _Rig(shared, [3, 7], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, history=True)
    hist = rig.trainer.history
    _steps(rig, 1, 1)
    name, victim = next((n, p) for n, p in rig.model.named_parameters()
                        if n.startswith("depth_predictor.") and n.endswith(".weight") and p.requires_grad and p.grad is not None)
    handle = victim.register_hook(lambda g: torch.full_like(g, float("nan")))
    try:
        rig.k = 1
        from monosowa_amd.helpers.trainer_helper import stage_batch
        rig.trainer.train_step(*stage_batch(rig.loader.batches[1], rig.trainer.device))
    finally:
        handle.remove()
    torch.cuda.synchronize()
    raw = hist.ring[:2].cpu()
    G = len(hist.groups)
    param_cols = [hist.n_loss + 3 * q + 1 for q in range(G)]
    assert torch.equal(raw[0, param_cols].view(torch.int64), raw[1, param_cols].view(torch.int64))      # bitwise: not a parameter moved
    rows = hist.drain()
    assert rows[0]["guard"]["skip"] == 0 and all(v == 0 for v in rows[0]["grad_nonfinite"].values())
    assert rows[1]["guard"]["skip"] == 1 and math.isnan(rows[1]["guard"]["norm"])
    assert rows[1]["grad_nonfinite"] == {g: (victim.numel() if g == "depth_predictor" else 0) for g in hist.groups}, name
    assert math.isnan(rows[1]["grad_norm"]["depth_predictor"])
    assert all(math.isfinite(v) for g, v in rows[1]["grad_norm"].items() if g != "depth_predictor")
    assert rows[1]["param_norm"] == rows[0]["param_norm"] and rig.opt.guard_report()["skipped_total"] == 1


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_train_writes_one_json_line_per_step_and_logs_the_epoch_means(shared, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rig = _Rig(shared, [3, 7], history=True, save_frequency=1, save_all=0, max_epoch=2)
    trainer = rig.trainer
    trainer.lr_scheduler = type("S", (), {"step": lambda self: None})()
    logs = _Logs()
    trainer.logger.addHandler(logs)
    level = trainer.logger.level
    trainer.logger.setLevel(logging.INFO)
    try:
        trainer.train()
    finally:
        trainer.logger.removeHandler(logs)
        trainer.logger.setLevel(level)
    out = os.path.join(str(tmp_path), "outputs", "shipped")
    assert sorted(os.listdir(out)) == ["checkpoint.pth", "history.jsonl"]

    def strict(name):
        raise AssertionError("not valid JSON: " + name)
    rows = [json.loads(l, parse_constant=strict) for l in open(os.path.join(out, "history.jsonl")).read().splitlines()]
    assert [(r["epoch"], r["step"]) for r in rows] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert all(set(r) == {"epoch", "step", "lr", "micro_batches", "losses", "loss_detr", "grad_norm", "param_norm", "grad_nonfinite"}
               for r in rows)
    assert all(isinstance(r["loss_detr"], float) and r["grad_norm"]["backbone.layer4"] > 0 for r in rows)
    for epoch in (0, 1):
        assert any(l.startswith("Epoch %d: mean over 2 of 2 steps: loss_detr: " % epoch) and "loss_ce: " in l for l in logs.lines)
        assert any(l.startswith("Epoch %d: grad_norm median: " % epoch) for l in logs.lines)
    assert trainer.history.kernel_commits == 4
    assert set(torch.load(os.path.join(out, "checkpoint.pth"), map_location="cpu", weights_only=False)) == CHECKPOINT_KEYS


def test_without_the_key_nothing_is_built_written_or_launched(shared, tmp_path, monkeypatch):
    from monosowa_amd import history, pointwise
    monkeypatch.chdir(tmp_path)

    def never(*a, **k):
        raise AssertionError("the history was touched with the key absent")
    monkeypatch.setattr(pointwise, "step_stats", never)
    monkeypatch.setattr(pointwise.load(), "mono_step_stats_f32", never)
    monkeypatch.setattr(history.StepHistory, "__init__", never)
    rig = _Rig(shared, [3, 7])
    assert rig.trainer.history is None
    rig.trainer.train_one_epoch(0)
    assert rig.k == 2 and rig.opt.last_fused_plans() is not None and len(rig.opt.last_fused_plans()) == 2
    assert not os.path.exists(os.path.join(str(tmp_path), "outputs"))
