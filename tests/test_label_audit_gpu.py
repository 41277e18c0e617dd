"""``trainer.label_audit`` on the GPU: ``mono_label_audit_f32`` alone against the label-by-label float64 reference
(tests/label_audit_reference.py) and against the fused criterion's per-layer sums, its placement independence, confinement and return
codes, a NaN that stays with its label, and train steps of the shipped architecture (dropout 0, 640 x 192, batch 2, the rig of
tests/test_accumulation_gpu.py) with the key on and off, plain and with ``global_batch`` giving K = 2, and ``LabelAudit.scan``.

Metric: |x - x_R| / max(|x_R|, 1e-30) per element of the [T, 9] rows, x_R the float64 evaluation from the float32 inputs.
BOUND: 4 x the worst such error of the SAME expressions evaluated in float32 torch on the CPU (``rows(case, layer, torch.float32)``)
over the two shared cases and the layers 0 and 2; the factor 4 covers the device library's expf / logf against libm and another
contraction of the products (the practice of tests/test_criterion_kernels_gpu.py).  The means themselves are taken in float64 on both
sides: their error is orders below."""
import logging
import os
import warnings

import numpy as np
import pytest
import torch

import label_audit_reference as R
from test_accumulation_gpu import RES, _Rig, dev, shared      # noqa: F401  (fixtures)
from test_criterion_kernels_gpu import A_VALUE
from test_ema_cpu import CHECKPOINT_KEYS
from test_history_gpu import _Logs
from test_train_step_grads_gpu import _mode

pytestmark = pytest.mark.gpu
# worst e_kernel (MI355X) / worst e_P (float32 torch on the CPU), both over G3 and G1 at the layers 0 and 2, and 4 x e_P
BOUND = 5.2e-7           # 1.1e-7 (G3, layer 0, the heading column) / 1.3e-7 (G3, layer 2, the 1 - GIoU column), 5.2e-7
SENTINEL = 777.0
TINY = 1e-30


def _tensors(case, device):
    """The twelve kernel arguments in the entry point's order, contiguous on the device."""
    order = ("logits", "boxes", "depth", "dims", "angle", "idx", "labels", "t_box", "t_depth", "t_size", "t_bin", "t_res")
    return [case[k].to(device).contiguous() for k in order]


def _run(case, layer, device, out=None):
    """The kernel's [T, 9] rows of ``layer`` (into ``out``'s storage when given)."""
    from monosowa_amd import pointwise
    T = case["labels"].shape[0]
    if out is None:
        out = torch.full((T, 9), SENTINEL, dtype=torch.float64, device=device)
    tensors = _tensors(case, device)
    assert pointwise.label_audit_supported(tensors[0])
    pointwise.label_audit(*tensors, out.data_ptr(), T, layer)
    return out


# =================================================================================================== 1. values against float64
@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("layer", [0, 2])
def test_rows_equal_the_float64_reference(dev, name, layer):
    case = R.shared_case(name)
    NL, B, C, Q, G, sizes = R.CASES[name]
    T = sum(sizes)
    assert case["idx"].shape == (3, NL, G * T) and 0 in sizes
    want = R.rows(case, layer)
    e_p = R.rel_error(R.rows(case, layer, torch.float32), want)
    got = _run(case, layer, dev).cpu()
    e_f = R.rel_error(got, want)
    per_column = ((got - want).abs() / want.abs().clamp_min(TINY)).max(0).values.tolist()
    print("\nMEASURED %s layer %d: e_F %.3e  e_P %.3e  bound %.1e  per column %s" % (name, layer, e_f, e_p, BOUND, ["%.1e" % e for e in per_column]))
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, 8], torch.full((T,), float(G), dtype=torch.float64))            # the count is exact
    assert e_f <= BOUND and e_p <= BOUND
    # the layers hold other predictions and other pairs: reading the wrong one cannot pass
    assert R.rel_error(got[:, :8], R.rows(case, 2 - layer)[:, :8]) > 1e-2


# =================================================================================================== 2. against the fused criterion
@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("layer", [0, 2])
def test_rows_times_counts_add_up_to_the_fused_criterions_sums(dev, name, layer):
    """mono_matched_losses_fwd_f32's out[layer] = {center, bbox, giou, depth, dim, angle}; its dim entry is (sum of |s - s*| / s*) x
    (sum |s - s*| / that sum) = the plain size-L1 sum, the audit's column 5."""
    from monosowa_amd.pointwise import matched_losses
    case = R.shared_case(name)
    got = _run(case, layer, dev).cpu()
    t = _tensors(case, dev)
    sums = matched_losses(t[1], t[2], t[3], t[4], t[5], *t[7:]).double().cpu()[layer]
    mine = (got[:, [0, 1, 2, 3, 5, 6]] * got[:, 8:9]).sum(0)
    err = ((mine - sums).abs() / sums.abs().clamp_min(TINY)).tolist()
    print("\nMEASURED %s layer %d: sum_t values x count against the fused sums %s (bound %.1e)" % (name, layer, ["%.1e" % e for e in err], A_VALUE + BOUND))
    assert max(err) <= A_VALUE + BOUND


# =================================================================================================== 3. reproducible and confined
def test_two_placements_give_the_same_bytes_and_nothing_else_is_written(dev):
    from monosowa_amd import pointwise
    case = R.shared_case("G3")
    T = case["labels"].shape[0]
    buf = torch.full((4096,), SENTINEL, dtype=torch.float64, device=dev)
    a, b = buf[3:3 + 9 * T].view(T, 9), buf[2050:2050 + 9 * T].view(T, 9)
    assert a.data_ptr() % 16 != b.data_ptr() % 16
    _run(case, 0, dev, out=a)
    _run(case, 0, dev, out=b)
    assert torch.equal(a, b) and torch.equal(a.view(torch.int64), b.view(torch.int64)) and not (a == SENTINEL).any()
    inside = torch.zeros(4096, dtype=torch.bool, device=dev)
    inside[3:3 + 9 * T] = inside[2050:2050 + 9 * T] = True
    assert (buf[~inside] == SENTINEL).all()
    # every input is read only
    fresh = R.make_case(51 + 2 + 30, *[R.CASES["G3"][i] for i in (0, 1, 3, 2, 4, 5)])
    assert all(torch.equal(case[k], fresh[k]) for k in case)

    # return codes: nothing is launched, nothing is written
    lib = pointwise.load()
    NL, B, C, Q, G, sizes = R.CASES["G3"]
    ptrs = [x.data_ptr() for x in _tensors(case, dev)]
    out = torch.full((T + 2, 9), SENTINEL, dtype=torch.float64, device=dev)
    call = lambda p, o, *ints: lib.mono_label_audit_f32(*p, o, *ints, None)
    good = (NL, B, Q, C, G * T, T, 0)
    assert call(ptrs, out[1:].data_ptr(), NL, B, Q, C, G * T, 0, 0) == 0                         # T == 0
    for i in range(12):
        assert call(ptrs[:i] + [None] + ptrs[i + 1:], out[1:].data_ptr(), *good) == -1, i
    assert call(ptrs, None, *good) == -1
    for bad in ((NL, B, Q, C, G * T, T, NL), (NL, B, Q, C, G * T, T, -1), (NL, B, Q, 256, G * T, T, 0), (NL, B, Q, C, -1, T, 0),
                (NL, B, Q, C, G * T, -1, 0), (0, B, Q, C, G * T, T, 0), (NL, -1, Q, C, G * T, T, 0), (NL, B, 0, C, G * T, T, 0),
                (NL, B, Q, 0, G * T, T, 0)):
        assert call(ptrs, out[1:].data_ptr(), *bad) == -2, bad
    assert not pointwise.label_audit_supported(torch.zeros(1, 1, 1, 256, device=dev))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # K == 0 with labels: every row is nine zeros (idx may be NULL then)
    assert call(ptrs[:5] + [None] + ptrs[6:], out[1:].data_ptr(), NL, B, Q, C, 0, T, 0) == 0
    torch.cuda.synchronize()
    assert (out[0] == SENTINEL).all() and (out[T + 1] == SENTINEL).all() and not out[1:T + 1].any()


# =================================================================================================== 4. NaN stays with its label
def test_a_nan_depth_of_one_matched_query_stays_in_its_labels_row(dev):
    case = {k: v.clone() for k, v in R.shared_case("G3").items()}
    clean = _run(case, 2, dev).cpu()
    k = 40
    b, q, t = case["idx"][:, 2, k].tolist()
    case["depth"][2, b, q, 0] = float("nan")
    got = _run(case, 2, dev).cpu()
    assert torch.isnan(got[t, [3, 4]]).all()
    keep = torch.ones(clean.shape, dtype=torch.bool)
    keep[t, 3] = keep[t, 4] = False
    assert torch.equal(got.view(torch.int64)[keep], clean.view(torch.int64)[keep]) and torch.isfinite(got[keep]).all()
    # the same NaN in a layer the call does not read changes nothing
    assert torch.equal(_run(case, 0, dev).cpu(), _run(R.shared_case("G3"), 0, dev).cpu())


# =================================================================================================== 5. the Trainer
SEEDS = [3, 7, 11, 13, 17, 19]


def _cfg(K):
    return {"global_batch": 4} if K == 2 else {}


def _name_images(rig):
    """Every image of the rig's loader gets its own id (``make_batch`` hands out zeros)."""
    for i, batch in enumerate(rig.loader.batches):
        batch[3]["img_id"] = np.array([1000 + 10 * i + 7, 1000 + 10 * i + 2])


def _loader_keys(batches):
    ids, lines = [], []
    for batch in batches:
        hb, hs = np.nonzero(batch[2]["mask_2d"].numpy())
        ids += batch[3]["img_id"][hb].tolist()
        lines += hs.tolist()
    return ids, lines


def _run_steps(rig, K, steps, first=0):
    """``steps`` optimizer steps of K loader batches each from step ``first`` on, forward j seeded with 100 + j; -> [(total, loss matrix)]."""
    from monosowa_amd.helpers.trainer_helper import stage_batch
    out = []
    for s in range(first, first + steps):
        rig.k = s * K
        raws = rig.loader.batches[s * K:(s + 1) * K]
        total, ld = rig.trainer.train_step(*stage_batch(raws[0], rig.trainer.device)) if K == 1 else rig.trainer.train_cycle(raws)
        out.append((total.detach().clone(), ld.mat.detach().clone()))
    return out


class _Spy:
    """Keeps copies of what the criterion hands ``observe`` (device copies: nothing waits) and passes the call on."""

    def __init__(self, audit):
        self.calls, self.audit, self.observe = [], audit, audit.observe
        audit.observe = self

    def __call__(self, *args, **kwargs):
        self.calls.append(([a.detach().clone() for a in args[:6]] + [{k: v.detach().clone() for k, v in args[6].items()}], kwargs))
        return self.observe(*args, **kwargs)


@pytest.mark.parametrize("K", [1, 2])
def test_steps_with_the_key_on_and_off_train_identically_and_the_rows_name_and_measure_the_steps_labels(shared, K):
    steps = 2
    seeds = SEEDS[:steps * K]
    try:
        with _mode(True):
            off = _Rig(shared, seeds, **_cfg(K))
            assert off.trainer.label_audit is None and off.crit.audit is None and off.trainer.accum_steps == K
            plain = _run_steps(off, K, steps)
            on = _Rig(shared, seeds, label_audit=True, **_cfg(K))
            audit = on.trainer.label_audit
            assert audit is not None and on.crit.audit is audit and audit.capacity == len(seeds) * 2 * 50
            _name_images(on)
            spy = _Spy(audit)
            audited = _run_steps(on, K, steps)
    finally:
        shared[2].__dict__.pop("audit", None)
    # (a) the same losses and the same updated parameters, bit for bit
    for (t0, m0), (t1, m1) in zip(plain, audited):
        assert torch.equal(t0, t1) and torch.equal(m0, m1)
    a, b = off.state(), on.state()
    assert set(a) == set(b) and len(a) > 900 and any(k.startswith("exp_avg_sq.") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between the runs with the key off and on" % k
    assert audit.kernel_observes == steps * K == len(spy.calls) and audit.early_drains == 0
    # (b) the keys are the host masks' (img_id, line) pairs in order, every label has group_num pairs
    got = audit.drain()
    ids, lines = _loader_keys(on.loader.batches)
    assert got["img_id"].tolist() == ids and got["line"].tolist() == lines and len(ids) > 20
    assert got["epoch"].tolist() == [0] * len(ids) and (got["cls"] == 1).all()
    assert (got["values"][:, 8] == on.crit.group_num).all() and on.crit.group_num > 1
    # (c) the values against the float64 reference fed with the step's own outputs and pairs
    row, worst = 0, 0.0
    for args, kwargs in spy.calls:
        assert kwargs == {"layer": 0}
        case = R.case_of_observe(args)
        want = R.rows(case, 0)
        err = R.rel_error(torch.from_numpy(got["values"][row:row + len(want)]), want)
        worst = max(worst, err)
        row += len(want)
    print("\nMEASURED K = %d: worst error of the drained rows against the float64 reference %.3e (bound %.1e)" % (K, worst, BOUND))
    assert row == len(ids) and worst <= BOUND
    assert audit.drain()["values"].shape == (0, 9)


@pytest.mark.parametrize("K", [1, 2])
def test_steps_with_the_key_on_do_not_synchronise(shared, K):
    try:
        rig = _Rig(shared, SEEDS[:3 * K], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, label_audit=True, **_cfg(K))
        audit = rig.trainer.label_audit
        _run_steps(rig, K, 1)                              # plans, tables and kernel selection belong to the first step
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                _run_steps(rig, K, 2, first=1)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    finally:
        shared[2].__dict__.pop("audit", None)
    assert [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()] == []
    assert audit.kernel_observes == 3 * K and audit.early_drains == 0
    got = audit.drain()
    assert len(got["line"]) == sum(int(b[2]["mask_2d"].sum()) for b in rig.loader.batches) and np.isfinite(got["values"]).all()


def test_train_writes_one_file_per_epoch_and_logs_the_summary(shared, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    try:
        rig = _Rig(shared, [3, 7], label_audit=True, save_frequency=1, save_all=0, max_epoch=2)
        _name_images(rig)
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
    finally:
        shared[2].__dict__.pop("audit", None)
    out = os.path.join(str(tmp_path), "outputs", "shipped")
    assert sorted(os.listdir(out)) == ["checkpoint.pth", "label_audit"]
    assert sorted(os.listdir(os.path.join(out, "label_audit"))) == ["epoch_000.npz", "epoch_001.npz"]
    ids, lines = _loader_keys(rig.loader.batches)
    for epoch in (0, 1):
        got = np.load(os.path.join(out, "label_audit", "epoch_%03d.npz" % epoch))
        assert set(got.files) == {"epoch", "img_id", "line", "cls", "values", "columns"}
        assert got["img_id"].tolist() == ids and got["line"].tolist() == lines and got["epoch"].tolist() == [epoch] * len(ids)
        assert got["values"].shape == (len(ids), 9) and (got["values"][:, 8] == rig.crit.group_num).all()
        assert any(l.startswith("Epoch %d: label audit: %d labels seen, |d - d*| median: " % (epoch, len(ids))) and "max: " in l for l in logs.lines)
    assert trainer.label_audit.kernel_observes == 4
    assert set(torch.load(os.path.join(out, "checkpoint.pth"), map_location="cpu", weights_only=False)) == CHECKPOINT_KEYS


def test_without_the_key_nothing_is_built_written_or_launched(shared, tmp_path, monkeypatch):
    from monosowa_amd import label_audit, pointwise
    monkeypatch.chdir(tmp_path)

    def never(*a, **k):
        raise AssertionError("the label audit was touched with the key absent")
    monkeypatch.setattr(pointwise, "label_audit", never)
    monkeypatch.setattr(pointwise.load(), "mono_label_audit_f32", never)
    monkeypatch.setattr(label_audit.LabelAudit, "__init__", never)
    monkeypatch.setattr(label_audit, "columns_torch", never)
    rig = _Rig(shared, [3, 7])
    assert rig.trainer.label_audit is None and rig.crit.audit is None and "audit" not in rig.crit.__dict__
    rig.trainer.train_one_epoch(0)
    assert rig.k == 2
    assert not os.path.exists(os.path.join(str(tmp_path), "outputs"))


# =================================================================================================== 6. scan
def test_scan_pairs_every_label_once_and_names_it_like_the_loader(shared, dev):
    from monosowa_amd import LabelAudit
    rig = _Rig(shared, [3, 7, 11])
    _name_images(rig)
    audit = LabelAudit(3 * 2 * 50, dev)
    got = audit.scan(rig.model, rig.crit, rig.loader, dev)
    assert rig.model.training and rig.crit.training and rig.crit.audit is None and "audit" not in rig.crit.__dict__
    ids, lines = _loader_keys(rig.loader.batches)
    assert got["img_id"].tolist() == ids and got["line"].tolist() == lines
    assert (got["values"][:, 8] == 1).all() and np.isfinite(got["values"]).all() and audit.kernel_observes == 3
    assert (got["values"][:, [0, 1, 2, 4, 5, 6]] > 0).all() and ((got["values"][:, 7] > 0) & (got["values"][:, 7] < 1)).all()
