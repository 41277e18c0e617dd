"""``trainer.ema_decay`` on the GPU: ``mono_ema_update_f32`` alone and under a guard record, train steps of the shipped architecture
(dropout 0, 640 x 192, batch 2, the rig of tests/test_accumulation_gpu.py) with the key on and off under the deterministic flag, no host
synchronisation, nothing stale in what the eval forward derives from parameters, the device-side skip, and ``Trainer.train()``'s
evaluation on the averaged weights.  The reference is numpy in float32 (tests/test_ema_cpu.py ``ema_reference``): three roundings."""
import logging
import os
import warnings

import numpy as np
import pytest
import torch

import test_detector_gpu as D
from test_accumulation_gpu import CHUNK, RES, SENTINEL, _Rig, _kernel_layout, _view, dev, shared      # noqa: F401  (fixtures)
from test_ema_cpu import CHECKPOINT_KEYS, SPECIAL, assert_same_bits, ema_reference
from test_train_step_grads_gpu import _mode

pytestmark = pytest.mark.gpu
kitti = D.kitti                                # the fixture: a KITTI directory written from the golden files
W = np.float32(1.0 - 10 / 19)                  # the schedule's w at t = 9


# --------------------------------------------------------------------------------------------------------------- 1. / 2. kernel alone
def _kernel_case(dev):
    """Averages and parameters laid out in two buffers with sentinels in between (``_kernel_layout``): sizes 1 ... 65537, the three
    misaligned pairs, a channels-last tensor, 600 seven-element tensors at every alignment; the specials at head and tail of each
    tensor that holds them twice, one special in every other."""
    layout, length = _kernel_layout()
    assert [int(np.prod(s)) for s, _, _, _ in layout[:9]] == [1, 3, 4, 5, 255, 32767, 32768, 32769, 65537]
    rng = np.random.default_rng(31)
    e_h = np.full(length, SENTINEL, dtype=np.float32)
    p_h = np.full(length, -SENTINEL, dtype=np.float32)
    inside = np.zeros(length, dtype=bool)
    k = len(SPECIAL)
    for i, (shape, e0, p0, _) in enumerate(layout):
        n = int(np.prod(shape))
        e, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        if n >= 2 * k:
            e[:k], p[:k] = zip(*SPECIAL)
            e[-k:], p[-k:] = zip(*SPECIAL)
        else:
            e[0], p[0] = SPECIAL[i % k]
        assert not inside[e0:e0 + n].any()
        e_h[e0:e0 + n], p_h[p0:p0 + n] = e, p
        inside[e0:e0 + n] = True
    assert not inside[0] and not inside[-1] and all(not inside[e0 - 1] and not inside[e0 + int(np.prod(s))] for s, e0, _, _ in layout)
    want = e_h.copy()
    for shape, e0, p0, _ in layout:
        n = int(np.prod(shape))
        want[e0:e0 + n] = ema_reference(e_h[e0:e0 + n], p_h[p0:p0 + n], W)
    ebuf, pbuf = torch.from_numpy(e_h).to(dev), torch.from_numpy(p_h).to(dev)
    assert ebuf.data_ptr() % 16 == 0 and pbuf.data_ptr() % 16 == 0
    avgs = [_view(ebuf, e0, shape, cl) for shape, e0, _, cl in layout]
    params = [_view(pbuf, p0, shape, cl) for shape, _, p0, cl in layout]
    assert {(a.data_ptr() % 16, b.data_ptr() % 16) for a, b in zip(avgs[9:12], params[9:12])} == {(4, 4), (4, 0), (0, 4)}
    assert avgs[12].is_contiguous(memory_format=torch.channels_last) and len({a.data_ptr() % 16 for a in avgs[13:]}) == 4
    # every access of the kernel lies inside the two buffers: the table's counts are the tensors' sizes
    for a, b in zip(avgs, params):
        assert ebuf.data_ptr() <= a.data_ptr() and a.data_ptr() + 4 * a.numel() <= ebuf.data_ptr() + 4 * length
        assert pbuf.data_ptr() <= b.data_ptr() and b.data_ptr() + 4 * b.numel() <= pbuf.data_ptr() + 4 * length
    return {"e_h": e_h, "p_h": p_h, "inside": inside, "want": want, "ebuf": ebuf, "pbuf": pbuf, "avgs": avgs, "params": params}


def _assert_kernel_result(case):
    got = case["ebuf"].cpu().numpy()
    want, inside = case["want"], case["inside"]
    nan = np.isnan(want)
    assert nan.sum() >= 3 * 6 and np.isinf(want).any() and ((want != 0) & (np.abs(want) < 1e-38)).any()
    assert_same_bits(got, want)
    assert np.array_equal(got.view(np.int32)[~inside], case["e_h"].view(np.int32)[~inside])          # every sentinel unchanged
    assert np.array_equal(case["pbuf"].cpu().numpy().view(np.int32), case["p_h"].view(np.int32))     # the parameters are read only


def test_kernel_averages_exactly_the_tensor_elements_bit_for_bit(dev):
    from monosowa_amd import pointwise
    from monosowa_amd.ema import EMAPlan
    case = _kernel_case(dev)
    assert pointwise.accumulate_supported(case["avgs"], case["params"])
    plan = EMAPlan(case["avgs"], case["params"])
    assert plan.n_chunks == sum(-(-a.numel() // CHUNK) for a in case["avgs"]) == 613 + 1 + 2       # 32769 -> 2 chunks, 65537 -> 3
    assert plan.matches(case["avgs"], case["params"]) and not plan.matches(case["params"], case["avgs"])
    plan.launch(W)
    torch.cuda.synchronize()
    _assert_kernel_result(case)
    lib = pointwise.load()
    assert lib.mono_ema_update_f32(plan.dev.data_ptr(), 0, float(W), None, None) == 0               # nothing to do, nothing launched
    assert lib.mono_ema_update_f32(plan.dev.data_ptr(), -1, float(W), None, None) != 0
    assert lib.mono_ema_update_f32(None, plan.n_chunks, float(W), None, None) != 0
    torch.cuda.synchronize()
    _assert_kernel_result(case)


def test_kernel_under_a_guard_record_stores_nothing_when_the_step_is_skipped(dev):
    """The record comes from ``GradGuard.run`` over a gradient set with and without a NaN."""
    from monosowa_amd.ema import EMAPlan
    from monosowa_amd.pointwise import FusedAdamWPlan, GradGuard
    case = _kernel_case(dev)
    plan = EMAPlan(case["avgs"], case["params"])
    ps = [torch.zeros(1000, device=dev), torch.zeros(CHUNK + 3, device=dev)]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    grads = [torch.full_like(p, 0.5) for p in ps]
    table = FusedAdamWPlan(ps, ms, vs, 0.0)
    guard = GradGuard(dev)
    grads[1][CHUNK + 1] = float("nan")
    table.refresh(grads)
    guard.run([table], 0.1, True)
    plan.launch(W, guard.record.data_ptr())
    torch.cuda.synchronize()
    assert guard.report()["skip"] == 1 and guard.report()["skipped_total"] == 1
    assert np.array_equal(case["ebuf"].cpu().numpy().view(np.int32), case["e_h"].view(np.int32))     # not a byte of e changed
    grads[1][CHUNK + 1] = 0.5
    table.refresh(grads)
    guard.run([table], 0.1, True)
    plan.launch(W, guard.record.data_ptr())                                                          # the same record, skip = 0
    torch.cuda.synchronize()
    report = guard.report()
    assert report["skip"] == 0 and report["skipped_total"] == 1 and report["coef"] < 1.0
    _assert_kernel_result(case)


# --------------------------------------------------------------------------------------------------------------- 3. key on and off
def _params(rig):
    return {n: p.detach().cpu().numpy().copy() for n, p in rig.model.named_parameters()}


def _steps(rig, K, n_steps):
    """n_steps optimizer steps of K loader batches each; forward j of the run is seeded with 100 + j on every rig.  Parameter
    snapshots before the first and after every step."""
    from monosowa_amd.helpers.trainer_helper import stage_batch
    snaps = [_params(rig)]
    for s in range(n_steps):
        rig.k = s * K
        raws = rig.loader.batches[s * K:(s + 1) * K]
        if K == 1:
            rig.trainer.train_step(*stage_batch(raws[0], rig.trainer.device))
        else:
            rig.trainer.train_cycle(raws)
        snaps.append(_params(rig))
    return snaps


def _assert_replay(ema, snaps, first_update=0):
    """The averaged tensors against the numpy replay from the snapshots (warm-up schedule, update t uses snapshot t + 1)."""
    from monosowa_amd.ema import ema_weight
    tracked = ema.tracked()
    assert len(tracked) > 300
    assert all(e.stride() == p.stride() for e, p in zip(*ema._pairs()))          # the copy keeps its parameter's layout
    moved = 0
    for n, e in tracked.items():
        want = snaps[0][n]
        for t in range(len(snaps) - 1):
            want = ema_reference(want, snaps[t + 1][n], ema_weight(ema.decay, first_update + t, ema.warmup))
        got = e.detach().cpu().numpy()
        assert_same_bits(got, want, n)
        moved += int(not np.array_equal(want, snaps[0][n]) and not np.array_equal(want, snaps[-1][n]))
    assert moved > 250


@pytest.mark.parametrize("K", [1, 2])
def test_steps_with_the_key_on_and_off_train_identically_and_the_average_is_the_replay(shared, K):
    steps = 3 if K == 1 else 2
    seeds = [3, 7, 11, 13][:steps * K]
    cfg = {"global_batch": 4} if K == 2 else {}
    with _mode(True):
        off = _Rig(shared, seeds, **cfg)
        assert off.trainer.ema is None and off.trainer.accum_steps == K
        _steps(off, K, steps)
        on = _Rig(shared, seeds, ema_decay=0.999, **cfg)
        ema = on.trainer.ema
        assert ema is not None and ema.updates == 0 and ema.plan is None
        snaps = _steps(on, K, steps)
    a, b = off.state(), on.state()
    assert set(a) == set(b) and len(a) > 900 and any(k.startswith("exp_avg_sq.") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between the runs with the key off and on" % k
    assert ema.updates == steps and ema.plan is not None and ema.plan.launches == steps           # one update per optimizer step / cycle
    _assert_replay(ema, snaps)


# --------------------------------------------------------------------------------------------------------------- 4. no host sync
def test_train_step_with_the_key_on_does_not_synchronise(shared, monkeypatch):
    from monosowa_amd import ema as E
    from monosowa_amd.helpers.trainer_helper import stage_batch
    built = []
    init = E.EMAPlan.__init__
    monkeypatch.setattr(E.EMAPlan, "__init__", lambda self, *a: (built.append(1), init(self, *a))[1])
    rig = _Rig(shared, [3, 7, 11], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, ema_decay=0.999)
    batches = [stage_batch(raw, rig.trainer.device) for raw in rig.loader.batches]
    rig.trainer.train_step(*batches[0])                   # plans, tables and kernel selection belong to the first step
    plan = rig.trainer.ema.plan
    assert built == [1] and plan.launches == 1
    table = plan.dev.cpu().numpy().copy()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            rig.trainer.train_step(*batches[1])
            assert plan.launches == 2
            rig.trainer.train_step(*batches[2])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()] == []
    assert rig.trainer.ema.plan is plan and plan.launches == 3 and built == [1]           # one launch per step, the table shipped once
    assert np.array_equal(plan.dev.cpu().numpy(), table)
    assert rig.opt.guard_record_address() == rig.opt._guard.record.data_ptr() and rig.opt.last_step_skipped() is False
    assert rig.opt.guard_report()["skipped_total"] == 0 and rig.trainer.ema.updates == 3


# --------------------------------------------------------------------------------------------------------------- 5. nothing stale
def _eval_forward(model, batch):
    inputs, calibs, targets, _ = batch
    with torch.no_grad():
        out = model.eval()(inputs, calibs, None, targets["img_size"], dn_args=0)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


def _fresh_model_from(shared, state):
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    cfg = shared[0]
    torch.manual_seed(1)
    model, _ = build_model(dict(cfg["model"], device="cuda", dropout=0.0, depth_map_size=(RES[0] // 16, RES[1] // 16)))
    model = to_mi355x_layout(model.to(next(iter(state.values())).device))
    model.load_state_dict(state)
    return model.eval()


def test_eval_forward_on_the_average_sees_every_update(shared, dev):
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.synthetic import make_batch
    with _mode(True):
        rig = _Rig(shared, [3, 7, 11], ema_decay=0.999)
        ema = rig.trainer.ema
        batches = [stage_batch(raw, rig.trainer.device) for raw in rig.loader.batches]
        probe = stage_batch(make_batch(2, "cpu", seed=21, resolution=RES), rig.trainer.device)
        rig.trainer.train_step(*batches[0])
        first = _eval_forward(ema.sync_untracked(), probe)
        assert any("_folded" in m.__dict__ for m in ema.module.modules()), "the eval forward is expected to keep folded weights"
        rig.model.train()
        for b in batches[1:]:
            rig.trainer.train_step(*b)
        assert ema.updates == 3 and not ema.module.training
        second = _eval_forward(ema.sync_untracked(), probe)
        want = _eval_forward(_fresh_model_from(shared, ema.state_dict()["module"]), probe)
    assert set(first) == set(second) == set(want) and {"pred_logits", "pred_boxes", "pred_depth"} <= set(want)
    for k in want:
        assert torch.equal(second[k], want[k]), "%s of the averaged module differs from a fresh model on the same weights" % k
    assert any(not torch.equal(first[k], second[k]) for k in want)


def test_detector_on_the_average_sees_every_update(kitti):
    """detect, update, detect on ``Detector(cfg, model=ema.module)``: the rows of a fresh Detector on the same weights."""
    from monosowa_amd import Detector
    from monosowa_amd.ema import ModelEMA
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    fixtures, root = kitti
    model, crit, cfg = D._model()
    _, frames, P2 = D._frames_of(D._val_loader(fixtures, root, 3, device_aug=True))
    frames, P2 = frames[:3], P2[:3]
    dcfg = {"dataset": D._dataset_cfg(fixtures, root, 3), "tester": dict(D.TESTER_CFG), "model": cfg["model"]}
    opt = build_optimizer(cfg["optimizer"], model)
    ema = ModelEMA(model, 0.999)

    def train(seeds):
        model.train(), crit.train()
        for s in seeds:
            inputs, calibs, targets, _ = make_batch(2, D._dev(), seed=s, resolution=(320, 96))
            tl = prepare_targets(targets, 2)
            opt.zero_grad(set_to_none=True)
            weighted_total(crit(model(inputs.contiguous(memory_format=torch.channels_last), calibs, tl, targets["img_size"]), tl),
                           crit.weight_dict).backward()
            opt.step()
            ema.update(opt)
        model.eval()
    with D.deterministic():
        train([70])
        det = Detector(dcfg, model=ema.sync_untracked())
        first = det.detect(frames, P2, batch_size=3)
        assert det.engine.replays == 1
        train([71, 72])
        assert ema.updates == 3 and ema.plan.launches == 3
        second = det.detect(frames, P2, batch_size=3)
        assert det.engine.replays == 2 and det.engine.eager_forwards == 0          # from a graph again, a recaptured one
        det.close()
        fresh, _, _ = D._model(seed=1)
        fresh.load_state_dict(ema.state_dict()["module"])
        other = Detector(dcfg, model=fresh)
        want = other.detect(frames, P2, batch_size=3)
        other.close()
    for k in range(3):
        assert second[k].shape == (50, 14) and second[k].tobytes() == want[k].tobytes(), k
    assert any(a.tobytes() != b.tobytes() for a, b in zip(first, second))


# --------------------------------------------------------------------------------------------------------------- 6. device-side skip
def test_nan_micro_batch_under_the_device_guard_leaves_the_average_alone(shared):
    rig = _Rig(shared, [3, 7], optimizer={"clip_max_norm": 0.1, "skip_nonfinite": True}, global_batch=4, ema_decay=0.999)
    ema = rig.trainer.ema
    rig.cycle(step=True)
    assert rig.opt._guard is not None and rig.opt._guard_host is None, "the device path must have served the step"
    assert rig.opt.guard_report()["skipped_total"] == 0 and ema.updates == 1 and ema.plan.launches == 1
    bits = lambda: {n: e.detach().clone() for n, e in ema.module.named_parameters()}
    before, live = bits(), rig.state()
    clean = rig.loader.batches[1][0][1, 0, 5, 7].clone()
    rig.loader.batches[1][0][1, 0, 5, 7] = float("nan")              # in the LAST micro-batch, as test_accumulation_gpu.py does
    rig.cycle(step=True)
    assert rig.opt.guard_report()["skipped_total"] == 1
    assert ema.updates == 2 and ema.plan.launches == 2                # launched, and the kernel itself stored nothing
    after = bits()
    assert all(torch.equal(before[n], after[n]) for n in before)
    now = rig.state()
    assert all(torch.equal(live[k], now[k]) for k in live)
    try:                                   # whatever the shared matcher noted about that micro-batch's costs is taken down here
        rig.crit.matcher.check_device_status(block=True)
    except ValueError:
        pass
    rig.loader.batches[1][0][1, 0, 5, 7] = clean
    rig.cycle(step=True)                                              # the next clean step moves the average
    assert rig.opt.guard_report()["skipped_total"] == 1 and ema.updates == 3
    moved = bits()
    assert sum(not torch.equal(before[n], moved[n]) for n in ema.tracked()) > 250


# --------------------------------------------------------------------------------------------------------------- 7. Trainer.train()
class _StubTester:
    def __init__(self, model):
        self.model, self.seen, self.fail = model, [], False

    def inference(self):
        self.seen.append(self.model)
        if self.fail:
            raise RuntimeError("stub inference failure")

    def evaluate(self):
        return 1.0


def test_train_evaluates_the_average_and_saves_it_with_the_best_checkpoint(shared, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rig = _Rig(shared, [3, 7], ema_decay=0.999, save_frequency=1, save_all=0)
    trainer, ema = rig.trainer, rig.trainer.ema
    trainer.lr_scheduler = type("S", (), {"step": lambda self: None})()
    trainer.tester = tester = _StubTester(rig.model)
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    trainer.logger.addHandler(handler)
    level = trainer.logger.level
    trainer.logger.setLevel(logging.INFO)
    try:
        trainer.train()
    finally:
        trainer.logger.removeHandler(handler)
        trainer.logger.setLevel(level)
    assert tester.seen == [ema.module] and tester.model is rig.model and ema.updates == 2
    assert any(r.getMessage().startswith("Test Epoch 1") and "EMA" in r.getMessage() for r in records)
    out = os.path.join(str(tmp_path), "outputs", "shipped")
    assert sorted(os.listdir(out)) == ["checkpoint.pth", "checkpoint_best.pth"]
    for name in ("checkpoint.pth", "checkpoint_best.pth"):
        ckpt = torch.load(os.path.join(out, name), map_location="cpu", weights_only=False)
        assert set(ckpt) == CHECKPOINT_KEYS | {"ema_state"} and ckpt["ema_state"]["updates"] == 2
        mine, live = ema.module.state_dict(), rig.model.state_dict()
        assert list(ckpt["ema_state"]["module"]) == list(mine) == list(ckpt["model_state"])
        for n in mine:
            assert torch.equal(ckpt["ema_state"]["module"][n], mine[n].cpu()), n
            assert torch.equal(ckpt["model_state"][n], live[n].cpu()), n
    assert ckpt["best_result"] == 1.0 and ckpt["best_epoch"] == 1
    # the live model comes back after a failed pass as well
    tester.fail = True
    with pytest.raises(RuntimeError, match="stub inference failure"):
        trainer._evaluate()
    assert tester.model is rig.model and tester.seen[-1] is ema.module
