"""``trainer.ema_decay``: the exponential moving average of the weights on the CPU -- the torch fallback's three float32 roundings against
numpy, the warm-up schedule, the config key, two Trainer steps replayed from parameter snapshots, the checkpoint key through the Trainer,
``load_checkpoint``, the Detector and the Tester, and the guard's host-side skip.  The model is the tiny one of
tests/test_accumulation_cpu.py (``_build()``: MSDA through the oracle, depth map 12 x 4, dropout 0, 192 x 64, batch 2)."""
import logging
import os

import numpy as np
import pytest
import torch
import yaml

from test_accumulation_cpu import _Loader, _process_state, _seed_hook, _trainer      # noqa: F401  (_process_state: autouse fixture)
from test_distributed_gloo import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKPOINT_KEYS = {"epoch", "model_state", "optimizer_state", "best_result", "best_epoch"}

# (e, p) pairs: e == p, signed zeros, Inf - Inf, NaN in either operand, p - e overflowing, subnormal t, w * d underflowing to zero
SPECIAL = [(1.5, 1.5), (-2.25, -2.25), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0), (np.inf, np.inf), (-np.inf, -np.inf),
           (np.inf, -np.inf), (np.inf, 1.0), (1.0, -np.inf), (np.nan, 1.0), (1.0, np.nan), (np.nan, np.inf), (-3e38, 1e38), (3e38, -1e38),
           (0.0, 1e-38), (1e-38, 0.0), (1.0, 1.0 + 2.0 ** -20), (0.0, 1e-45), (1e-45, 0.0), (-1e-44, 1e-44), (1e-39, 3e-39),
           (16777216.0, 16777217.0), (3.0e38, 3.4e38)]


def ema_reference(e, p, w):
    """numpy in float32: d = p - e; t = w * d; e' = e + t, each rounded to float32."""
    e, p, w = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(w)
    with np.errstate(all="ignore"):
        d = (p - e).astype(np.float32)
        t = (w * d).astype(np.float32)
        out = (e + t).astype(np.float32)
    assert d.dtype == t.dtype == out.dtype == np.float32
    return out


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), what


def special_operands(n, rng):
    """n >= 2 * len(SPECIAL) random (e, p) values with the specials at both ends."""
    e, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    k = len(SPECIAL)
    e[:k], p[:k] = zip(*SPECIAL)
    e[-k:], p[-k:] = zip(*SPECIAL)
    return e, p


# --------------------------------------------------------------------------------------------------- 1. fallback arithmetic
@pytest.mark.parametrize("w", [0.1, 0.5, 2.0 ** -12, 1.0 - 0.9998])
def test_fallback_arithmetic_equals_numpy_float32_bit_for_bit(w):
    from monosowa_amd.ema import ema_fallback_
    rng = np.random.default_rng(23)
    e, p = special_operands(1000, rng)
    want = ema_reference(e, p, w)
    # the specials do what their names say
    k = len(SPECIAL)
    with np.errstate(all="ignore"):
        d = p[:k] - e[:k]
        t = np.float32(w) * d
    assert np.isnan(want).sum() >= 2 * 6 and np.isinf(d).sum() >= 4 and np.isinf(want[:k]).any()
    assert ((t != 0) & (np.abs(t) < np.float32(1.17549435e-38))).any(), "no subnormal t"
    assert ((d != 0) & (t == 0)).any(), "no w * d underflowing to zero"
    assert np.array_equal(want[:2].view(np.int32), e[:2].view(np.int32))                 # e == p: e stays
    avgs = [torch.from_numpy(e[:400].copy()), torch.from_numpy(e[400:].copy()).view(20, 30)]
    params = [torch.from_numpy(p[:400].copy()), torch.from_numpy(p[400:].copy()).view(20, 30)]
    ema_fallback_(avgs, params, np.float32(w))
    assert_same_bits(np.concatenate([a.numpy().reshape(-1) for a in avgs]), want)
    assert np.array_equal(np.concatenate([q.numpy().reshape(-1) for q in params]).view(np.int32), p.view(np.int32))     # p is read only

    class One(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.from_numpy(e.copy()))

    # ... and ModelEMA.update is that arithmetic with the schedule's w
    from monosowa_amd.ema import ModelEMA
    live = One()
    ema = ModelEMA(live, decay=1.0 - float(np.float32(w)), warmup=False)
    with torch.no_grad():
        live.a.copy_(torch.from_numpy(p))
    ema.update()
    assert_same_bits(ema.module.a.detach().numpy(), ema_reference(e, p, ema_weight_of(ema, 0)))
    assert ema.updates == 1 and not ema.module.training


def ema_weight_of(ema, t):
    d = min(ema.decay, (1 + t) / (10 + t)) if ema.warmup else ema.decay
    return np.float32(1.0 - d)


# --------------------------------------------------------------------------------------------------- 2. the schedule
def test_schedule_and_the_weight_the_update_receives(monkeypatch):
    from monosowa_amd import ema as E
    decay = 0.999
    want = {0: 1 / 10, 1: 2 / 11, 9: 10 / 19, 10: 11 / 20, 10000: 0.999}             # 10001 / 10010 = 0.99910...: the decay is the smaller
    for t, d in want.items():
        assert E.ema_decay_at(decay, t, True) == d
        assert E.ema_decay_at(decay, t, False) == decay
        w = E.ema_weight(decay, t, True)
        assert isinstance(w, np.float32) and w == np.float32(1.0 - d)
        assert E.ema_weight(decay, t, False) == np.float32(1.0 - decay)
    assert E.ema_decay_at(decay, 8980, True) == 8981 / 8990 < decay == E.ema_decay_at(decay, 9000, True)      # where the warm-up ends
    seen = []
    monkeypatch.setattr(E, "ema_fallback_", lambda avgs, params, w: seen.append(w))
    live = torch.nn.Linear(3, 2)
    for warmup in (True, False):
        ema = E.ModelEMA(live, decay, warmup=warmup)
        del seen[:]
        for t in sorted(want):
            ema.updates = t
            ema.update()
            assert ema.updates == t + 1
        assert [type(w) for w in seen] == [np.float32] * 5
        assert seen == [np.float32(1.0 - (want[t] if warmup else decay)) for t in sorted(want)]
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            E.ModelEMA(live, bad)


def test_entry_point_refuses_a_null_table_and_a_negative_count_and_takes_zero_chunks():
    """None of the three launches anything, so they are answered without a GPU."""
    import ctypes
    from monosowa_amd import pointwise
    lib = pointwise.load()
    table = (ctypes.c_ulonglong * 4)()
    assert lib.mono_ema_update_f32(table, 0, 0.1, None, None) == 0
    assert lib.mono_ema_update_f32(table, -1, 0.1, None, None) != 0
    assert lib.mono_ema_update_f32(None, 1, 0.1, None, None) != 0
    assert lib.mono_ema_update_f32(None, 0, 0.1, None, None) != 0


# --------------------------------------------------------------------------------------------------- 3. the key
def test_key_absent_none_or_zero_is_off_and_bad_values_raise(tmp_path, monkeypatch):
    from monosowa_amd.helpers.save_helper import get_checkpoint_state, save_checkpoint
    model, crit, opt = _build()
    loader = _Loader([])
    for cfg in ({}, {"ema_decay": None}, {"ema_decay": 0}, {"ema_decay": 0.0}):
        trainer = _trainer(model, crit, opt, loader, **cfg)
        assert trainer.ema is None
        state = trainer._checkpoint_state(0.0, 0)
        assert set(state) == CHECKPOINT_KEYS
    assert set(get_checkpoint_state(model, opt, 1, 0.0, 0)) == CHECKPOINT_KEYS
    save_checkpoint(trainer._checkpoint_state(0.0, 0), str(tmp_path / "off"))
    assert set(torch.load(str(tmp_path / "off.pth"), weights_only=False)) == CHECKPOINT_KEYS
    for bad in (1.0, -0.1, "x", 1, True, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _trainer(model, crit, opt, loader, ema_decay=bad)
    on = _trainer(model, crit, opt, loader, ema_decay=0.999)
    assert on.ema is not None and on.ema.decay == 0.999 and on.ema.warmup is True and on.ema.updates == 0
    assert set(on._checkpoint_state(0.0, 0)) == CHECKPOINT_KEYS | {"ema_state"}
    assert _trainer(model, crit, opt, loader, ema_decay=0.999, ema_warmup=False).ema.warmup is False


# --------------------------------------------------------------------------------------------------- 4. two steps on the Trainer
def _two_steps(decay=0.999, optimizer=None, **cfg):
    """A Trainer with the key on, two train steps on two batches; parameter snapshots before the first and after each step."""
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.helpers.trainer_helper import stage_batch
    model, crit, opt = _build()
    if optimizer:
        ycfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
        opt = build_optimizer(dict(ycfg["optimizer"], **optimizer), model)
    loader = _Loader([7, 8])
    state = _seed_hook(model)
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    trainer = _trainer(model, crit, opt, loader, ema_decay=decay, **cfg)
    trainer.model.train(), crit.train()
    snap = lambda: {n: p.detach().clone().numpy() for n, p in model.named_parameters()}
    snaps = [snap()]
    state["k"] = 0
    for raw in loader:
        trainer.train_step(*stage_batch(raw, trainer.device))
        snaps.append(snap())
    return trainer, model, crit, opt, loader, snaps, frozen, state


def test_two_trainer_steps_equal_the_replay_from_parameter_snapshots():
    trainer, model, crit, opt, loader, snaps, frozen, _ = _two_steps()
    ema = trainer.ema
    assert ema.updates == 2 and ema.module is not model and not ema.module.training and model.training
    assert len(frozen) >= 10, "the frozen stem / layer1 are expected among the parameters"
    tracked = ema.tracked()
    assert set(tracked) == {n for n, p in model.named_parameters() if p.requires_grad} and len(tracked) > 200
    moved = 0
    for n, e in tracked.items():
        want = ema_reference(snaps[0][n], snaps[1][n], np.float32(1.0 - 1 / 10))
        want = ema_reference(want, snaps[2][n], np.float32(1.0 - 2 / 11))
        assert_same_bits(e.detach().numpy(), want, n)
        moved += int(not np.array_equal(want, snaps[0][n]) and not np.array_equal(want, snaps[2][n]))
    assert moved > 200, "the average must differ from both the start and the live weights"
    # frozen parameters and buffers: copied, not averaged.  The live ones are edited here so that the copy is seen to happen.
    with torch.no_grad():
        dict(model.named_parameters())[frozen[0]].add_(1.0)
        name0, buf0 = next(iter(model.named_buffers()))
        buf0.add_(1.0)
    assert not torch.equal(dict(ema.module.named_parameters())[frozen[0]], dict(model.named_parameters())[frozen[0]])
    assert ema.sync_untracked() is ema.module
    mine = dict(ema.module.named_parameters())
    for n in frozen:
        assert torch.equal(mine[n], dict(model.named_parameters())[n]), n
    bufs = dict(ema.module.named_buffers())
    assert len(bufs) > 100
    for n, b in model.named_buffers():
        assert torch.equal(bufs[n], b), n
    for n, e in tracked.items():                                  # ... and the averaged tensors were left alone by it
        assert e.requires_grad and e is mine[n]


# --------------------------------------------------------------------------------------------------- 5. checkpoints
class _Logs(logging.Handler):
    def __init__(self):
        super().__init__()
        self.records = []

    def emit(self, record):
        self.records.append(record)


def _save(trainer, directory, name="checkpoint"):
    from monosowa_amd.helpers.save_helper import save_checkpoint
    os.makedirs(str(directory), exist_ok=True)
    trainer.epoch = 1
    save_checkpoint(trainer._checkpoint_state(0.0, 0), os.path.join(str(directory), name))
    return os.path.join(str(directory), name + ".pth")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Two steps with the key on, saved with and without the average."""
    from monosowa_amd.helpers.save_helper import get_checkpoint_state, save_checkpoint
    trainer, model, crit, opt, loader, snaps, frozen, _ = _two_steps()
    out = tmp_path_factory.mktemp("ema_ckpt")
    path = _save(trainer, out)
    save_checkpoint(get_checkpoint_state(model, opt, 1, 0.0, 0), str(out / "plain"))
    return trainer, path, str(out / "plain.pth"), str(out)


def test_saved_checkpoint_carries_the_average_beside_the_model(trained):
    trainer, path, plain, _ = trained
    ckpt = torch.load(path, weights_only=False)
    assert set(ckpt) == CHECKPOINT_KEYS | {"ema_state"}
    assert set(ckpt["ema_state"]) == {"module", "updates", "decay", "warmup"}
    assert ckpt["ema_state"]["updates"] == 2 and ckpt["ema_state"]["decay"] == 0.999 and ckpt["ema_state"]["warmup"] is True
    assert list(ckpt["ema_state"]["module"]) == list(ckpt["model_state"])
    assert set(torch.load(plain, weights_only=False)) == CHECKPOINT_KEYS
    differ = 0
    for n, e in trainer.ema.tracked().items():
        assert torch.equal(ckpt["ema_state"]["module"][n], e)
        differ += int(not torch.equal(ckpt["model_state"][n], e))
    assert differ > 200                                                  # (parameters that never get a gradient do not move)


def test_resume_restores_the_average_and_its_count(trained, monkeypatch):
    """save -> a fresh Trainer with ``resume_model`` (other initial weights, another configured decay): the file's state wins."""
    trainer, path, _, out = trained
    _save(trainer, os.path.join(out, "run", "tiny"))                     # where a Trainer with save_path "run" named "tiny" looks
    monkeypatch.chdir(out)
    model, crit, opt = _build(seed=6)
    sched = type("S", (), {"last_epoch": 0})()
    from monosowa_amd.helpers.trainer_helper import Trainer
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fresh = Trainer({"save_path": "run", "max_epoch": 1, "ema_decay": 0.5, "resume_model": True}, model, opt, _Loader([]), None, sched,
                    None, logging.getLogger("test_ema"), crit, "tiny")
    assert sched.last_epoch == 0
    assert fresh.epoch == 1 and fresh.ema.updates == 2 and fresh.ema.decay == 0.999 and fresh.ema.warmup is True
    want, got = trainer.ema.module.state_dict(), fresh.ema.module.state_dict()
    assert list(want) == list(got)
    for n in want:
        assert torch.equal(want[n], got[n]), n
    live = dict(model.named_parameters())
    for n, p in trainer.model.named_parameters():
        assert torch.equal(live[n], p), n
    assert fresh.ema.source is model and fresh.ema.module is not model


def test_checkpoint_without_the_key_starts_the_average_from_the_loaded_weights_with_one_warning(trained):
    from monosowa_amd.ema import ModelEMA
    from monosowa_amd.helpers.save_helper import load_checkpoint
    trainer, path, plain, _ = trained
    model, _, _ = _build(seed=5)
    ema = ModelEMA(model, 0.999)
    ema.updates = 7
    addresses = [e.data_ptr() for e in ema.module.parameters()]
    logger, logs = logging.getLogger("test_ema.absent"), _Logs()
    logger.addHandler(logs)
    try:
        load_checkpoint(model=model, optimizer=None, filename=plain, map_location="cpu", logger=logger, ema=ema)
    finally:
        logger.removeHandler(logs)
    warnings_ = [r for r in logs.records if r.levelno == logging.WARNING]
    assert len(warnings_) == 1 and "ema_state" in warnings_[0].getMessage() and plain in warnings_[0].getMessage()
    assert ema.updates == 0
    saved = dict(trainer.model.named_parameters())
    for n, e in ema.module.named_parameters():
        assert torch.equal(e, saved[n]) and torch.equal(dict(model.named_parameters())[n], saved[n]), n
    assert addresses == [e.data_ptr() for e in ema.module.parameters()]               # in place: a chunk table would survive
    # with the key present nothing is logged as a warning and the state is the file's
    logs2 = _Logs()
    logger.addHandler(logs2)
    try:
        load_checkpoint(model=model, optimizer=None, filename=path, map_location="cpu", logger=logger, ema=ema)
    finally:
        logger.removeHandler(logs2)
    assert not [r for r in logs2.records if r.levelno >= logging.WARNING] and ema.updates == 2
    assert addresses == [e.data_ptr() for e in ema.module.parameters()]


def _assert_holds_the_average(model, trainer):
    avg, live = dict(trainer.ema.module.named_parameters()), dict(trainer.model.named_parameters())
    differ = 0
    for n, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), avg[n]), n
        differ += int(not torch.equal(avg[n], live[n]))
    assert differ > 200
    bufs = dict(trainer.ema.module.named_buffers())
    for n, b in model.named_buffers():
        assert torch.equal(b.cpu(), bufs[n]), n


def test_load_checkpoint_weights_ema_puts_the_average_into_the_model(trained):
    from monosowa_amd.helpers.save_helper import load_checkpoint
    trainer, path, plain, _ = trained
    model, _, opt = _build(seed=5)
    assert load_checkpoint(model=model, optimizer=opt, filename=path, map_location="cpu", weights="ema") == (1, 0.0, 0)
    _assert_holds_the_average(model, trainer)
    model2, _, _ = _build(seed=5)
    load_checkpoint(model=model2, optimizer=None, filename=path, map_location="cpu")               # the default is the live weights
    for n, p in trainer.model.named_parameters():
        assert torch.equal(dict(model2.named_parameters())[n], p), n
    with pytest.raises(KeyError) as e:
        load_checkpoint(model=model2, optimizer=None, filename=plain, map_location="cpu", weights="ema")
    assert plain in str(e.value) and "ema_state" in str(e.value)
    with pytest.raises(ValueError):
        load_checkpoint(model=model2, optimizer=None, filename=path, map_location="cpu", weights="best")


def _detector_cfg():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    dataset = {k: v for k, v in cfg["dataset"].items() if k != "root_dir"}
    return {"dataset": dataset, "tester": {"topk": 50, "threshold": 0.2},
            "model": dict(cfg["model"], depth_map_size=(12, 4), dropout=0.0)}


def test_detector_loads_the_average_on_the_cpu_path(trained):
    from monosowa_amd import Detector
    trainer, path, plain, _ = trained
    det = Detector(_detector_cfg(), checkpoint=path, weights="ema", device="cpu")
    _assert_holds_the_average(det.model, trainer)
    for weights in (None, "model"):
        other = Detector(_detector_cfg(), checkpoint=path, device="cpu", **({} if weights is None else {"weights": weights}))
        for n, p in trainer.model.named_parameters():
            assert torch.equal(dict(other.model.named_parameters())[n], p), n
    with pytest.raises(KeyError):
        Detector(_detector_cfg(), checkpoint=plain, weights="ema", device="cpu")
    with pytest.raises(ValueError, match="weights"):
        Detector(_detector_cfg(), model=trainer.model, weights="ema", device="cpu")
    with pytest.raises(ValueError, match="weights"):
        Detector(_detector_cfg(), checkpoint=path, weights="best", device="cpu")


class _DL:
    class dataset:
        max_objs, class_name = 50, ["Pedestrian", "Car", "Cyclist"]


def test_tester_weights_key_selects_what_test_loads(trained, tmp_path, monkeypatch):
    import shutil
    from monosowa_amd.helpers.tester_helper import Tester
    trainer, path, plain, _ = trained
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    out = tmp_path / "run" / "m"
    os.makedirs(str(out))
    shutil.copy(path, str(out / "checkpoint_epoch_1.pth"))
    for mode in ("single", "all"):
        for weights in ("ema", "model", None):
            model, _, _ = _build(seed=5)
            cfg = {"type": "KITTI", "topk": 50, "mode": mode, "checkpoint": 1}
            if weights is not None:
                cfg["weights"] = weights
            tester = Tester(cfg, model, _DL(), logging.getLogger("test_ema"), {"save_path": str(tmp_path / "run") + "/"}, "m")
            tester.output_dir = str(out)
            assert tester.weights == (weights or "model")
            ran = []
            tester.inference = lambda: ran.append("inference")
            tester.evaluate = lambda: 0.5
            assert tester.test() == 0.5 and ran == ["inference"]
            if weights == "ema":
                _assert_holds_the_average(model, trainer)
            else:
                for n, p in trainer.model.named_parameters():
                    assert torch.equal(dict(model.named_parameters())[n], p), n
    with pytest.raises(ValueError, match="weights"):
        Tester({"type": "KITTI", "topk": 50, "weights": "best"}, model, _DL(), logging.getLogger("test_ema"), {"save_path": "x/"}, "m")


# --------------------------------------------------------------------------------------------------- 6. host-path skip
def test_host_path_skip_leaves_parameters_moments_and_average_alone():
    from monosowa_amd.helpers.trainer_helper import stage_batch
    trainer, model, crit, opt, loader, snaps, frozen, state = _two_steps(optimizer={"skip_nonfinite": True})
    assert opt.guard_enabled and opt._guard is None and opt.guard_report()["skipped_total"] == 0
    assert opt.last_step_skipped() is False and opt.guard_record_address() is None
    ema = trainer.ema
    assert ema.updates == 2

    def bits():
        out = {"p." + n: p.detach().clone() for n, p in model.named_parameters()}
        out.update({"e." + n: p.detach().clone() for n, p in ema.module.named_parameters()})
        for n, p in model.named_parameters():
            for key in ("exp_avg", "exp_avg_sq"):
                if key in opt.state.get(p, {}):
                    out[key + "." + n] = opt.state[p][key].clone()
        return out
    before = bits()
    assert sum(k.startswith("exp_avg_sq.") for k in before) > 200
    name, poisoned = next((n, p) for n, p in model.named_parameters() if p.requires_grad and p.numel() > 8)
    handle = poisoned.register_hook(lambda g: g * float("nan"))
    state["k"] = 0
    trainer.train_step(*stage_batch(loader.batches[0], trainer.device))
    handle.remove()
    assert torch.isnan(poisoned.grad).all()
    assert opt.last_step_skipped() is True and opt.guard_report()["skipped_total"] == 1
    after = bits()
    assert set(after) == set(before)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert ema.updates == 3                                              # t advances on a skipped step too
    state["k"] = 1
    trainer.train_step(*stage_batch(loader.batches[1], trainer.device))       # the next clean step moves all three
    assert opt.last_step_skipped() is False and opt.guard_report()["skipped_total"] == 1 and ema.updates == 4
    moved = bits()
    w = np.float32(1.0 - 4 / 13)                                         # t = 3
    for n, e in ema.tracked().items():
        assert_same_bits(moved["e." + n].numpy(), ema_reference(before["e." + n].numpy(), moved["p." + n].numpy(), w), n)
    assert sum(not torch.equal(before["e." + n], moved["e." + n]) for n in ema.tracked()) > 200
