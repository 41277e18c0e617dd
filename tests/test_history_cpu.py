"""``trainer.history`` without a GPU: the float64 fallback of ``StepHistory`` against numpy on a small ``nn`` model, the key's validation,
the JSON encoding of non-finite values, a capacity overflow, ``history.jsonl`` over a fresh and a resumed run, the entry point's return
codes (none of them launches anything) and two gloo ranks.

Tolerance of a sum of squares: n non-negative doubles added in any order lie within n * 2^-53 of the exact sum, relative (every partial
sum is rounded once, 2^-53 relative, and all terms have one sign); the products of float32 values are exact in float64.  A norm is
the square root of that: half the relative error plus the root's own rounding, so n * 2^-53 bounds it too (n >= 1)."""
import ctypes
import json
import logging
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_accumulation_cpu import _Loader, _process_state, _seed_hook, _spawn, _trainer      # noqa: F401  (_process_state: autouse fixture)
from test_distributed_gloo import _build
from test_ema_cpu import CHECKPOINT_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


class _Net(torch.nn.Module):
    """Six default groups in ``named_parameters`` order: level_embed (a module's own parameters come first), backbone.layer1, backbone.layer2, depthaware_transformer.encoder, depthaware_transformer.decoder, head."""

    def __init__(self):
        super().__init__()
        body = torch.nn.ModuleDict({"layer1": torch.nn.Linear(6, 5), "layer2": torch.nn.Linear(5, 37)})
        self.backbone = torch.nn.Sequential(torch.nn.ModuleDict({"body": body}))
        self.depthaware_transformer = torch.nn.ModuleDict({"encoder": torch.nn.Linear(37, 301), "decoder": torch.nn.Linear(301, 4)})
        self.head = torch.nn.Linear(4, 1)
        self.level_embed = torch.nn.Parameter(torch.ones(3))            # never gets a gradient: its group reports zeros

    def forward(self, x):
        b = self.backbone[0]["body"]
        t = self.depthaware_transformer
        return self.head(t["decoder"](torch.tanh(t["encoder"](torch.tanh(b["layer2"](b["layer1"](x)))))))


GROUPS = ["level_embed", "backbone.layer1", "backbone.layer2", "depthaware_transformer.encoder", "depthaware_transformer.decoder", "head"]


def _reference(model):
    """{group: (sum g^2, sum p^2, non-finite g, elements)} in numpy float64 over the parameters that have a gradient."""
    from monosowa_amd.history import default_group
    out = {g: [0.0, 0.0, 0, 0] for g in GROUPS}
    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        g64, p64 = p.grad.numpy().astype(np.float64), p.detach().numpy().astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            r = out[default_group(name)]
            r[0] += float((g64 * g64).sum())
            r[1] += float((p64 * p64).sum())
        r[2] += int((~np.isfinite(g64)).sum())
        r[3] += g64.size
    return out


def _close(got, want, n):
    return abs(got - want) <= 2 * n * U * abs(want)          # both sides carry an n * 2^-53 error against the exact value


# --------------------------------------------------------------------------------------------------- 1. the fallback against numpy
def test_default_groups_and_the_group_limit():
    from monosowa_amd import StepHistory
    from monosowa_amd.history import default_group
    assert default_group("backbone.0.body.layer3.5.conv2.weight") == "backbone.layer3"
    assert default_group("backbone.0.body.conv1.weight") == "backbone"
    assert default_group("depthaware_transformer.decoder.layers.0.norm1.bias") == "depthaware_transformer.decoder"
    assert default_group("depthaware_transformer.level_embed") == "depthaware_transformer"
    assert default_group("class_embed.0.weight") == "class_embed" and default_group("query_embed") == "query_embed"
    net = _Net()
    assert StepHistory(net, {}, 1).groups == GROUPS
    assert StepHistory(net, {}, 1, group_of=lambda name: "all").groups == ["all"]
    wide = torch.nn.Sequential(*[torch.nn.Linear(1, 1) for _ in range(65)])
    with pytest.raises(ValueError, match="64"):
        StepHistory(wide, {}, 1)
    assert len(StepHistory(torch.nn.Sequential(*list(wide)[:64]), {}, 1).groups) == 64
    with pytest.raises(ValueError):
        StepHistory(net, {}, 0)


def test_fallback_columns_equal_numpy_float64_and_non_finite_values_are_counted_per_group():
    from monosowa_amd import StepHistory
    from monosowa_amd.helpers.optimizer_helper import AdamW
    torch.manual_seed(3)
    net = _Net()
    opt = AdamW(net.parameters(), lr=1e-2, clip_max_norm=10.0, skip_nonfinite=True)
    weight_dict = {"loss_b": 2.0, "loss_a": 0.5, "loss_missing": 1.0}
    hist = StepHistory(net, weight_dict, capacity=4)
    assert hist.ring is None
    rows_want = []
    for step, poison in enumerate((None, "nan", "inf")):
        opt.zero_grad(set_to_none=True)
        y = net(torch.randn(8, 6))
        loss_dict = {"loss_a": (y ** 2).mean(), "class_error": y.mean().detach(), "loss_b": y.abs().mean()}
        total = loss_dict["loss_a"] * 0.5 + loss_dict["loss_b"] * 2.0
        total.backward()
        if poison == "nan":
            net.depthaware_transformer["encoder"].weight.grad[300, 36] = float("nan")
            net.head.bias.grad[0] = float("-inf")
        if poison == "inf":
            net.backbone[0]["body"]["layer2"].bias.grad[[0, 36]] = float("inf")
        hist.add_losses(loss_dict, total)
        opt.step()
        assert opt.last_fused_plans() is None                      # CPU tensors: the foreach path
        hist.commit(opt, epoch=2, step=step, lr=opt.param_groups[0]["lr"], micro_batches=1)
        rows_want.append((_reference(net), {k: float(loss_dict[k].detach().double()) for k in ("loss_b", "loss_a")},
                          float(total.detach().double())))
    assert hist.loss_keys == ["loss_b", "loss_a"] and hist.ring.shape == (4, 3 + 3 * 6 + 3) and hist.ring.dtype == torch.float64
    assert hist.kernel_commits == 0
    rows = hist.drain()
    assert len(rows) == 3 and not hist.ring.any() and hist.drain() == []
    for step, (row, (want, losses, total)) in enumerate(zip(rows, rows_want)):
        assert (row["epoch"], row["step"], row["lr"], row["micro_batches"]) == (2, step, 1e-2, 1)
        assert row["losses"] == losses and list(row["losses"]) == ["loss_b", "loss_a"] and row["loss_detr"] == total      # exactly float64(term)
        assert "guard" not in row                                   # no device-side guard in these steps
        assert list(row["grad_norm"]) == list(row["param_norm"]) == list(row["grad_nonfinite"]) == GROUPS
        for g, (gs, ps, bad, n) in want.items():
            assert row["grad_nonfinite"][g] == bad, (step, g)
            assert _close(row["param_norm"][g], math.sqrt(ps), n), (step, g)
            if math.isnan(gs):
                assert math.isnan(row["grad_norm"][g]), (step, g)
            elif math.isinf(gs):
                assert row["grad_norm"][g] == math.inf, (step, g)
            else:
                assert _close(row["grad_norm"][g], math.sqrt(gs), max(n, 1)), (step, g)
        assert row["grad_norm"]["level_embed"] == 0.0 and row["param_norm"]["level_embed"] == 0.0
    assert [sum(r["grad_nonfinite"].values()) for r in rows] == [0, 2, 2]
    assert rows[1]["grad_nonfinite"]["depthaware_transformer.encoder"] == 1 and rows[1]["grad_nonfinite"]["head"] == 1
    assert math.isnan(rows[1]["grad_norm"]["depthaware_transformer.encoder"]) and rows[1]["grad_norm"]["head"] == math.inf
    assert rows[2]["grad_nonfinite"]["backbone.layer2"] == 2 and rows[2]["grad_norm"]["backbone.layer2"] == math.inf
    # the guard's host path skipped steps 1 and 2: param_norm is what it was after step 0
    assert rows[1]["param_norm"] == rows[0]["param_norm"] == rows[2]["param_norm"]


def test_accumulated_losses_scale_the_terms_and_take_the_total_as_it_is_and_a_changed_key_set_raises():
    from monosowa_amd import StepHistory
    net = _Net()
    hist = StepHistory(net, {"loss_a": 1.0, "loss_b": 3.0}, capacity=2)
    a = [torch.tensor(0.1), torch.tensor(0.7), torch.tensor(1.3)]
    b = [torch.tensor(2.5), torch.tensor(1e-3), torch.tensor(4.0)]
    K = 3
    for k in range(K):
        total = (a[k] + 3.0 * b[k]) / K                            # Trainer.train_cycle: the total carries its 1 / K
        hist.add_losses({"loss_a": a[k], "loss_b": b[k], "cardinality_error": torch.tensor(1.0)}, total, scale=1.0 / K)
    with pytest.raises(ValueError, match="loss_c"):
        hist.add_losses({"loss_a": a[0], "loss_b": b[0], "cardinality_error": a[0], "loss_c": a[0]}, a[0])
    with pytest.raises(ValueError, match="loss_b"):
        hist.add_losses({"loss_a": a[0], "cardinality_error": a[0]}, a[0])
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    hist.commit(opt, epoch=0, step=0, lr=0.1, micro_batches=K)
    row, = hist.drain()
    for key, terms in (("loss_a", a), ("loss_b", b)):
        want = sum(float(t.double()) for t in terms) / K
        assert abs(row["losses"][key] - want) <= 4 * np.spacing(want), key
    want = sum(float(((x + 3.0 * y) / K).double()) for x, y in zip(a, b))
    assert abs(row["loss_detr"] - want) <= 4 * np.spacing(want)
    assert row["micro_batches"] == K and all(v == 0 for v in row["grad_norm"].values())      # sgd without gradients: zeros


# --------------------------------------------------------------------------------------------------- 2. the key
def test_key_absent_none_or_false_is_off_and_anything_but_a_bool_raises():
    model, crit, opt = _build()
    loader = _Loader([])
    for cfg in ({}, {"history": None}, {"history": False}):
        trainer = _trainer(model, crit, opt, loader, **cfg)
        assert trainer.history is None
        assert set(trainer._checkpoint_state(0.0, 0)) == CHECKPOINT_KEYS
    for bad in (1, 0, "true", "yes", 1.0, [], {}):
        with pytest.raises(ValueError, match="history"):
            _trainer(model, crit, opt, loader, history=bad)
    on = _trainer(model, crit, opt, _Loader([7, 8, 9]), history=True, global_batch=4)
    assert on.history is not None and on.history.capacity == 2 and on.history.ring is None
    assert set(on._checkpoint_state(0.0, 0)) == CHECKPOINT_KEYS
    assert "backbone.layer2" in on.history.groups and "depthaware_transformer.decoder" in on.history.groups
    assert 5 < len(on.history.groups) <= 64


# --------------------------------------------------------------------------------------------------- 3. JSON
def test_non_finite_numbers_are_written_as_strings_and_every_line_is_valid_json():
    from monosowa_amd.history import to_json
    row = {"epoch": 0, "lr": 2e-4, "loss_detr": float("nan"), "losses": {"a": float("inf"), "b": np.float64("-inf"), "c": 1.5},
           "grad_nonfinite": {"g": np.int64(3)}, "guard": {"norm": float("inf"), "coef": 0.0, "skip": 1}, "l": [float("nan"), 2]}
    line = to_json(row)
    assert "NaN" not in line and "Infinity" not in line and "\n" not in line

    def strict(name):
        raise AssertionError("not valid JSON: " + name)
    back = json.loads(line, parse_constant=strict)
    assert back == {"epoch": 0, "lr": 2e-4, "loss_detr": "nan", "losses": {"a": "inf", "b": "-inf", "c": 1.5}, "grad_nonfinite": {"g": 3},
                    "guard": {"norm": "inf", "coef": 0.0, "skip": 1}, "l": ["nan", 2]}
    assert float(back["loss_detr"]) != float(back["loss_detr"]) and float(back["losses"]["b"]) == -math.inf


# --------------------------------------------------------------------------------------------------- 4. overflow
def test_commit_on_a_full_ring_drains_into_the_backlog_and_no_row_is_lost():
    from monosowa_amd import StepHistory
    net = _Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    hist = StepHistory(net, {"loss_a": 1.0}, capacity=2)
    for step in range(5):
        opt.zero_grad(set_to_none=True)
        loss = (net(torch.full((2, 6), float(step))) ** 2).mean()
        loss.backward()
        hist.add_losses({"loss_a": loss}, loss * 1.0)
        opt.step()
        hist.commit(opt, epoch=1, step=step, lr=0.1, micro_batches=1)
        assert len(hist._meta) <= 2 and len(hist._backlog) == (step // 2) * 2
    rows = hist.drain()
    assert [r["step"] for r in rows] == [0, 1, 2, 3, 4] and len({r["loss_detr"] for r in rows}) == 5
    assert all(r["losses"]["loss_a"] == r["loss_detr"] and r["grad_norm"]["head"] > 0 for r in rows)
    assert hist.drain() == [] and not hist.ring.any()


# --------------------------------------------------------------------------------------------------- 5. the file
class _Logs(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _lines(path):
    return [json.loads(l, parse_constant=lambda name: pytest.fail("not valid JSON: " + name)) for l in open(path).read().splitlines()]


def test_a_fresh_run_truncates_history_jsonl_and_a_resumed_one_appends(tmp_path, monkeypatch):
    from monosowa_amd.helpers.save_helper import save_checkpoint
    from monosowa_amd.helpers.trainer_helper import Trainer
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    model, crit, opt = _build()
    _seed_hook(model)
    loader = _Loader([7, 8])
    sched = type("S", (), {"last_epoch": 0, "step": lambda self: None})()
    logger = logging.getLogger("test_history")
    logs = _Logs()
    logger.addHandler(logs)
    logger.setLevel(logging.INFO)
    try:
        def trainer(**cfg):
            t = Trainer(dict({"save_path": "run", "max_epoch": 1, "save_frequency": 1, "save_all": 0, "history": True}, **cfg), model, opt,
                        loader, None, sched, None, logger, crit, "tiny")
            t.log_interval = 10 ** 9
            model.train(), crit.train()
            return t
        path = os.path.join("run", "tiny", "history.jsonl")
        os.makedirs(os.path.dirname(path))
        open(path, "w").write("stale line of an earlier run\n")
        first = trainer()
        first.train()
        rows = _lines(path)
        assert [(r["epoch"], r["step"], r["micro_batches"]) for r in rows] == [(0, 0, 1), (0, 1, 1)]
        assert set(torch.load(os.path.join("run", "tiny", "checkpoint.pth"), weights_only=False)) == CHECKPOINT_KEYS
        assert set(rows[0]) == {"epoch", "step", "lr", "micro_batches", "losses", "loss_detr", "grad_norm", "param_norm", "grad_nonfinite"}
        weight_dict = crit.weight_dict
        assert list(rows[0]["losses"]) == [k for k in weight_dict if k in rows[0]["losses"]] and len(rows[0]["losses"]) > 20
        want = sum(rows[0]["losses"][k] * weight_dict[k] for k in rows[0]["losses"])
        assert abs(rows[0]["loss_detr"] - want) <= 1e-5 * abs(want)          # the float32 total against the float64 recombination
        assert any(l.startswith("Epoch 0: mean over 2 of 2 steps: loss_detr: ") and "loss_ce: " in l for l in logs.lines)
        assert any(l.startswith("Epoch 0: grad_norm median: ") and "max: " in l for l in logs.lines)
        assert not any("non-finite" in l for l in logs.lines)
        second = trainer(max_epoch=2, resume_model=True)
        assert second.epoch == 1
        second.train()
        rows = _lines(path)
        assert [(r["epoch"], r["step"]) for r in rows] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        third = trainer()                                       # no resume_model: the file starts over
        third.train()
        assert [(r["epoch"], r["step"]) for r in _lines(path)] == [(0, 0), (0, 1)]
    finally:
        logger.removeHandler(logs)


# --------------------------------------------------------------------------------------------------- 6. return codes
def test_entry_point_refuses_null_arguments_and_bad_counts_and_takes_zero_chunks():
    """None of these launches anything, so they are answered without a GPU."""
    from monosowa_amd import pointwise
    lib = pointwise.load()
    V, I = ctypes.c_void_p, ctypes.c_int
    buf = (ctypes.c_double * 16)()
    buf[:] = [7.0] * 16
    tables, groups = (V * 8)(*[ctypes.addressof(buf)] * 8), (V * 8)(*[ctypes.addressof(buf)] * 8)
    zero = (I * 8)(*[0] * 8)
    call = lambda t=tables, n=zero, g=groups, nt=2, ng=6, p=buf, o=buf: lib.mono_step_stats_f32(t, n, g, nt, ng, None, p, o, None)
    assert call() == 0 and list(buf) == [7.0] * 16                    # zero chunks: nothing launched, the caller's row stands
    assert call(nt=8, ng=64) == 0 and call(nt=1, ng=1) == 0
    for kw in ({"t": None}, {"n": None}, {"g": None}, {"p": None}, {"o": None}):
        assert call(**kw) == -1, kw
    for kw in ({"nt": 0}, {"nt": 9}, {"nt": -1}, {"ng": 0}, {"ng": 65}, {"n": (I * 8)(0, -1)}):
        assert call(**kw) == -2, kw
    assert call(t=(V * 8)(), n=(I * 8)(1, 0)) == -1 and call(g=(V * 8)(), n=(I * 8)(0, 1)) == -1      # chunks, but no table / group array
    assert list(buf) == [7.0] * 16


# --------------------------------------------------------------------------------------------------- 7. two ranks
def _rank_worker(rank, world, port, path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = os.path.join(os.path.dirname(path), "rank%d" % rank)
    os.makedirs(out)
    os.chdir(out)
    model, crit, opt = _build()
    loader = _Loader([7 + rank])
    state = _seed_hook(model)
    trainer = _trainer(model, crit, opt, loader, history=True)
    assert isinstance(trainer.model, torch.nn.parallel.DistributedDataParallel)
    trainer.log_interval = 10 ** 9
    seen = []
    forward = crit.forward

    def spy(*a, **k):
        ld = forward(*a, **k)
        seen.append(torch.stack([ld[key].detach().double() for key in crit.weight_dict if key in ld]))
        return ld
    crit.forward = spy
    reduces = []
    all_reduce = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (reduces.append(t.dtype), all_reduce(t, *a, **k))[1]
    state["k"] = rank
    trainer.train_one_epoch(0)
    dist.all_reduce = all_reduce
    assert len(seen) == 1 and reduces.count(torch.float64) == 1          # ONE all-reduce of the ring
    both = [torch.zeros_like(seen[0]) for _ in range(world)]
    dist.all_gather(both, seen[0])
    mean = ((both[0] + both[1]) / world).tolist()
    written = os.path.exists(os.path.join(out, "outputs", "tiny", "history.jsonl"))
    flags = [torch.zeros(1) for _ in range(world)]
    dist.all_gather(flags, torch.tensor([float(written)]))
    assert [bool(f) for f in flags] == [True, False]                    # rank 0 alone writes
    if rank == 0:
        row, = [json.loads(l) for l in open(os.path.join(out, "outputs", "tiny", "history.jsonl"))]
        got = list(row["losses"].values())
        assert len(got) == len(mean) > 20 and both[0].tolist() != both[1].tolist()
        assert all(abs(g - m) <= 2 * np.spacing(abs(m)) for g, m in zip(got, mean)), (got, mean)
        assert row["grad_norm"]["class_embed"] > 0 and row["grad_nonfinite"]["class_embed"] == 0
        torch.save("ok", path)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_average_the_loss_columns_and_rank_0_alone_writes_the_file(tmp_path):
    assert _spawn(_rank_worker, tmp_path / "ranks.pt") == "ok"
