"""bench.py's options around the headline: a plain run drops every extra leg (--full brings them back), --dump-outputs writes
the last timed step's results, and the pre-heat's state restore.  The CPU tests drive bench.py's own functions on a small
model; the GPU test runs the plain benchmark end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

LEGS = ("no_cpu_baseline", "no_inference_leg", "no_dataloader_leg", "no_step_roofline", "no_offsets_probe")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_drops_the_extra_legs_and_full_keeps_them(monkeypatch):
    plain = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert plain.steps == 7 and plain.warmup == 2 and not plain.full and plain.dump_outputs == ""
    assert all(getattr(plain, k) for k in LEGS)
    full = _parse(monkeypatch, "--steps", "7", "--full")
    assert full.full and not any(getattr(full, k) for k in LEGS)
    some = _parse(monkeypatch, "--full", "--no-cpu-baseline")
    assert some.no_cpu_baseline and not some.no_inference_leg


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(8, 4)
        self.head = torch.nn.Linear(4, 2)
        self.unused = torch.nn.Linear(2, 2)
        self.register_buffer("count", torch.zeros(1))

    def forward(self, x):
        self.count += 1
        h = torch.nn.functional.dropout(self.lin(x).relu(), 0.5, self.training)
        return {"pred": self.head(h), "aux_outputs": [{"pred": h}]}


def _setup():
    from monosowa_amd.helpers.optimizer_helper import AdamW
    torch.manual_seed(0)
    model = _Tiny()
    opt = AdamW([{"params": list(model.parameters()), "weight_decay": 1e-4}], lr=1e-2)
    x = torch.randn(16, 8)
    keep = {}

    def step():
        opt.zero_grad(set_to_none=True)
        out = model(x)
        losses = {"loss_a": out["pred"].square().mean(), "loss_b": out["aux_outputs"][0]["pred"].abs().mean()}
        total = losses["loss_a"] + losses["loss_b"]
        total.backward()
        opt.step()
        keep.update(loss=total, losses=losses, outputs=out)
    return model, opt, step, keep


def test_step_state_restore_returns_to_the_initial_state_whatever_ran_before():
    """After a restore the next steps compute what a freshly built model and optimizer compute, bit for bit, however many steps
    ran since the snapshot (the pre-heat runs for a time; --dump-outputs restores once more before the last timed step)."""
    from monosowa_amd import flash_attn, pointwise
    results = []
    for steps_before in (0, 1, 4):
        model, opt, step, keep = _setup()
        counters = flash_attn._seed_counter[0], pointwise._seed_counter[0]
        restore = bench.step_state(model, opt, torch.device("cpu"))
        for _ in range(steps_before):
            step()
        flash_attn._seed_counter[0] += 3               # what the HIP dropout kernels would have drawn
        pointwise._seed_counter[0] += 5
        restore()
        assert (flash_attn._seed_counter[0], pointwise._seed_counter[0]) == counters
        assert all(int(st["step"]) == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())
        step()
        step()
        results.append([p.detach().clone() for p in model.parameters()] + [model.count.clone(), keep["loss"].detach().clone()])
    assert all(torch.equal(a, b) for r in results[1:] for a, b in zip(results[0], r))


def test_timed_steps_runs_before_last_once_right_before_the_last_step():
    calls = []
    elapsed = bench.timed_steps(lambda b: calls.append("step"), None, 4, torch.device("cpu"), lambda: calls.append("restore"))
    assert elapsed >= 0 and calls == ["step", "step", "step", "restore", "step"]
    calls.clear()
    bench.timed_steps(lambda b: calls.append("step"), None, 2, torch.device("cpu"))
    assert calls == ["step", "step"]


def test_dump_outputs_writes_the_last_steps_results(tmp_path, monkeypatch):
    model, opt, step, keep = _setup()
    step()
    step()
    big = torch.arange(bench.DUMP_MAX_FULL + 5, dtype=torch.float32)
    keep["outputs"] = dict(keep["outputs"], big=big, idx=torch.arange(3), f64=torch.ones(2, dtype=torch.float64))
    bench.dump_outputs(str(tmp_path / "a"), keep, model, train=True)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(["loss.npy", "losses.loss_a.npy", "losses.loss_b.npy", "outputs.pred.npy", "outputs.aux_outputs.0.pred.npy",
                            "outputs.big.sample.npy", "outputs.idx.npy", "outputs.f64.npy", "params.npy", "grads.npy"])
    load = lambda name: np.load(tmp_path / "a" / (name + ".npy"))
    assert load("loss").dtype == np.float32 and load("loss").shape == () and load("loss").item() == keep["loss"].item()
    assert np.array_equal(load("outputs.pred"), keep["outputs"]["pred"].detach().numpy())
    assert load("outputs.idx").dtype == np.float64 and load("outputs.f64").dtype == np.float64
    params = list(model.parameters())
    assert np.array_equal(load("params"), torch.cat([p.detach().reshape(-1) for p in params]).numpy())
    grads = load("grads")
    n_lin = sum(p.numel() for p in params[:4])
    assert np.array_equal(grads[:n_lin], torch.cat([p.grad.reshape(-1) for p in params[:4]]).numpy())
    assert not grads[n_lin:].any()                      # the unused layer has no gradient: zeros
    sample = load("outputs.big.sample")
    assert sample.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(sample) >= 0) and sample.max() <= bench.DUMP_MAX_FULL + 4
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BUDGET_BYTES
    bench.dump_outputs(str(tmp_path / "b"), keep, model, train=True)
    assert np.array_equal(np.load(tmp_path / "b" / "outputs.big.sample.npy"), sample)      # fixed positions
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), keep, model, train=True)


@pytest.mark.gpu
def test_plain_bench_times_exactly_the_steps_asked_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run prints the headline line only (no extra legs) with ms_per_step of the K timed steps; two runs with the same
    arguments but pre-heats of different length dump the same results of the last timed step, which starts from the initial
    state.  Up to rounding only: the MSDA backward's float atomics sum in a different order every run."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MONOSOWA_BENCH_FORCE_LAUNCH"):
        env.pop(k, None)
    lines = []
    for run, preheat in (("a", "1"), ("b", "2")):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--preheat-seconds", preheat,
               "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "img/s"
        assert abs(line["value"] - 16 * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]
        assert line["dtype"] == "f32" and line["higher_is_better"] is True and line["roofline"] is None
        assert not {"cpu_baseline", "inference", "dataloader"} & set(line)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "params.sample.npy", "grads.sample.npy", "outputs.pred_logits.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= bench.DUMP_BUDGET_BYTES
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, f
        assert np.isfinite(a).all() and np.isfinite(b).all(), f
        a, b = a.astype(np.float64), b.astype(np.float64)
        rel = np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-30)
        assert rel <= (1e-3 if f.startswith("grads") else 1e-4), (f, rel)
    loss = [float(np.load(tmp_path / run / "loss.npy")) for run in "ab"]
    assert abs(loss[0] - loss[1]) <= 1e-5 * abs(loss[0]), loss
