"""Cost of the per-step training record (``trainer.history``), measured inside ONE process (the method of tools/ema_ab.py):

1. the train step of the shipped model at the benchmark shape (batch 16, 1280 x 384), steps alternating between the key off (no
   ``StepHistory`` call at all) and on (``add_losses`` in front of the optimizer step, the two launches of ``mono_step_stats_f32`` behind
   it).  Every step is timed with a device sync; median and min-max per setting.  The device launches of one ``add_losses`` call are
   counted under the profiler.
2. the device time of the ``mono_step_stats_f32`` pair -- 8 bytes per element: two loads, next to no stores -- and of
   ``mono_grad_accumulate_f32`` -- 12 bytes per element: two loads, one store -- over the same tensors: the parameters and gradients the
   optimizer's own chunk tables of the last step point at (the accumulate table is made of their p, g and n columns), rounds alternating
   between the two: device events around ``--reps`` back-to-back launches, divided by the number of launches.  The accumulate launches
   add the gradients INTO the parameters, so this part runs last.

    python tools/history_ab.py [--steps 40] [--rounds 15] [--reps 20] [--only-kernels] [--out profiles/history_ab.json]

One JSON line on stdout (and in --out)."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monosowa_amd import miopen_tuning   # noqa: E402
miopen_tuning.use_shipped_db(0)

import numpy as np   # noqa: E402
import torch   # noqa: E402
import yaml    # noqa: E402

from monosowa_amd import pointwise   # noqa: E402
from monosowa_amd._lib import on_device, raw_stream   # noqa: E402
from monosowa_amd.helpers.model_helper import build_model   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.helpers.trainer_helper import Trainer, stage_batch   # noqa: E402
from monosowa_amd.monodetr.criterion import weighted_total   # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402

BATCH = 16


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 64                     # the ring's capacity: drained by step_ab before it is full


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_ab(trainer, batch, steps):
    """ms per train step with the key off / on, alternated."""
    hist = trainer.history
    settings = [False, True]

    def step(on):
        trainer.history = hist if on else None
        trainer.train_step(*batch)
    for on in settings * 4:                  # warm both variants (the first commit ships the group ids)
        step(on)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for i in range(steps):
        on = settings[i & 1]
        if on and len(hist._meta) >= hist.capacity - 1:
            hist.drain()                     # outside the timed region: no overflow drain inside a step
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(on)
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3)
    trainer.history = hist
    return times


def add_losses_launches(trainer, batch):
    """Device launches of one ``add_losses`` call (kernels and copies on the device, from the profiler)."""
    from torch.profiler import ProfilerActivity, profile
    inputs, calibs, targets, info = batch
    tl = trainer.prepare_targets(targets, inputs.shape[0])
    with torch.no_grad():
        loss_dict = trainer.detr_loss(trainer.model(inputs, calibs, tl, targets["img_size"], dn_args=None), tl, None, info)
        total = weighted_total(loss_dict, trainer.detr_loss.weight_dict)
    hist = trainer.history
    hist.drain()
    hist.add_losses(loss_dict, total)
    torch.cuda.synchronize()
    counts = {}
    for scale in (1.0, 0.5):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            hist.add_losses(loss_dict, total, scale=scale)
            torch.cuda.synchronize()
        counts[scale] = sorted(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    hist.ring.zero_()
    return counts


def kernel_ab(trainer, rounds, reps):
    """us of device time per call of the stats pair and per launch of the accumulate kernel, alternated (the order flips every round),
    both over the parameters and gradients of the optimizer's last step."""
    hist, opt = trainer.history, trainer.optimizer
    plans = opt.last_fused_plans()
    assert plans, "the fused AdamW path must have served the last step"
    dev = plans[0].device
    arrays = [hist._group_array(p) for p in plans]
    total = sum(p.n_chunks for p in plans)
    partials = torch.empty(3 * total, dtype=torch.float64, device=dev)
    out = torch.zeros(3 * len(hist.groups) + 3, dtype=torch.float64, device=dev)
    # mono_grad_accumulate_f32's table {acc, g, n} from the p, g and n columns of the AdamW tables
    cols = [p.view[:p.n_chunks * 32].view(np.uint64).reshape(4, p.n_chunks) for p in plans]
    table = np.empty(total * 20, dtype=np.uint8)
    table[:total * 16].view(np.uint64).reshape(2, total)[:] = np.concatenate([c[:2] for c in cols], axis=1)
    table[total * 16:].view(np.int32)[:] = np.concatenate([p.n for p in plans])
    acc_table = torch.from_numpy(table).to(dev)
    elements = int(sum(int(p.n.sum()) for p in plans))
    lib = pointwise.load()

    def stats():
        pointwise.step_stats(plans, arrays, len(hist.groups), None, partials, out.data_ptr())

    def acc():
        with on_device(dev):
            code = lib.mono_grad_accumulate_f32(acc_table.data_ptr(), total, raw_stream())
        assert code == 0
    kernels = [("mono_step_stats_f32", stats), ("mono_grad_accumulate_f32", acc)]
    for _, fn in kernels * 3:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in kernels}
    for r in range(rounds):
        for name, fn in (kernels if r % 2 == 0 else kernels[::-1]):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                fn()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) * 1e3 / reps)
    return times, elements, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed train steps, both settings together")
    ap.add_argument("--rounds", type=int, default=15, help="timed rounds per kernel")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per timed round")
    ap.add_argument("--only-kernels", action="store_true", help="part 2 alone: the run to put under a kernel trace or counters")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = model.to(dev)
    crit.to(dev)
    opt = build_optimizer(cfg["optimizer"], model)
    trainer = Trainer(dict(cfg["trainer"], history=True), model, opt, _Loader(), None, None, None, logging.getLogger("history_ab"), crit,
                      "history_ab")
    assert trainer.history is not None
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    batch = stage_batch((inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in targets.items()}, info), dev)
    result = {"batch": BATCH, "groups": len(trainer.history.groups)}
    if args.only_kernels:
        trainer.train_step(*batch)
    else:
        steps = step_ab(trainer, batch, args.steps)
        hist = trainer.history
        assert hist.kernel_commits > 0, "the device path must have served the commits"
        result.update({"ms_per_step_key_off": _spread(steps[False]), "ms_per_step_key_on": _spread(steps[True])})
        off, on = result["ms_per_step_key_off"]["median"], result["ms_per_step_key_on"]["median"]
        result["key_on_minus_off_ms"] = on - off
        result["key_on_minus_off_percent"] = 100.0 * (on / off - 1.0)
        result["key_on_median_inside_key_off_min_max"] = bool(result["ms_per_step_key_off"]["min"] <= on <= result["ms_per_step_key_off"]["max"])
        launches = add_losses_launches(trainer, batch)
        result["add_losses_device_launches"] = {"scale_1": len(launches[1.0]), "scale_other": len(launches[0.5])}
        result["add_losses_device_launch_names"] = launches[1.0]
        trainer.train_step(*batch)               # the optimizer's tables point at this step's gradients again
    kernels, elements, n_chunks = kernel_ab(trainer, args.rounds, args.reps)
    result.update({"elements": elements, "chunks": n_chunks, "launches_per_timed_round": args.reps,
                   "bytes_per_call": {"mono_step_stats_f32": 8 * elements, "mono_grad_accumulate_f32": 12 * elements}})
    for name, xs in kernels.items():
        s = _spread(xs)
        s["gb_per_s_at_median"] = result["bytes_per_call"][name] / (s["median"] * 1e-6) / 1e9
        result["us_per_call_" + name] = s
    s, a = result["us_per_call_mono_step_stats_f32"], result["us_per_call_mono_grad_accumulate_f32"]
    result["stats_minus_accumulate_percent"] = 100.0 * (s["median"] / a["median"] - 1.0)
    result["stats_not_slower_than_accumulate"] = bool(s["median"] <= a["median"])
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
