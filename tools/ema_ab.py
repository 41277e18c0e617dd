"""Cost of the weight average (``trainer.ema_decay``), measured inside ONE process (the method of tools/ab_step.py and tools/accum_ab.py):

1. the train step of the shipped model at the benchmark shape (batch 16, 1280 x 384), steps alternating between the key off (no
   ``ModelEMA.update`` at all) and on (one ``mono_ema_update_f32`` launch behind the optimizer step).  Every step is timed with a device
   sync; median and min-max per setting.
2. the device time of ``mono_ema_update_f32`` and of its sibling ``mono_grad_accumulate_f32`` -- the same 12 bytes per element: two
   loads, one store -- over the same full-model tensor list (every parameter the optimizer moves) and from the same device table,
   rounds alternating between the two: device events around ``--reps`` back-to-back launches, divided by the number of launches.

    python tools/ema_ab.py [--steps 40] [--rounds 15] [--reps 20] [--only-kernels] [--out profiles/ema_ab.json]

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

import torch   # noqa: E402
import yaml    # noqa: E402

from monosowa_amd import pointwise   # noqa: E402
from monosowa_amd._lib import on_device, raw_stream   # noqa: E402
from monosowa_amd.ema import EMAPlan   # noqa: E402
from monosowa_amd.helpers.model_helper import build_model   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.helpers.trainer_helper import Trainer, stage_batch   # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402

BATCH = 16
DECAY = 0.9998


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 1


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_ab(trainer, batch, steps):
    """ms per train step with the key off / on, alternated."""
    ema = trainer.ema
    settings = [False, True]

    def step(on):
        trainer.ema = ema if on else None
        trainer.train_step(*batch)
    for on in settings * 4:                  # warm both variants (the first update ships the table)
        step(on)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for i in range(steps):
        on = settings[i & 1]
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(on)
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3)
    trainer.ema = ema
    return times


def kernel_ab(params, rounds, reps):
    """us of device time per launch of the two kernels, alternated (the order flips every round).  Both run over the SAME tensors from
    the SAME device table -- destination = a copy of every tracked parameter, source = the parameters; the two tables have one layout --
    so neither addresses nor allocation placement differ between them, only the kernel."""
    dev = params[0].device
    with torch.no_grad():
        dsts = [p.detach().clone() for p in params]
    assert pointwise.accumulate_supported(dsts, params)
    plan = EMAPlan(dsts, params)
    lib = pointwise.load()
    w = 1.0 - DECAY

    def ema():
        plan.launch(w)

    def acc():
        with on_device(dev):
            code = lib.mono_grad_accumulate_f32(plan.dev.data_ptr(), plan.n_chunks, raw_stream())
        assert code == 0
    kernels = [("mono_ema_update_f32", ema), ("mono_grad_accumulate_f32", acc)]
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
    elements = sum(p.numel() for p in params)
    return times, elements, plan.n_chunks


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
    trainer = Trainer(dict(cfg["trainer"], ema_decay=DECAY), model, opt, _Loader(), None, None, None, logging.getLogger("ema_ab"), crit,
                      "ema_ab")
    assert trainer.ema is not None
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    batch = stage_batch((inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in targets.items()}, info), dev)
    result = {"batch": BATCH, "decay": DECAY}
    if not args.only_kernels:
        steps = step_ab(trainer, batch, args.steps)
        assert trainer.ema.plan is not None, "the device path must have served the updates"
        result.update({"launches_per_update": trainer.ema.plan.launches / trainer.ema.updates,
                       "ms_per_step_key_off": _spread(steps[False]), "ms_per_step_key_on": _spread(steps[True])})
        off, on = result["ms_per_step_key_off"]["median"], result["ms_per_step_key_on"]["median"]
        result["key_on_minus_off_ms"] = on - off
        result["key_on_minus_off_percent"] = 100.0 * (on / off - 1.0)
    _, tracked = trainer.ema._pairs()
    kernels, elements, n_chunks = kernel_ab(tracked, args.rounds, args.reps)
    result.update({"tracked_tensors": len(tracked), "tracked_elements": elements, "chunks": n_chunks, "bytes_per_launch": 12 * elements,
                   "launches_per_timed_round": args.reps})
    for name, xs in kernels.items():
        s = _spread(xs)
        s["gb_per_s_at_median"] = 12 * elements / (s["median"] * 1e-6) / 1e9
        result["us_per_launch_" + name] = s
    e, a = result["us_per_launch_mono_ema_update_f32"], result["us_per_launch_mono_grad_accumulate_f32"]
    result["ema_minus_accumulate_percent"] = 100.0 * (e["median"] / a["median"] - 1.0)
    result["ema_median_inside_accumulate_min_max"] = bool(a["min"] <= e["median"] <= a["max"])
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
