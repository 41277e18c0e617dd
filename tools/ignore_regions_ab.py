"""Cost of the ignore regions (``ignore_boxes`` / ``ignore_mask`` in the targets, ``dataset.ignore_regions``), measured inside ONE
process (the method of tools/label_weights_ab.py):

1. the train step of the shipped model at the benchmark shape (batch 16, 1280 x 384), steps alternating between the keys absent (the
   launches of before) and present (a few ignore boxes per image: the flags launch in front of the matcher's wait and the focal launches
   through the ignore entry points).  Every step is timed with a device sync; median and min-max per setting.
2. the device time of the flags launch, and of each of the four focal entry points with flag bytes next to its sibling, on the
   predictions, pairs and targets of the last step: device events around ``--reps`` back-to-back launches, divided by the number of
   launches, ``--rounds`` times, the order alternating.

    python tools/ignore_regions_ab.py [--steps 40] [--rounds 15] [--reps 20] [--out profiles/ignore_regions_ab.json]

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
from monosowa_amd.helpers.model_helper import build_model   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.helpers.trainer_helper import Trainer, stage_batch   # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402

BATCH = 16
BOXES_PER_IMAGE = 4


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 64


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_ab(trainer, batches, steps):
    """ms per train step with the keys absent / present, alternated."""
    settings = [False, True]
    for on in settings * 4:                  # warm both variants
        trainer.train_step(*batches[on])
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for i in range(steps):
        on = settings[i & 1]
        torch.cuda.synchronize()
        t = time.perf_counter()
        trainer.train_step(*batches[on])
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3)
    return times


class _Capture:
    """Stands in for the label audit during one forward: keeps what the criterion hands ``observe``."""
    args = None

    def observe(self, *args, **kwargs):
        self.args = args


def kernel_times(trainer, batch, rounds, reps):
    """us of device time per launch of the flags kernel and of the four focal entry points with and without the flag bytes, on one
    step's own tensors (the weighted ones with a weight of 1 per label)."""
    crit = trainer.detr_loss
    capture = _Capture()
    crit.audit = capture
    try:
        trainer.train_step(*batch)
    finally:
        del crit.audit
    logits, boxes, depth, dims, angle, idx, flat = capture.args
    dev = logits.device
    f32, i64 = torch.float32, torch.int64
    NL, B, Q, C = logits.shape
    K, T = idx.shape[2], flat["labels"].shape[0]
    lg, bx, idx = logits.contiguous(), boxes.contiguous(), idx.contiguous()
    labels = flat["labels"].reshape(-1).to(i64).contiguous()
    tw = torch.ones(T, dtype=f32, device=dev)
    sizes = torch.as_tensor(batch[2]["mask_2d"]._host_mask.sum(1), dtype=f32).to(dev)
    gb = batch[2]["ignore_boxes"].to(f32).contiguous()
    gm = batch[2]["ignore_mask"].contiguous().view(torch.uint8)
    M = gb.shape[1]
    flags = torch.empty((NL, B, Q), dtype=torch.uint8, device=dev)
    counts = torch.empty((NL,), dtype=torch.int32, device=dev)
    lib, st = pointwise.load(), pointwise.raw_stream()
    out3, go1, glog = torch.empty(NL, 3, device=dev), torch.ones(NL, device=dev), torch.empty_like(lg)
    alpha = float(crit.focal_alpha)
    tail = (NL, B, Q, C, K, alpha, 2.0, st)
    L, I, LB, S, W, FL, O, G, GL = (t.data_ptr() for t in (lg, idx, labels, sizes, tw, flags, out3, go1, glog))
    calls = {
        "ignore_flags": lambda: lib.mono_ignore_flags_f32(bx.data_ptr(), gb.data_ptr(), gm.data_ptr(), FL, counts.data_ptr(), NL, B, Q, M,
                                                          float(crit.ignore_ioa), st),
        "focal_fwd": lambda: lib.mono_focal_fwd_f32(L, I, LB, S, O, *tail),
        "focal_ignore_fwd": lambda: lib.mono_focal_ignore_fwd_f32(L, I, LB, S, FL, O, *tail),
        "focal_bwd": lambda: lib.mono_focal_bwd_f32(L, I, LB, G, GL, *tail),
        "focal_ignore_bwd": lambda: lib.mono_focal_ignore_bwd_f32(L, I, LB, FL, G, GL, *tail),
        "focal_weighted_fwd": lambda: lib.mono_focal_weighted_fwd_f32(L, I, LB, S, W, O, *tail),
        "focal_weighted_ignore_fwd": lambda: lib.mono_focal_weighted_ignore_fwd_f32(L, I, LB, S, W, FL, O, *tail),
        "focal_weighted_bwd": lambda: lib.mono_focal_weighted_bwd_f32(L, I, LB, W, G, GL, *tail),
        "focal_weighted_ignore_bwd": lambda: lib.mono_focal_weighted_ignore_bwd_f32(L, I, LB, W, FL, G, GL, *tail),
    }
    for name, fn in calls.items():
        code = fn()
        assert code == 0, (name, code)
    torch.cuda.synchronize()
    flagged = counts.tolist()
    times = {name: [] for name in calls}
    names = list(calls)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                calls[name]()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) * 1e3 / reps)
    return times, {"labels": int(T), "pairs": int(K), "layers": int(NL), "cells_per_layer": int(B * Q), "ignore_slots": int(M),
                   "ignore_boxes": int(batch[2]["ignore_mask"].sum()), "flagged_per_layer": flagged}


def ignore_boxes(batch, per_image, seed=7):
    """[B, 50, 4] / [B, 50]: ``per_image`` windows of 0.1 .. 0.3 of the image per image, packed at the front."""
    rng = np.random.default_rng(seed)
    boxes, mask = np.zeros((batch, 50, 4), np.float32), np.zeros((batch, 50), bool)
    lo = rng.uniform(0.0, 0.7, (batch, per_image, 2))
    boxes[:, :per_image] = np.concatenate([lo, np.minimum(lo + rng.uniform(0.1, 0.3, (batch, per_image, 2)), 1.0)], -1)
    mask[:, :per_image] = True
    return torch.from_numpy(boxes), torch.from_numpy(mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed train steps, both settings together")
    ap.add_argument("--rounds", type=int, default=15, help="timed rounds per kernel")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per timed round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = model.to(dev)
    crit.to(dev)
    opt = build_optimizer(cfg["optimizer"], model)
    trainer = Trainer(dict(cfg["trainer"]), model, opt, _Loader(), None, None, None, logging.getLogger("ignore_regions_ab"), crit,
                      "ignore_regions_ab")
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    pin = lambda tg: (inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in tg.items()}, info)
    gb, gm = ignore_boxes(BATCH, BOXES_PER_IMAGE)
    batches = {False: stage_batch(pin(targets), dev), True: stage_batch(pin(dict(targets, ignore_boxes=gb, ignore_mask=gm)), dev)}
    result = {"batch": BATCH, "group_num": int(crit.group_num), "ignore_ioa": float(crit.ignore_ioa)}
    steps = step_ab(trainer, batches, args.steps)
    result.update({"ms_per_step_keys_absent": _spread(steps[False]), "ms_per_step_keys_present": _spread(steps[True])})
    off, on = result["ms_per_step_keys_absent"], result["ms_per_step_keys_present"]
    result["keys_present_minus_absent_ms"] = on["median"] - off["median"]
    result["keys_present_minus_absent_percent"] = 100.0 * (on["median"] / off["median"] - 1.0)
    result["keys_present_median_inside_keys_absent_min_max"] = bool(off["min"] <= on["median"] <= off["max"])
    times, sizes = kernel_times(trainer, batches[True], args.rounds, args.reps)
    result.update(sizes)
    ignored, cells = crit.ignore_report()
    result["ignored_per_layer"] = ignored
    result["launches_per_timed_round"] = args.reps
    result["us_per_launch"] = {name: _spread(t) for name, t in times.items()}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
