"""Paired timing of the shipped train step (per-GPU batch 16, 1280 x 384) with the optimizer's guard off and on
(``optimizer.clip_max_norm`` / ``optimizer.skip_nonfinite``, monosowa_amd/helpers/optimizer_helper.py) inside ONE process: blocks of
steps alternate between the two (off, on, off, on, ...), every block ends in a device sync, medians are compared -- the method of
tools/ab_step.py for a setting that lives on the optimizer.  Prints one JSON line.

    python tools/guarded_step_ab.py [--steps 120] [--block 4] [--clip 0.1]
    python tools/guarded_step_ab.py --only on --steps 6        (guarded steps alone: the run to put under a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monosowa_amd import miopen_tuning   # noqa: E402
miopen_tuning.use_shipped_db(0)

import torch   # noqa: E402
import yaml    # noqa: E402

from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.monodetr.criterion import weighted_total   # noqa: E402
from monosowa_amd.synthetic import make_batch, prepare_targets    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--block", type=int, default=4, help="steps per timed block (no sync inside a block, as in bench.py)")
    ap.add_argument("--clip", type=float, default=0.1)
    ap.add_argument("--only", choices=["off", "on"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = to_mi355x_layout(model.to(dev)).train()
    crit.to(dev).train()
    opt = build_optimizer(cfg["optimizer"], model)
    inputs, calibs, targets, info = make_batch(16, dev)
    inputs = inputs.contiguous(memory_format=torch.channels_last)

    def guard(on):
        opt.clip_max_norm, opt.skip_nonfinite = (args.clip, True) if on else (None, False)

    def step():
        tl = prepare_targets(targets, 16)
        opt.zero_grad(set_to_none=True)
        o = model(inputs, calibs, tl, targets["img_size"])
        weighted_total(crit(o, tl), crit.weight_dict).backward()
        opt.step()

    variants = [False, True] if args.only is None else [args.only == "on"]
    for on in variants * 8:              # warm every variant
        guard(on)
        step()
    torch.cuda.synchronize()
    times = {on: [] for on in variants}
    for i in range(args.steps // args.block):
        on = variants[i % len(variants)]
        guard(on)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.block):
            step()
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3 / args.block)
    out = {"workload": "train step, batch 16, 1280x384", "block": args.block, "clip_max_norm": args.clip}
    for on, ts in times.items():
        out["guard_on" if on else "guard_off"] = {"median_ms": round(statistics.median(ts), 3), "mean_ms": round(statistics.mean(ts), 3),
                                                  "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "blocks": len(ts)}
    if len(times) == 2:
        out["on_minus_off_median_ms"] = round(statistics.median(times[True]) - statistics.median(times[False]), 3)
    if True in times:
        out["guard_report"] = opt.guard_report()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
