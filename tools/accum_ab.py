"""Paired A/B of the gradient accumulation inside ONE process (the method of tools/ab_step.py): the shipped model at per-GPU batch
16, ``trainer.global_batch: 32`` (K = 2), cycles alternating between ``pointwise.FUSED_ACCUMULATE`` on (one HIP launch adds every
fresh gradient into its accumulator) and off (autograd's in-place add per parameter).  Every cycle is timed with a device sync;
medians are compared (the method resolves 0.3 % of a step, tools/ab_step.py).  Then one profiled cycle per setting: device events in
the cycle, counted like tools/launch_census.py (copies included); the count should fall by about one per gradient tensor and
extra micro-step.

    python tools/accum_ab.py [--cycles 40] [--out profiles/accum_ab.json]

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
from monosowa_amd.helpers.model_helper import build_model   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.helpers.trainer_helper import Trainer   # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402

BATCH, K = 16, 2


class _Loader:
    """K collated host batches in pinned memory, as a DataLoader with pin_memory hands them over."""
    batch_size = BATCH

    def __init__(self):
        self.batches = []
        for k in range(K):
            inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444 + k)
            self.batches.append((inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in targets.items()}, info))

    def __len__(self):
        return K

    def __iter__(self):
        return iter(self.batches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=40, help="timed cycles, both settings together")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = model.to(dev)
    crit.to(dev)
    opt = build_optimizer(cfg["optimizer"], model)
    loader = _Loader()
    trainer = Trainer(dict(cfg["trainer"], global_batch=BATCH * K), model, opt, loader, None, None, None, logging.getLogger("accum_ab"), crit,
                      "accum_ab")
    assert trainer.accum_steps == K
    trainer.model.train()
    crit.train()
    raws = list(loader)
    settings = [True, False]

    def cycle(on):
        pointwise.FUSED_ACCUMULATE = on
        trainer.train_cycle(raws)
    for on in settings * 4:                  # warm both variants
        cycle(on)
    torch.cuda.synchronize()
    times = {True: [], False: []}
    for i in range(args.cycles):
        on = settings[i & 1]
        torch.cuda.synchronize()
        t = time.perf_counter()
        cycle(on)
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3)

    from torch.profiler import ProfilerActivity, profile
    launches = {}
    for on in settings:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            cycle(on)
            torch.cuda.synchronize()
        launches[on] = len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])
    tensors = len([p for p in model.parameters() if p.grad is not None])
    result = {"batch": BATCH, "micro_steps": K, "cycles_per_setting": len(times[True]),
              "ms_per_cycle_kernel": statistics.median(times[True]), "ms_per_cycle_autograd": statistics.median(times[False]),
              "min_ms_kernel": min(times[True]), "min_ms_autograd": min(times[False]),
              "launches_per_cycle_kernel": launches[True], "launches_per_cycle_autograd": launches[False],
              "gradient_tensors": tensors}
    result["launch_drop"] = launches[False] - launches[True]
    result["expected_launch_drop"] = tensors * (K - 1)             # one in-place add per gradient tensor and extra micro-step
    result["kernel_minus_autograd_percent"] = 100.0 * (result["ms_per_cycle_kernel"] / result["ms_per_cycle_autograd"] - 1.0)
    result["resolution_percent"] = 0.3                             # of the paired-median method; slower by more than this: drop the kernel
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
