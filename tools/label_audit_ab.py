"""Cost of the label audit (``trainer.label_audit``), measured inside ONE process (the method of tools/history_ab.py):

1. the train step of the shipped model at the benchmark shape (batch 16, 1280 x 384), steps alternating between the key off (no
   ``LabelAudit`` call at all, ``criterion.audit`` None) and on (``begin_batch`` in front of the forward, ``observe`` -- one launch of
   ``mono_label_audit_f32`` and one copy of the classes -- behind the matching).  Every step is timed with a device sync; median and
   min-max per setting.
2. the device time of ``mono_label_audit_f32`` alone on the predictions, pairs and targets of the last step: device events around
   ``--reps`` back-to-back launches, divided by the number of launches, ``--rounds`` times -- and the same around whole ``observe``
   calls (the launch, the copy of the classes and the host work between them), the two alternating.

    python tools/label_audit_ab.py [--steps 40] [--rounds 15] [--reps 20] [--out profiles/label_audit_ab.json]

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

from monosowa_amd import label_audit, pointwise   # noqa: E402
from monosowa_amd.helpers.model_helper import build_model   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.helpers.trainer_helper import Trainer, stage_batch   # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402

BATCH = 16


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 64                     # ring of 64 x 16 x 50 rows: drained by step_ab before it is full


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_ab(trainer, batch, steps):
    """ms per train step with the key off / on, alternated."""
    audit, crit = trainer.label_audit, trainer.detr_loss
    settings = [False, True]

    def step(on):
        trainer.label_audit = crit.audit = audit if on else None
        trainer.train_step(*batch)
    for on in settings * 4:                  # warm both variants
        step(on)
    torch.cuda.synchronize()
    audit.drain()
    times = {False: [], True: []}
    for i in range(steps):
        on = settings[i & 1]
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(on)
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3)
    trainer.label_audit = crit.audit = audit
    return times


class _Capture:
    """Stands in for the audit during one forward: keeps what the criterion hands ``observe``."""
    args = None

    def observe(self, *args, **kwargs):
        self.args = (args, kwargs)


def kernel_times(trainer, batch, rounds, reps):
    """us of device time per launch of mono_label_audit_f32 on one step's own tensors, and their sizes."""
    audit, crit = trainer.label_audit, trainer.detr_loss
    capture = _Capture()
    trainer.label_audit, crit.audit = None, capture
    try:
        trainer.train_step(*batch)
    finally:
        trainer.label_audit = crit.audit = audit
    (logits, boxes, depth, dims, angle, idx, flat), kwargs = capture.args
    T = flat["labels"].shape[0]
    probe = label_audit.LabelAudit(T, logits.device)

    def launch():
        probe.begin_batch([0], torch.ones(1, T, dtype=torch.bool))
        probe.observe(logits, boxes, depth, dims, angle, idx, flat, **kwargs)
        probe._fill, probe._keys = 0, []          # the same rows again
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    assert probe.kernel_observes == 3, "the device path must have served the observes"
    f32, i64 = torch.float32, torch.int64
    tensors = [t.contiguous() for t in (logits, boxes, depth, dims, angle)] + [idx.contiguous(), flat["labels"].reshape(-1).to(i64).contiguous(),
               flat["boxes_3d"].to(f32).contiguous(), flat["depth"].reshape(-1).to(f32).contiguous(), flat["size_3d"].to(f32).contiguous(),
               flat["heading_bin"].reshape(-1).to(i64).contiguous(), flat["heading_res"].reshape(-1).to(f32).contiguous()]
    out = torch.zeros(T, label_audit.WIDTH, dtype=torch.float64, device=logits.device)

    def kernel():
        pointwise.label_audit(*tensors, out.data_ptr(), T, kwargs.get("layer", 0))
    kernel()
    torch.cuda.synchronize()
    assert torch.equal(out, probe.ring[:T])
    times = {"observe": [], "kernel": []}
    for r in range(rounds):
        for name, fn in ((("observe", launch), ("kernel", kernel)) if r % 2 == 0 else (("kernel", kernel), ("observe", launch))):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                fn()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) * 1e3 / reps)
    return times, {"labels": int(T), "pairs": int(idx.shape[2]), "layers": int(idx.shape[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed train steps, both settings together")
    ap.add_argument("--rounds", type=int, default=15, help="timed rounds of the kernel")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back observes per timed round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = model.to(dev)
    crit.to(dev)
    opt = build_optimizer(cfg["optimizer"], model)
    trainer = Trainer(dict(cfg["trainer"], label_audit=True), model, opt, _Loader(), None, None, None, logging.getLogger("label_audit_ab"),
                      crit, "label_audit_ab")
    assert trainer.label_audit is not None and crit.audit is trainer.label_audit
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    batch = stage_batch((inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in targets.items()}, info), dev)
    result = {"batch": BATCH, "group_num": int(crit.group_num)}
    steps = step_ab(trainer, batch, args.steps)
    assert trainer.label_audit.kernel_observes > 0 and trainer.label_audit.early_drains == 0
    result.update({"ms_per_step_key_off": _spread(steps[False]), "ms_per_step_key_on": _spread(steps[True])})
    off, on = result["ms_per_step_key_off"], result["ms_per_step_key_on"]
    result["key_on_minus_off_ms"] = on["median"] - off["median"]
    result["key_on_minus_off_percent"] = 100.0 * (on["median"] / off["median"] - 1.0)
    result["key_on_median_inside_key_off_min_max"] = bool(off["min"] <= on["median"] <= off["max"])
    times, sizes = kernel_times(trainer, batch, args.rounds, args.reps)
    result.update(sizes)
    result["observes_per_timed_round"] = args.reps
    result["us_per_call_mono_label_audit_f32"] = _spread(times["kernel"])
    result["us_per_observe_kernel_and_class_copy"] = _spread(times["observe"])
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
