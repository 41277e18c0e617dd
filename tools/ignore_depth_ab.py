"""Cost of ``model.ignore_depth_map`` (depth-map pixels under an ignore box leave ``loss_depth_map``), on the model of
tools/ignore_regions_ab.py:

1. the train step of the shipped model at the benchmark shape (batch 16, 1280 x 384), in ONE process, the steps cycling through three
   settings: the keys absent (no ignore boxes in the batch, ``model.ignore_depth_map`` off: the launches of before), ignore boxes present
   with the key off (``dataset.ignore_regions`` alone), and both present (four ignore boxes per image, the depth-map loss through the
   ignore entry points).  ``--steps`` timed steps per setting, each timed with a device sync; median and min-max per setting.
2. the device time per launch of the four sibling -> ignore pairs of csrc/ddn_loss.hip on the depth-map logits, boxes and ignore boxes
   of one such step: device events around ``--reps`` back-to-back launches, divided by the number of launches, ``--rounds`` times, the
   order alternating.
3. with ``--parent DIR`` (a built checkout of the parent commit): ``bench.py --gpus 1`` -- its train leg -- of that checkout and of this
   tree, alternated ``--bench-rounds`` times, each run a fresh child process under its own time limit; the first failure ends the
   series.  The usual condition: this tree's median ms per step inside the parent's own min-max.

    python tools/ignore_depth_ab.py [--steps 20] [--rounds 15] [--reps 20] [--parent DIR] [--out profiles/ignore_depth_ab.json]

One JSON line on stdout (and in --out)."""
import argparse
import json
import logging
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 16
BOXES_PER_IMAGE = 4


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 64


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


SETTINGS = ("keys_absent", "ignore_boxes_only", "keys_present")


def _apply(trainer, setting):
    trainer.detr_loss.ignore_depth_map = setting == "keys_present"


def step_ab(trainer, batches, steps):
    """ms per train step of the three settings, cycled."""
    import torch
    for setting in SETTINGS * 3:                  # warm every variant
        _apply(trainer, setting)
        trainer.train_step(*batches[setting])
    torch.cuda.synchronize()
    times = {s: [] for s in SETTINGS}
    for i in range(steps * len(SETTINGS)):
        setting = SETTINGS[i % len(SETTINGS)]
        _apply(trainer, setting)
        torch.cuda.synchronize()
        t = time.perf_counter()
        trainer.train_step(*batches[setting])
        torch.cuda.synchronize()
        times[setting].append((time.perf_counter() - t) * 1e3)
    return times


def kernel_times(trainer, batch, rounds, reps):
    """us of device time per launch of the four DDN loss entry points and of their ignore siblings, on one step's own tensors (the
    weighted ones with a weight of 1 per box)."""
    import torch
    from monosowa_amd import pointwise
    crit = trainer.detr_loss
    seen = {}
    inner = crit.ddn_loss.forward_padded

    def capture(logits, boxes, depth, valid, box_weight=None, ignore=None):
        seen.update(logits=logits.detach(), boxes=boxes.detach(), depth=depth.detach(), valid=valid, ignore=ignore)
        return inner(logits, boxes, depth, valid, box_weight=box_weight, ignore=ignore)
    crit.ddn_loss.forward_padded = capture
    try:
        _apply(trainer, "keys_present")
        trainer.train_step(*batch)
    finally:
        del crit.ddn_loss.forward_padded
    lg = seen["logits"]
    B, C, H, W = lg.shape
    sb, sc, sp = pointwise._ddn_strides(lg)
    bx, dp, vl = seen["boxes"].contiguous(), seen["depth"].contiguous(), seen["valid"].contiguous()
    gb, gv = seen["ignore"][0].contiguous(), seen["ignore"][1].contiguous()
    N, M = bx.shape[1], gb.shape[1]
    dev = lg.device
    bw = torch.ones((B, N), dtype=torch.float32, device=dev)
    lib, st = pointwise.load(), pointwise.raw_stream()
    blocks = lib.mono_ddn_loss_blocks(B, H, W)
    partial = torch.empty(blocks, dtype=torch.float32, device=dev)
    count = torch.empty(blocks, dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    grad = torch.empty_strided(lg.shape, lg.stride(), dtype=lg.dtype, device=dev)
    L, BX, DP, VL, BW, GB, GV, PA, CN, ON, GR = (t.data_ptr() for t in (lg, bx, dp, vl, bw, gb, gv, partial, count, one, grad))
    tail = (sb, sc, sp, float(crit.ddn_loss.alpha), float(crit.ddn_loss.gamma), float(crit.ddn_loss.fg_weight), float(crit.ddn_loss.bg_weight),
            1e-3, 60.0, st)
    d, di = (B, C, H, W, N), (B, C, H, W, N, M)
    calls = {
        "ddn_fwd": lambda: lib.mono_ddn_loss_fwd_f32(L, BX, DP, VL, PA, *d, *tail),
        "ddn_ignore_fwd": lambda: lib.mono_ddn_loss_ignore_fwd_f32(L, BX, DP, VL, GB, GV, PA, CN, *di, *tail),
        "ddn_bwd": lambda: lib.mono_ddn_loss_bwd_f32(L, BX, DP, VL, ON, GR, *d, *tail),
        "ddn_ignore_bwd": lambda: lib.mono_ddn_loss_ignore_bwd_f32(L, BX, DP, VL, GB, GV, ON, GR, *di, *tail),
        "ddn_weighted_fwd": lambda: lib.mono_ddn_loss_weighted_fwd_f32(L, BX, DP, VL, BW, PA, *d, *tail),
        "ddn_weighted_ignore_fwd": lambda: lib.mono_ddn_loss_weighted_ignore_fwd_f32(L, BX, DP, VL, BW, GB, GV, PA, CN, *di, *tail),
        "ddn_weighted_bwd": lambda: lib.mono_ddn_loss_weighted_bwd_f32(L, BX, DP, VL, BW, ON, GR, *d, *tail),
        "ddn_weighted_ignore_bwd": lambda: lib.mono_ddn_loss_weighted_ignore_bwd_f32(L, BX, DP, VL, BW, GB, GV, ON, GR, *di, *tail),
    }
    for name, fn in calls.items():
        code = fn()
        assert code == 0, (name, code)
    torch.cuda.synchronize()
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
    return times, {"map": [int(H), int(W)], "bins": int(C), "box_slots": int(N), "ignore_slots": int(M),
                   "ignore_boxes": int(gv.sum()), "logit_strides": [int(sb), int(sc), int(sp)]}


def ignore_boxes(batch, per_image, seed=7):
    """[B, 50, 4] / [B, 50]: ``per_image`` windows of 0.1 .. 0.3 of the image per image, packed at the front."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    boxes, mask = np.zeros((batch, 50, 4), np.float32), np.zeros((batch, 50), bool)
    lo = rng.uniform(0.0, 0.7, (batch, per_image, 2))
    boxes[:, :per_image] = np.concatenate([lo, np.minimum(lo + rng.uniform(0.1, 0.3, (batch, per_image, 2)), 1.0)], -1)
    mask[:, :per_image] = True
    return torch.from_numpy(boxes), torch.from_numpy(mask)


def measure(args):
    from monosowa_amd import miopen_tuning
    miopen_tuning.use_shipped_db(0)
    import torch
    import yaml
    from monosowa_amd.helpers.model_helper import build_model
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.helpers.trainer_helper import Trainer, stage_batch
    from monosowa_amd.synthetic import make_batch
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = model.to(dev)
    crit.to(dev)
    opt = build_optimizer(cfg["optimizer"], model)
    trainer = Trainer(dict(cfg["trainer"]), model, opt, _Loader(), None, None, None, logging.getLogger("ignore_depth_ab"), crit,
                      "ignore_depth_ab")
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    pin = lambda tg: (inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in tg.items()}, info)
    gb, gm = ignore_boxes(BATCH, BOXES_PER_IMAGE)
    with_boxes = stage_batch(pin(dict(targets, ignore_boxes=gb, ignore_mask=gm)), dev)
    batches = {"keys_absent": stage_batch(pin(targets), dev), "ignore_boxes_only": with_boxes, "keys_present": with_boxes}
    result = {"batch": BATCH, "ignore_boxes_per_image": BOXES_PER_IMAGE}
    steps = step_ab(trainer, batches, args.steps)
    for s in SETTINGS:
        result["ms_per_step_" + s] = _spread(steps[s])
    off, on = result["ms_per_step_keys_absent"], result["ms_per_step_keys_present"]
    result["keys_present_minus_absent_ms"] = on["median"] - off["median"]
    result["keys_present_minus_absent_percent"] = 100.0 * (on["median"] / off["median"] - 1.0)
    result["keys_present_median_inside_keys_absent_min_max"] = bool(off["min"] <= on["median"] <= off["max"])
    times, sizes = kernel_times(trainer, batches["keys_present"], args.rounds, args.reps)
    result.update(sizes)
    result["ignored_pixels"] = list(crit.ignore_depth_report())
    result["launches_per_timed_round"] = args.reps
    result["us_per_launch"] = {name: _spread(t) for name, t in times.items()}
    _apply(trainer, "keys_absent")
    return result


def bench_ab(parent, rounds, steps, warmup, limit):
    """``bench.py``'s train leg of the parent checkout and of this tree, alternated; every run a child process under its own limit."""
    runs = {"parent": [], "tree": []}
    for r in range(rounds):
        for name, root in (("parent", parent), ("tree", ROOT)):
            cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                   "--no-cpu-baseline", "--no-inference-leg", "--no-dataloader-leg", "--no-step-roofline", "--no-offsets-probe"]
            done = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=limit, text=True)
            if done.returncode != 0:
                return {"error": "%s run %d ended with status %d" % (name, r, done.returncode), "runs": runs}
            line = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
            runs[name].append(float(line["ms_per_step"]))
            print("bench %s round %d: %.3f ms/step" % (name, r, runs[name][-1]), file=sys.stderr, flush=True)
    out = {"steps": steps, "warmup": warmup, "ms_per_step_parent": _spread(runs["parent"]), "ms_per_step_tree": _spread(runs["tree"]),
           "runs": runs}
    p, t = out["ms_per_step_parent"], out["ms_per_step_tree"]
    out["tree_median_inside_parent_min_max"] = bool(p["min"] <= t["median"] <= p["max"])
    out["tree_minus_parent_percent"] = 100.0 * (t["median"] / p["median"] - 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed train steps per setting")
    ap.add_argument("--rounds", type=int, default=15, help="timed rounds per kernel")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per timed round")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: alternate bench.py's train leg with this tree's")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--bench-limit", type=float, default=240.0, help="seconds per bench.py run")
    ap.add_argument("--skip-steps", action="store_true", help="only the bench.py series")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {}
    if args.parent:                      # first, while this process has not touched the GPU
        result["bench_train_leg"] = bench_ab(os.path.abspath(args.parent), args.bench_rounds, args.bench_steps, args.bench_warmup,
                                             args.bench_limit)
    if not args.skip_steps and "error" not in result.get("bench_train_leg", {}):
        result.update(measure(args))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if "error" in result.get("bench_train_leg", {}) else 0


if __name__ == "__main__":
    sys.exit(main())
