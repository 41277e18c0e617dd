"""Cost of the per-label loss weights (``label_weight`` in the targets, ``dataset.label_weights``), measured inside ONE process (the
method of tools/label_audit_ab.py):

1. the train step of the shipped model at the benchmark shape (batch 16, 1280 x 384), steps alternating between the key absent (the
   unweighted launches) and present (a ``label_weight`` of mixed values: the six weighted launches and one gather of the padded
   per-box weights).  Every step is timed with a device sync; median and min-max per setting.
2. the device time of every weighted kernel next to its unweighted sibling on the predictions, pairs and targets of the last step:
   device events around ``--reps`` back-to-back launches, divided by the number of launches, ``--rounds`` times, the two alternating.

    python tools/label_weights_ab.py [--steps 40] [--rounds 15] [--reps 20] [--out profiles/label_weights_ab.json]

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
from monosowa_amd.monodetr import box_ops    # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402

BATCH = 16


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 64


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def step_ab(trainer, batches, steps):
    """ms per train step with the key absent / present, alternated."""
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


def kernel_times(trainer, batch, weights, rounds, reps):
    """us of device time per launch of the six unweighted entry points and of their weighted siblings on one step's own tensors."""
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
    pred = [t.contiguous() for t in (boxes, depth, dims, angle)]
    idx = idx.contiguous()
    tg = [flat["boxes_3d"].to(f32).contiguous(), flat["depth"].reshape(-1).to(f32).contiguous(), flat["size_3d"].to(f32).contiguous(),
          flat["heading_bin"].reshape(-1).to(i64).contiguous(), flat["heading_res"].reshape(-1).to(f32).contiguous()]
    labels = flat["labels"].reshape(-1).to(i64).contiguous()
    tw = weights.to(dev).to(f32).contiguous()
    assert tw.shape[0] == T
    lib, st = pointwise.load(), pointwise.raw_stream()
    out6, comp = torch.empty(NL, 6, device=dev), torch.empty(NL, device=dev)
    go6 = torch.ones(NL, 6, device=dev)
    grads = torch.zeros(NL * B * Q * 35, device=dev)
    n = NL * B * Q
    g4 = [grads[:n * 6], grads[n * 6:n * 8], grads[n * 8:n * 11], grads[n * 11:]]
    p = lambda ts: [t.data_ptr() for t in ts]
    m_args = p(pred) + [idx.data_ptr()] + p(tg)
    out3, go1, glog = torch.empty(NL, 3, device=dev), torch.ones(NL, device=dev), torch.empty_like(logits)
    lg = logits.contiguous()
    # the depth map's padded inputs, as forward_fast builds them
    host = batch[2]["mask_2d"]._host_mask
    counts = host.sum(1)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    maxn = int(counts.max())
    sizes = torch.as_tensor(counts, dtype=f32).to(dev)
    slot = torch.as_tensor(np.minimum(offs[:, None] + np.arange(maxn)[None, :], T - 1), dtype=i64).to(dev)
    valid = torch.as_tensor(np.arange(maxn)[None, :] < counts[:, None]).to(dev).contiguous()
    w, h = crit.depth_map_size
    boxes2d = box_ops.box_cxcywh_to_xyxy(flat["boxes"] * torch.tensor([w, h, w, h], device=dev, dtype=f32))[slot].contiguous()
    depth2d = flat["depth"].reshape(-1)[slot].contiguous()
    weight2d = tw[slot].contiguous()
    dmap = torch.randn(B, 81, h, w, device=dev).contiguous(memory_format=torch.channels_last)
    sb, sc, sp = pointwise._ddn_strides(dmap)
    partial = torch.empty(lib.mono_ddn_loss_blocks(B, h, w), device=dev)
    one, gmap = torch.ones(1, device=dev), torch.empty_like(dmap)
    d_args = [dmap.data_ptr(), boxes2d.data_ptr(), depth2d.data_ptr(), valid.data_ptr()]
    d_tail = (B, 81, h, w, maxn, sb, sc, sp, 0.25, 2.0, 13.0, 1.0, 1e-3, 60.0, st)
    alpha = float(crit.focal_alpha)
    calls = {
        "matched_losses_fwd": lambda: lib.mono_matched_losses_fwd_f32(*m_args, out6.data_ptr(), comp.data_ptr(), NL, B, Q, K, st),
        "matched_losses_weighted_fwd": lambda: lib.mono_matched_losses_weighted_fwd_f32(*m_args, tw.data_ptr(), out6.data_ptr(), comp.data_ptr(), NL, B, Q, K, st),
        "matched_losses_bwd": lambda: lib.mono_matched_losses_bwd_f32(*m_args, comp.data_ptr(), go6.data_ptr(), *p(g4), NL, B, Q, K, st),
        "matched_losses_weighted_bwd": lambda: lib.mono_matched_losses_weighted_bwd_f32(*m_args, tw.data_ptr(), comp.data_ptr(), go6.data_ptr(), *p(g4), NL, B, Q, K, st),
        "focal_fwd": lambda: lib.mono_focal_fwd_f32(lg.data_ptr(), idx.data_ptr(), labels.data_ptr(), sizes.data_ptr(), out3.data_ptr(), NL, B, Q, C, K, alpha, 2.0, st),
        "focal_weighted_fwd": lambda: lib.mono_focal_weighted_fwd_f32(lg.data_ptr(), idx.data_ptr(), labels.data_ptr(), sizes.data_ptr(), tw.data_ptr(), out3.data_ptr(), NL, B, Q, C, K, alpha, 2.0, st),
        "focal_bwd": lambda: lib.mono_focal_bwd_f32(lg.data_ptr(), idx.data_ptr(), labels.data_ptr(), go1.data_ptr(), glog.data_ptr(), NL, B, Q, C, K, alpha, 2.0, st),
        "focal_weighted_bwd": lambda: lib.mono_focal_weighted_bwd_f32(lg.data_ptr(), idx.data_ptr(), labels.data_ptr(), tw.data_ptr(), go1.data_ptr(), glog.data_ptr(), NL, B, Q, C, K, alpha, 2.0, st),
        "ddn_loss_fwd": lambda: lib.mono_ddn_loss_fwd_f32(*d_args, partial.data_ptr(), *d_tail),
        "ddn_loss_weighted_fwd": lambda: lib.mono_ddn_loss_weighted_fwd_f32(*d_args, weight2d.data_ptr(), partial.data_ptr(), *d_tail),
        "ddn_loss_bwd": lambda: lib.mono_ddn_loss_bwd_f32(*d_args, one.data_ptr(), gmap.data_ptr(), *d_tail),
        "ddn_loss_weighted_bwd": lambda: lib.mono_ddn_loss_weighted_bwd_f32(*d_args, weight2d.data_ptr(), one.data_ptr(), gmap.data_ptr(), *d_tail),
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
    return times, {"labels": int(T), "pairs": int(K), "layers": int(NL), "depth_map_boxes_per_image": maxn}


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
    trainer = Trainer(dict(cfg["trainer"]), model, opt, _Loader(), None, None, None, logging.getLogger("label_weights_ab"), crit,
                      "label_weights_ab")
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    pin = lambda tg: (inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in tg.items()}, info)
    rng = np.random.default_rng(7)
    mask = targets["mask_2d"].numpy()
    w = np.ones(mask.shape, np.float32)
    w[mask] = np.where(rng.random(int(mask.sum())) < 0.5, rng.choice([0.0, 0.25, 0.5, 1.0, 2.0], int(mask.sum())),
                       rng.uniform(0.0, 1.5, int(mask.sum()))).astype(np.float32)
    batches = {False: stage_batch(pin(targets), dev), True: stage_batch(pin(dict(targets, label_weight=torch.from_numpy(w))), dev)}
    result = {"batch": BATCH, "group_num": int(crit.group_num)}
    steps = step_ab(trainer, batches, args.steps)
    result.update({"ms_per_step_key_absent": _spread(steps[False]), "ms_per_step_key_present": _spread(steps[True])})
    off, on = result["ms_per_step_key_absent"], result["ms_per_step_key_present"]
    result["key_present_minus_absent_ms"] = on["median"] - off["median"]
    result["key_present_minus_absent_percent"] = 100.0 * (on["median"] / off["median"] - 1.0)
    result["key_present_median_inside_key_absent_min_max"] = bool(off["min"] <= on["median"] <= off["max"])
    times, sizes = kernel_times(trainer, batches[True], torch.from_numpy(w[mask]), args.rounds, args.reps)
    result.update(sizes)
    result["launches_per_timed_round"] = args.reps
    result["us_per_launch"] = {name: _spread(t) for name, t in times.items()}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
