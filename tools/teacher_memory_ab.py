"""Cost of the label memory (``trainer.teacher_memory``), measured inside ONE process (the method of tools/teacher_ab.py), shipped
model, batch 16, 1280 x 384:

1. the device time per launch of ``mono_memory_merge_f64`` at B = 16, M = 50 and R = 50 / R = 100 rows per image, beside
   ``mono_fuse_dets_f64`` and ``mono_encode_targets_f64`` on the same rows in the same run: event pairs around ``--reps`` back-to-back
   launches, the median of 5.  The bank holds a first pass of the same rows, so every launch matches a full frame.
2. the train step with ``trainer.teacher`` on and the memory off / on, two Trainers alternating, ``--steps`` each, every step between
   two device synchronisations; median and min-max per setting.
3. with ``--parent DIR`` (a built checkout of the parent commit) and both keys absent: ``bench.py``'s train leg, parent and this tree
   alternated three times; this tree's median against the parent's own spread.

    python tools/teacher_memory_ab.py [--steps 20] [--reps 20] [--parent DIR] [--skip-steps] [--out profiles/teacher_memory_ab_<date>.json]

One JSON line on stdout (and in --out)."""
import argparse
import copy
import datetime
import json
import logging
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import teacher_ab as base   # noqa: E402  (sets the MIOpen database up before torch is imported)

import numpy as np   # noqa: E402
import torch   # noqa: E402
import yaml    # noqa: E402

from monosowa_amd.fuse import fuse_rows_device   # noqa: E402
from monosowa_amd.teacher import Teacher, encode_targets, student_records   # noqa: E402
from monosowa_amd.teacher_memory import LabelMemory   # noqa: E402

BATCH, SLOTS = base.BATCH, 50


def generated_rows(B, R, seed=0):
    """B images of R plausible rows, score descending: objects on a 6 m grid (disjoint), every third one seen twice a few centimetres
    apart, so that fuse suppresses some and the merge walks past claimed entries."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((B, R, 14))
    for b in range(B):
        scores = np.sort(rng.uniform(0.05, 0.95, R))[::-1]
        for i in range(R):
            j = i - 1 if i % 3 == 2 else i
            x, z = -45.0 + 6.0 * (j % 16) + (0.05 if i != j else 0.0), 8.0 + 6.0 * (j // 16)
            u = 600.0 + 700.0 * x / z
            rows[b, i] = (j % 3, 0.1, u - 40, 150, u + 40, 220, 1.5, 1.7, 4.0, x, 1.6, z, 0.3, scores[i])
    return rows


def kernel_times(teacher, raw, reps):
    dev = teacher.device
    canvas, calibs, targets, info = raw
    _, geom, _ = teacher._teacher_view(calibs, targets["img_size"])
    geom = geom.to(dev)
    records = torch.from_numpy(student_records(calibs, targets["img_size"], info["flip"], info["affine"], info["scale_depth"],
                                               info["canonical_scale"])).to(dev)
    settings = teacher.settings._replace(cls_mean_size=teacher._cms)
    out = {}
    for R in (50, 100):
        rows = torch.from_numpy(generated_rows(BATCH, R)).to(dev)
        count = torch.full((BATCH,), R, dtype=torch.int32, device=dev)
        frames = torch.arange(BATCH, dtype=torch.int32, device=dev)
        memory = LabelMemory(list(range(BATCH)), SLOTS, 0.5, 0.5, 0.0, dev)
        merged = memory.merge(rows, count, frames)
        fused = fuse_rows_device(rows, count, geom, 0.5, "seed", 1)
        encoded = encode_targets(rows, count, records, settings)
        kernels = [("mono_memory_merge_f64", lambda: memory.merge(rows, count, frames, out=merged)),
                   ("mono_fuse_dets_f64", lambda: fuse_rows_device(rows, count, geom, 0.5, "seed", 1, *fused)),
                   ("mono_encode_targets_f64", lambda: encode_targets(rows, count, records, settings, out=encoded))]
        for _, fn in kernels * 3:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in kernels}
        for r in range(5):
            for name, fn in (kernels if r % 2 == 0 else kernels[::-1]):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(reps):
                    fn()
                end.record()
                end.synchronize()
                times[name].append(start.elapsed_time(end) * 1e3 / reps)
        out["R=%d" % R] = {name: base._spread(xs) for name, xs in times.items()}
        out["R=%d" % R]["stats_of_a_launch"] = merged[2].sum(0).tolist()
    return out


def step_ab(trainers, raw, steps):
    """ms per optimizer step, memory off / on alternated, every step between two device synchronisations."""
    def step(t):
        t.train_cycle([raw], t._teacher_turn())
    for _ in range(4):
        for t in trainers.values():
            step(t)
    times = {k: [] for k in trainers}
    for _ in range(steps):
        for k, t in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(t)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the bench.py comparison")
    ap.add_argument("--skip-steps", action="store_true", help="kernels (and --parent) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacher_memory_ab_%s.json" % datetime.date.today().isoformat()))
    args = ap.parse_args()
    from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
    from monosowa_amd.helpers.model_helper import build_model
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.helpers.trainer_helper import Trainer
    from monosowa_amd.synthetic import make_batch
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    tmp = tempfile.TemporaryDirectory()
    dataset = dict(base.fixture_root(tmp.name), type="KITTI", device_aug=True, batch_size=BATCH, unlabelled_split="distinct")
    # the memory names every frame once per batch: a split of the fixture's six frames under 96 names each would repeat them, so the
    # frames are linked under distinct names
    ids = [int(x) for x in open(os.path.join(tmp.name, "ImageSets", "unlabelled.txt")).read().split()[:6]]
    names = []
    for k in range(6 * BATCH):
        name = "%06d" % (1000 + k)
        for sub, ext in (("image_2", ".png"), ("calib", ".txt")):
            os.symlink(os.path.join(tmp.name, "training", sub, "%06d%s" % (ids[k % 6], ext)), os.path.join(tmp.name, "training", sub, name + ext))
        names.append(name)
    with open(os.path.join(tmp.name, "ImageSets", "distinct.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    result = {"batch": BATCH, "resolution": [1280, 384], "slots": SLOTS}
    trainers, teachers = {}, {}
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    raw = (inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in targets.items()}, info)
    torch.manual_seed(0)
    model0, crit0 = build_model(cfg["model"])
    for key in ("memory_off", "memory_on"):
        trainer_cfg = dict(cfg["trainer"], teacher={"min_score": 0.3, "source": "model"})
        if key == "memory_on":
            trainer_cfg["teacher_memory"] = {"slots": SLOTS}
        whole = {"dataset": dataset, "tester": {"type": "KITTI", "topk": 50, "threshold": 0.0, "nms_iou": 0.5}, "model": cfg["model"],
                 "trainer": trainer_cfg}
        model, crit = copy.deepcopy(model0).to(dev), copy.deepcopy(crit0).to(dev)
        opt = build_optimizer(cfg["optimizer"], model)
        teachers[key] = Teacher(whole, model, dev, loader=build_unlabelled_loader(dataset, workers=4))
        trainers[key] = Trainer(trainer_cfg, model, opt, base._Loader(), None, None, None, logging.getLogger("teacher_memory_ab"), crit,
                                "teacher_memory_ab", teacher=teachers[key])
        trainers[key].model.train()
        crit.train()
        if args.skip_steps:
            break
    if not args.skip_steps:
        times = step_ab(trainers, raw, args.steps)
        for key, xs in times.items():
            result["ms_per_step_" + key] = base._spread(xs)
        result["memory_on_over_off"] = result["ms_per_step_memory_on"]["median"] / result["ms_per_step_memory_off"]["median"]
        result["memory_counts_last_cycle"] = list(trainers["memory_on"]._memory_counts)
        rows, count = teachers["memory_on"].last_rows           # what the shipped, untrained model gave the memory last
        kept = rows[np.arange(rows.shape[1])[None, :] < count[:, None]]
        result["rows_last_batch"] = {"rows": int(len(kept)), "finite": int(np.isfinite(kept).all(1).sum()),
                                     "sides_above_zero": int(((kept[:, 7] > 0) & (kept[:, 8] > 0)).sum()),
                                     "max_abs_x_z": float(np.abs(kept[:, [9, 11]]).max()) if len(kept) else 0.0}
    first = next(iter(teachers.values()))
    result["us_per_launch"] = kernel_times(first, first.next_raw(), args.reps)
    for t in teachers.values():
        t.close()
    if args.parent:
        del trainers, teachers
        torch.cuda.empty_cache()
        got = base.bench_ab(args.parent)
        result["bench_train_parent"], result["bench_train_tree"] = base._spread(got["parent"]), base._spread(got["tree"])
        p, t = result["bench_train_parent"], result["bench_train_tree"]
        result["tree_median_inside_parent_min_max"] = bool(p["min"] <= t["median"] <= p["max"])
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
