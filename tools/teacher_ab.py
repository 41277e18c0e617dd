"""Cost of the mean teacher (``trainer.teacher``), measured inside ONE process (the method of tools/ema_ab.py), shipped model, batch 16,
1280 x 384:

1. the train step with the key off (one labelled batch) / on (the same batch plus one pseudo-labelled micro-batch, the teacher one
   cycle ahead), alternating, ``--steps`` each; every step timed with a device sync; median and min-max per setting.  Then ``--steps``
   consecutive cycles with the key on and no synchronisation between them, as the train loop runs them: the host time inside
   ``collect()``'s event wait per cycle, the host time of the rest of the cycle, and the wall time per cycle.  The event sits on the
   training stream in front of the previous cycle's kernels, so the wait is the host's lead over the device; the one-cycle lookahead
   hides the teacher when the wall time per cycle is the synchronised step's, i.e. when the device is never left waiting.
2. the device time of ``mono_encode_targets_f64`` from event pairs around ``--reps`` back-to-back launches, beside
   ``mono_decode_dets_f64`` at the same 16 x 50 rows.
3. the wall time of ``encode_targets_host`` for the same rows.
4. with ``--parent DIR`` (a built checkout of the parent commit): ``bench.py``'s train leg, parent and this tree alternated three times;
   this tree's median against the parent's own spread.

The unlabelled frames are the six of tests/golden/kitti_dataset.npz, repeated to fill the batch, unless ``--root`` names a KITTI
directory with ``ImageSets/<--split>.txt``.

    python tools/teacher_ab.py [--steps 20] [--reps 20] [--parent DIR] [--out profiles/teacher_ab_<date>.json]

One JSON line on stdout (and in --out)."""
import argparse
import datetime
import json
import logging
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monosowa_amd import miopen_tuning   # noqa: E402
miopen_tuning.use_shipped_db(0)

import numpy as np   # noqa: E402
import torch   # noqa: E402
import yaml    # noqa: E402

from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader   # noqa: E402
from monosowa_amd.helpers.model_helper import build_model   # noqa: E402
from monosowa_amd.helpers.optimizer_helper import build_optimizer  # noqa: E402
from monosowa_amd.helpers.trainer_helper import Trainer   # noqa: E402
from monosowa_amd.kitti_eval import decode_dets_device   # noqa: E402
from monosowa_amd.synthetic import make_batch    # noqa: E402
from monosowa_amd.teacher import Teacher, encode_targets, encode_targets_host, student_records   # noqa: E402

BATCH = 16


class _Loader:
    batch_size = BATCH

    def __len__(self):
        return 1


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def fixture_root(path):
    """The synthetic KITTI directory of the test fixture under ``path``, its six frames repeated to fill a batch."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "kitti_dataset.npz"), allow_pickle=False)
    for i, name in enumerate(g["file_names"]):
        p = os.path.join(path, str(name))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(g["file_%03d" % i].tobytes())
    ids = ["%06d" % int(i) for i in g["ids"]]
    with open(os.path.join(path, "ImageSets", "unlabelled.txt"), "w") as f:
        f.write("\n".join(ids[k % len(ids)] for k in range(96 * BATCH)) + "\n")      # one pass outlasts the run: no loader restart
    return dict(json.loads(str(g["cfg_json"])), root_dir=path)


class _TimedComplete:
    """``engine.complete_oldest`` with the host ms of every call in ``calls`` and, of those, the ms inside the slot event's
    ``synchronize()`` in ``events``."""

    def __init__(self, engine):
        self.engine, self.complete, self.calls, self.events = engine, engine.complete_oldest, [], []
        self.event_wait = torch.cuda.Event.synchronize
        self.inside = False

    def __enter__(self):
        timed = self

        def complete():
            timed.inside = True
            t = time.perf_counter()
            try:
                return timed.complete()
            finally:
                timed.calls.append((time.perf_counter() - t) * 1e3)
                timed.inside = False

        def event_wait(event):
            if not timed.inside:
                return timed.event_wait(event)
            t = time.perf_counter()
            timed.event_wait(event)
            timed.events.append((time.perf_counter() - t) * 1e3)
        self.engine.complete_oldest = complete
        torch.cuda.Event.synchronize = event_wait
        return self

    def __exit__(self, *exc):
        self.engine.complete_oldest = self.complete
        torch.cuda.Event.synchronize = self.event_wait


def wait_ab(trainer, raw, steps):
    """``steps`` consecutive cycles with the key on and NO synchronisation between them, as the train loop runs them (one at the
    end): per cycle the host ms inside ``collect()``'s ``complete_oldest`` and, of that, inside the slot event's wait; the host ms of
    the rest of the cycle (refresh check, submit, every launch of the cycle); and the wall ms per cycle of the whole run.  The event
    was recorded on the training stream in front of the previous cycle's kernels, so the wait is the lead the host had over the device
    at the top of the cycle; the device starves only if the wall ms per cycle exceed the synchronised step's."""
    for _ in range(4):
        trainer.train_cycle([raw], trainer._teacher_turn())
    torch.cuda.synchronize()
    host = []
    with _TimedComplete(trainer.teacher.engine) as timed:
        start = time.perf_counter()
        for _ in range(steps):
            t = time.perf_counter()
            trainer.train_cycle([raw], trainer._teacher_turn())
            host.append((time.perf_counter() - t) * 1e3)
        enqueued = time.perf_counter()
        torch.cuda.synchronize()
        end = time.perf_counter()
    # (a batch that was ready inside submit() is handed back there and never waited for: "n" below says how many cycles waited)
    return {"ms_in_complete_oldest": _spread(timed.calls or [0.0]), "ms_in_slot_event_wait": _spread(timed.events or [0.0]),
            "ms_host_per_cycle": _spread(host), "ms_host_per_cycle_outside_complete_oldest": (sum(host) - sum(timed.calls)) / steps,
            "ms_wall_per_cycle": (end - start) * 1e3 / steps, "ms_final_synchronize": (end - enqueued) * 1e3, "cycles": steps}


def step_ab(trainer, raw, steps):
    """ms per optimizer step with the key off / on, alternated, every step between two device synchronisations, and the ms inside
    collect()'s ``complete_oldest`` of every step with the key on.  Under that bracket the batch's event has always completed, so
    this figure is the call's own overhead (``elapsed_time`` and the host copies of rows, count and the pinned extras), not a wait:
    ``wait_ab`` measures the wait."""
    teacher = trainer.teacher
    waits = []
    complete = teacher.engine.complete_oldest

    def timed_complete():
        t = time.perf_counter()
        done = complete()
        waits.append((time.perf_counter() - t) * 1e3)
        return done
    teacher.engine.complete_oldest = timed_complete

    def step(on):
        if on:
            trainer.train_cycle([raw], trainer._teacher_turn())
        else:
            trainer.train_cycle([raw])
    for on in [False, True] * 4:
        step(on)
    torch.cuda.synchronize()
    del waits[:]
    times = {False: [], True: []}
    for i in range(2 * steps):
        on = bool(i & 1)
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(on)
        torch.cuda.synchronize()
        times[on].append((time.perf_counter() - t) * 1e3)
    teacher.engine.complete_oldest = complete
    return times, waits


def kernel_times(teacher, raw, reps, rounds=10):
    """us of device time per launch of the encode and of the decode at the teacher's own shape, and the ms of the host encode."""
    dev = teacher.device
    canvas, calibs, targets, info = raw
    B, K = canvas.shape[0], teacher.topk
    g = torch.Generator().manual_seed(0)
    dets = torch.rand((B, K, 37), generator=g)
    dets[:, :, 0] = torch.randint(0, 3, (B, K), generator=g).float()
    dets[:, :, 6] = dets[:, :, 6] * 60 + 2
    dets = dets.to(dev)
    _, geom, _ = teacher._teacher_view(calibs, targets["img_size"])
    geom = geom.to(dev)
    cms = teacher._cms
    rows, count = decode_dets_device(dets, geom, cms, teacher.threshold)
    records = torch.from_numpy(student_records(calibs, targets["img_size"], info["flip"], info["affine"], info["scale_depth"],
                                               info["canonical_scale"])).to(dev)
    settings = teacher.settings._replace(cls_mean_size=cms)
    out = encode_targets(rows, count, records, settings)
    kernels = [("mono_encode_targets_f64", lambda: encode_targets(rows, count, records, settings, out=out)),
               ("mono_decode_dets_f64", lambda: decode_dets_device(dets, geom, cms, teacher.threshold, rows=rows, count=count))]
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
    rows_h, count_h, records_h = rows.cpu().numpy(), count.cpu().numpy(), records.cpu().numpy()
    host = []
    for _ in range(5):
        t = time.perf_counter()
        encode_targets_host(rows_h, count_h, records_h, teacher.settings)
        host.append((time.perf_counter() - t) * 1e3)
    return times, host, int(count_h.sum())


def bench_ab(parent, rounds=3):
    """images/s of bench.py's train leg, parent checkout and this tree alternated."""
    def leg(root):
        root = os.path.abspath(root)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
               "--no-inference-leg", "--no-dataloader-leg", "--no-step-roofline", "--no-offsets-probe"]
        text = subprocess.run(cmd, cwd=root, capture_output=True, text=True, check=True, timeout=600).stdout
        line = json.loads([x for x in text.splitlines() if x.startswith("{")][-1])
        return line.get("value", line.get("images_per_s"))
    got = {"parent": [], "tree": []}
    for _ in range(rounds):
        got["parent"].append(leg(parent))
        got["tree"].append(leg(ROOT))
        print("bench.py train leg, images/s: parent %.2f, tree %.2f" % (got["parent"][-1], got["tree"][-1]), file=sys.stderr, flush=True)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed optimizer steps per setting")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per timed round")
    ap.add_argument("--root", default=None, help="a KITTI directory with ImageSets/<split>.txt (default: the test fixture's frames)")
    ap.add_argument("--split", default="unlabelled")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the bench.py comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "teacher_ab_%s.json" % datetime.date.today().isoformat()))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    tmp = tempfile.TemporaryDirectory()
    dataset = fixture_root(tmp.name) if args.root is None else dict(cfg["dataset"], root_dir=args.root)
    dataset = dict(dataset, type="KITTI", device_aug=True, batch_size=BATCH, unlabelled_split=args.split)
    whole = {"dataset": dataset, "tester": {"type": "KITTI", "topk": 50, "threshold": 0.0}, "model": cfg["model"],
             "trainer": dict(cfg["trainer"], teacher={"min_score": 0.0, "source": "model"})}
    model, crit = build_model(cfg["model"])
    model = model.to(dev)
    crit.to(dev)
    opt = build_optimizer(cfg["optimizer"], model)
    teacher = Teacher(whole, model, dev, loader=build_unlabelled_loader(dataset, workers=4))
    trainer = Trainer(whole["trainer"], model, opt, _Loader(), None, None, None, logging.getLogger("teacher_ab"), crit, "teacher_ab",
                      teacher=teacher)
    trainer.model.train()
    crit.train()
    inputs, calibs, targets, info = make_batch(BATCH, "cpu", seed=444)
    raw = (inputs.pin_memory(), calibs.pin_memory(), {n: t.pin_memory() for n, t in targets.items()}, info)
    result = {"batch": BATCH, "resolution": [1280, 384], "per_step": 1}
    steps, waits = step_ab(trainer, raw, args.steps)
    result.update({"ms_per_step_key_off": _spread(steps[False]), "ms_per_step_key_on": _spread(steps[True]),
                   "ms_in_complete_oldest_per_synchronised_step": _spread(waits), "pseudo_counts_last_batch": list(teacher.last_counts)})
    off, on = result["ms_per_step_key_off"]["median"], result["ms_per_step_key_on"]["median"]
    result["key_on_over_off"] = on / off
    result["consecutive_key_on_cycles_no_synchronize"] = wait_ab(trainer, raw, args.steps)
    kernels, host, n_rows = kernel_times(teacher, teacher.next_raw(), args.reps)
    for name, xs in kernels.items():
        result["us_per_launch_" + name] = _spread(xs)
    result["ms_encode_targets_host"] = _spread(host)
    result["rows_encoded"] = n_rows
    teacher.close()                          # the loader's workers end here
    if args.parent:
        del trainer, teacher, model, opt
        torch.cuda.empty_cache()
        got = bench_ab(args.parent)
        result["bench_train_parent"], result["bench_train_tree"] = _spread(got["parent"]), _spread(got["tree"])
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
