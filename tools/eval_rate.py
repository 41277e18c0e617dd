"""What a whole evaluation pass delivers, and what the public Detector delivers (README "Detector").

    python tools/eval_rate.py [--images 512 --batch 16 --workers 4 --rounds 3] [--out profiles/NAME.json]
                              [--tester-file PATH]       another revision's tester_helper.py, alternated with the tree's (A/B)

On a seeded generated KITTI directory (tools/loader_rate.py's 1242 x 375 PNGs) with the shipped model, ``dataset.device_aug`` on
and off, every round measures

    wall-clock images / s of a whole ``Tester.inference()`` pass (loader start, forward, decode, result files), ended by a device
    synchronise;
    the model-only rate the pass reports (``last_img_per_s``);
    how long the pass waited for its DataLoader -- until the first batch (worker start-up), in all, and for its shutdown;
    ``Detector.detect`` over the same frames held in memory.

A warm-up pass of every leg comes first.  Prints one JSON line (per-round values, medians and min-max spread) and writes it
to --out."""
import argparse
import importlib.util
import json
import logging
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from loader_rate import P2, dataset_cfg, write_kitti_dir      # noqa: E402


def tester_class(path):
    """``Tester`` of the tree, or of another revision's tester_helper.py loaded beside it (its relative imports resolve here)."""
    if not path:
        from monosowa_amd.helpers.tester_helper import Tester
        return Tester
    import monosowa_amd.helpers  # noqa: F401
    spec = importlib.util.spec_from_file_location("monosowa_amd.helpers.tester_helper_other", path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module.Tester


class TimedLoader:
    """A DataLoader as the Tester sees it (``len``, ``dataset``, iteration) that records how long the consumer waited for it:
    until the first batch (worker start-up and the first decode), in all, and for the exhausted iterator to shut its workers down."""

    def __init__(self, loader):
        self.loader, self.dataset = loader, loader.dataset
        self.first = self.waited = self.closing = 0.0

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        t0 = time.perf_counter()
        it = iter(self.loader)
        n = 0
        while True:
            try:
                batch = next(it)
            except StopIteration:                                        # the exhausted iterator has shut its workers down by now
                self.closing = time.perf_counter() - t0
                break
            now = time.perf_counter()
            self.waited += now - t0
            if n == 0:
                self.first = now - t0
            n += 1
            yield batch
            t0 = time.perf_counter()


def summary(values):
    return {"values": values, "median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tester-file", default="")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    import yaml
    from PIL import Image
    from monosowa_amd import Detector
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    dev = torch.device("cuda", 0)
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        cfg = yaml.safe_load(f)
    torch.manual_seed(0)
    model, _ = build_model(dict(cfg["model"], device="cuda"))
    model = to_mi355x_layout(model.to(dev)).eval()
    testers = {"tree": tester_class("")}
    if args.tester_file:
        testers["other"] = tester_class(args.tester_file)
    logger = logging.getLogger("eval_rate")
    out = {"images": args.images, "batch": args.batch, "workers": args.workers, "rounds": args.rounds, "tester_file": args.tester_file,
           "device": torch.cuda.get_device_name(0), "inference_pass": {}, "detector": {}}

    with tempfile.TemporaryDirectory() as root:
        write_kitti_dir(root, args.images)

        def one_pass(which, device_aug):
            loader = TimedLoader(build_dataloader(dataset_cfg(root, False, device_aug, args.batch), workers=args.workers)[1])
            tester = testers[which]({"type": "KITTI", "topk": 50, "threshold": 0.2}, model, loader, logger, {"save_path": "unused/"}, "m")
            tester.output_dir = os.path.join(root, "results_" + which)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results = tester.inference()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            assert len(results) == args.images
            return {"img_per_s_end_to_end": args.images / wall, "img_per_s_model_only": tester.last_img_per_s,
                    "img_per_s_after_the_first_batch": (args.images - args.batch) / (wall - loader.first),
                    "seconds_to_the_first_batch": loader.first, "fraction_waiting_for_the_loader": loader.waited / wall,
                    "seconds_closing_the_loader": loader.closing, "seconds": wall}

        legs = [(which, flag) for flag in (True, False) for which in testers]
        raw = {leg: [] for leg in legs}
        for leg in legs:
            one_pass(*leg)                                               # warm-up: MIOpen / hipBLASLt first use, page cache
        for _ in range(args.rounds):
            for leg in legs:                                             # alternated
                raw[leg].append(one_pass(*leg))
        for (which, flag), passes in raw.items():
            out["inference_pass"]["%s, device_aug %s" % (which, "on" if flag else "off")] = {
                key: summary([p[key] for p in passes]) for key in passes[0]}

        frames = [np.array(Image.open(os.path.join(root, "training", "image_2", "%06d.png" % i))) for i in range(args.images)]
        cameras = np.broadcast_to(P2, (args.images, 3, 4))
        det = Detector({"dataset": dataset_cfg(root, False, False, args.batch), "tester": {"topk": 50, "threshold": 0.2}, "model": cfg["model"]},
                       model=model)
        det.detect(frames[:2 * args.batch], cameras[:2 * args.batch], batch_size=args.batch)
        rates = []
        for _ in range(args.rounds):
            seconds0, images0 = det.engine.model_seconds, det.engine.images
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = det.detect(frames, cameras, batch_size=args.batch)
            torch.cuda.synchronize()
            rates.append(args.images / (time.perf_counter() - t0))
            assert len(rows) == args.images
            out["detector"].setdefault("img_per_s_model_only", []).append(
                (det.engine.images - images0) / max(det.engine.model_seconds - seconds0, 1e-9))
        out["detector"]["img_per_s_end_to_end"] = summary(rates)
        out["detector"]["img_per_s_model_only"] = summary(out["detector"]["img_per_s_model_only"])
        det.close()

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
