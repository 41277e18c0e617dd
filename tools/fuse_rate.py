"""What tester.nms_iou / flip_tta cost (README "Duplicate suppression and flip consistency").

    python tools/fuse_rate.py [--images 512 --batch 16 --rounds 3] [--parent PATH] [--out profiles/NAME.json]

1. ``Detector.detect`` img/s by tools/eval_rate.py's protocol (the shipped model, tools/loader_rate.py's 1242 x 375 frames held in
   memory, a warm-up pass, then ``--rounds`` timed passes ended by a device synchronise) with the keys absent, with ``nms_iou`` alone
   and with ``flip_tta``.  The shipped model is untrained and keeps no row above the protocol's ``threshold: 0.2``, so the two keyed
   legs (and a keys-absent one) run a second time with ``threshold: 0.0``, where every image hands all 50 rows per view to the
   fuse.  Every leg is a fresh process.  With ``--parent PATH`` (a built checkout of the parent commit) the
   keys-absent leg alternates that tree and this one three times, and the result says whether this tree's median lies inside the
   parent's own min-max spread.
2. Device time of ``mono_fuse_dets_f64`` at B = 16, K = 50, V = 1 and 2 -- an event pair around 20 back-to-back launches, the
   median of 5 pairs -- beside ``mono_decode_dets_f64`` measured the same way on the same detections.

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"absent": {}, "nms_iou": {"nms_iou": 0.5}, "flip_tta": {"nms_iou": 0.5, "flip_tta": True, "fuse": "mean"}}


def summary(values):
    return {"values": values, "median": statistics.median(values), "min": min(values), "max": max(values)}


def child(args):
    """One leg in the tree ``--tree``: prints {"img_per_s": [...], "rows_per_image": x}."""
    sys.path.insert(0, args.tree)
    sys.path.insert(0, os.path.join(args.tree, "tools"))
    import torch
    import yaml
    from loader_rate import P2, dataset_cfg, make_image
    from monosowa_amd import Detector
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    dev = torch.device("cuda", 0)
    with open(os.path.join(args.tree, "configs", "monodetr.yaml")) as f:
        cfg = yaml.safe_load(f)
    torch.manual_seed(0)
    model, _ = build_model(dict(cfg["model"], device="cuda"))
    model = to_mi355x_layout(model.to(dev)).eval()
    rng = np.random.default_rng(0)
    distinct = [make_image(rng, 1242, 375) for _ in range(min(args.distinct, args.images))]
    frames = [distinct[i % len(distinct)] for i in range(args.images)]
    cameras = np.broadcast_to(P2, (args.images, 3, 4))
    det = Detector({"dataset": dataset_cfg("unused", False, False, args.batch), "tester": dict({"topk": 50, "threshold": args.threshold}, **LEGS[args.child]),
                    "model": cfg["model"]}, model=model)
    det.detect(frames[:2 * args.batch], cameras[:2 * args.batch], batch_size=args.batch)
    rates, kept = [], 0
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = det.detect(frames, cameras, batch_size=args.batch)
        torch.cuda.synchronize()
        rates.append(args.images / (time.perf_counter() - t0))
        kept = sum(len(r) for r in rows) / args.images
    det.close()
    print("RESULT " + json.dumps({"img_per_s": rates, "rows_per_image": kept}))


def run_leg(args, leg, tree, threshold=0.2):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--tree", tree, "--images", str(args.images), "--batch", str(args.batch),
           "--rounds", str(args.rounds), "--distinct", str(args.distinct), "--threshold", str(threshold)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode:
        raise RuntimeError("leg %s in %s failed (%d):\n%s" % (leg, tree, out.returncode, out.stderr[-2000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def kernel_times(launches=20, pairs=5):
    """us per launch of the decode and the fuse kernel at B = 16, K = 50 on the same random detections."""
    sys.path.insert(0, ROOT)
    import torch
    from monosowa_amd.fuse import fuse_rows_device
    from monosowa_amd.kitti_eval import decode_dets_device
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    B, K = 16, 50
    dets = np.zeros((2 * B, K, 37), dtype=np.float32)
    dets[..., 0] = rng.integers(0, 3, (2 * B, K))
    dets[..., 1] = np.sort(rng.uniform(0.3, 0.98, (2 * B, K)).astype(np.float32), axis=1)[:, ::-1]
    dets[..., 2:4] = rng.uniform(0.3, 0.7, (2 * B, K, 2))                 # crowded on purpose: most same-class pairs reach the clipping
    dets[..., 4:6] = rng.uniform(0.05, 0.3, (2 * B, K, 2))
    dets[..., 6] = rng.uniform(15, 30, (2 * B, K))
    dets[..., 7:19] = rng.normal(0, 2, (2 * B, K, 12))
    dets[..., 19:31] = rng.uniform(-0.6, 0.6, (2 * B, K, 12))
    dets[..., 31:34] = np.array([1.5, 1.7, 4.0]) + rng.normal(0, 0.1, (2 * B, K, 3))
    dets[..., 34:36] = dets[..., 2:4]
    dets[..., 36] = rng.uniform(0.5, 1.0, (2 * B, K))
    geom = np.tile(np.array([[1242, 375, 1.0, 1.0, 609.5593, 172.854, 721.5377, 721.5377, 0.06, 0.0]]), (B, 1))
    dets, geom = torch.from_numpy(dets).to(dev), torch.from_numpy(geom).to(dev)
    cms = torch.zeros((3, 3), dtype=torch.float64, device=dev)
    out = {}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(pairs):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(launches):
                fn()
            end.record()
            end.synchronize()
            us.append(start.elapsed_time(end) * 1e3 / launches)
        return summary(us)

    for V in (1, 2):
        d, g = dets[:V * B].contiguous(), torch.cat([geom] * V)
        rows, count = decode_dets_device(d, g, cms, 0.2)
        out["mono_decode_dets_f64, %d images" % (V * B)] = timed(lambda: decode_dets_device(d, g, cms, 0.2, rows, count))
        for mode in ("seed", "mean"):
            o = fuse_rows_device(rows, count, geom, 0.5, mode, V)
            out["mono_fuse_dets_f64, V = %d, %s" % (V, mode)] = timed(lambda: fuse_rows_device(rows, count, geom, 0.5, mode, V, *o))
            torch.cuda.synchronize()
            out["rows kept of %d candidates, V = %d, %s" % (V * K, V, mode)] = float(o[1].float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=64, help="distinct frames generated; the pass cycles through them")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit, alternated with this tree for the keys-absent leg")
    ap.add_argument("--child", default="")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--threshold", type=float, default=0.2)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)

    out = {"images": args.images, "batch": args.batch, "rounds": args.rounds, "detect_img_per_s": {}}
    absent = {"tree": [], "parent": []}
    for _ in range(3 if args.parent else 1):                             # alternated: parent, tree, parent, tree, ...
        for which, tree in ((("parent", args.parent),) if args.parent else ()) + (("tree", ROOT),):
            absent[which] += run_leg(args, "absent", tree)["img_per_s"]
    out["detect_img_per_s"]["keys absent, this tree"] = summary(absent["tree"])
    if args.parent:
        out["detect_img_per_s"]["keys absent, parent commit"] = summary(absent["parent"])
        out["tree_median_inside_the_parents_spread"] = min(absent["parent"]) <= statistics.median(absent["tree"]) <= max(absent["parent"])
    for threshold, legs in ((0.2, ("nms_iou", "flip_tta")), (0.0, ("absent", "nms_iou", "flip_tta"))):
        for leg in legs:
            res = run_leg(args, leg, ROOT, threshold)
            out["detect_img_per_s"]["threshold %g, %s %s" % (threshold, leg, json.dumps(LEGS[leg]))] = dict(
                summary(res["img_per_s"]), rows_per_image=res["rows_per_image"])
    out["kernel_us_per_launch"] = kernel_times()                        # (this process opens the GPU only now, after the legs' processes)
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
