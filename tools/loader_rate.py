"""What the KITTI loader costs and what dataset.device_aug buys (README "Image preparation on the GPU").

    python tools/loader_rate.py host   [--images 48]              ms per sample by stage on this machine's CPUs, flag off and on
    python tools/loader_rate.py kernel [--launches 200]           image_prep's launch per batch of 16, from device events
    python tools/loader_rate.py train  [--steps 40 --workers 4]   train steps fed by build_dataloader(type KITTI), flag off / on

Every mode works on a seeded generated KITTI directory of 1242 x 375 PNGs (smooth content plus noise, like camera images to a
PNG encoder) in a temporary folder, prints one JSON line and, with --out, writes it to a file as well."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
HBM_PEAK = 8.0e12                      # bytes / s, MI355X


def make_image(rng, w, h):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    chans = [127.5 + 100 * np.sin(xx / rng.uniform(30, 120) + yy / rng.uniform(20, 80) + rng.uniform(0, 6.28)) for _ in range(3)]
    return np.clip(np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def write_kitti_dir(root, n, samples=None, size=(1242, 375), seed=0):
    """n images with calibration and 2-5 projected cars each: ImageSets/train.txt + val.txt, training/{image_2, calib, label_2}.
    The split lists name ``samples`` entries (default n), cycling through the images, so that one epoch outlasts a timed leg."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for sub in ("ImageSets", "training/image_2", "training/calib", "training/label_2"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    row = lambda tag, m: tag + ": " + " ".join("%.6e" % v for v in np.asarray(m).reshape(-1))
    calib = "\n".join([row("P0", P2), row("P1", P2), row("P2", P2), row("P3", P2), row("R0_rect", np.eye(3)),
                       row("Tr_velo_to_cam", np.eye(3, 4)), row("Tr_imu_to_velo", np.eye(3, 4))]) + "\n"
    for i in range(n):
        Image.fromarray(make_image(rng, *size)).save(os.path.join(root, "training/image_2/%06d.png" % i))
        with open(os.path.join(root, "training/calib/%06d.txt" % i), "w") as f:
            f.write(calib)
        lines = []
        for _ in range(int(rng.integers(2, 6))):
            z, x = rng.uniform(8, 50), rng.uniform(-0.35, 0.35)
            x, y, (h, w, l) = x * z, 1.65, (1.5, 1.6, 3.9)
            u, v = P2[0, 0] * x / z + P2[0, 2], P2[1, 1] * (y - h / 2) / z + P2[1, 2]
            du, dv = P2[0, 0] * l / z / 2, P2[1, 1] * h / z / 2
            box = (max(u - du, 0), max(v - dv, 0), min(u + du, size[0] - 1), min(v + dv, size[1] - 1))
            lines.append("Car 0.00 0 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f"
                         % ((rng.uniform(-1.5, 1.5),) + box + (h, w, l, x, y, z, rng.uniform(-1.5, 1.5))))
        with open(os.path.join(root, "training/label_2/%06d.txt" % i), "w") as f:
            f.write("\n".join(lines) + "\n")
    for split in ("train", "val"):
        with open(os.path.join(root, "ImageSets", split + ".txt"), "w") as f:
            f.write("\n".join("%06d" % (i % n) for i in range(samples or n)) + "\n")


def dataset_cfg(root, aug_pd, device_aug, batch_size=16):
    return {"type": "KITTI", "root_dir": root, "train_split": "train", "test_split": "val", "batch_size": batch_size, "use_3d_center": True,
            "class_merging": False, "use_dontcare": False, "bbox2d_type": "anno", "meanshape": False, "writelist": ["Car"],
            "clip_2d": False, "aug_pd": aug_pd, "aug_crop": True, "random_flip": 0.5, "random_crop": 0.5, "scale": 0.05, "shift": 0.05,
            "depth_scale": "normal", "device_aug": device_aug}


def host(args, root):
    """ms per sample: the stages of the default mode timed one by one with the product's classes, then whole __getitem__
    calls and the collate of a batch of 16, flag off and on."""
    from PIL import Image
    from torch.utils.data import default_collate
    from monosowa_amd.image_prep import collate_raw
    from monosowa_amd.kitti_dataset import KITTI_Dataset, get_affine_transform
    out = {"mode": "host", "images": args.images, "cpus_visible": os.cpu_count(), "stages_ms": {}, "getitem_ms": {}, "collate16_ms_per_sample": {}}
    ds = KITTI_Dataset("train", dataset_cfg(root, True, False))
    t = {"decode": 0.0, "photometric + astype(uint8)": 0.0, "flip + transform": 0.0, "normalise + transpose": 0.0, "np.array(raw)": 0.0}
    np.random.seed(0)
    for i in range(args.images):
        t0 = time.perf_counter()
        img = ds.get_image(i)
        img.load()
        t1 = time.perf_counter()
        raw = np.array(img)
        t2 = time.perf_counter()
        pd_img = Image.fromarray(ds.pd(raw.astype(np.float32)).astype(np.uint8))
        t3 = time.perf_counter()
        size = np.array(img.size)
        _, inv = get_affine_transform(size / 2, size, 0, ds.resolution, inv=1)
        res = pd_img.transpose(Image.FLIP_LEFT_RIGHT).transform(tuple(ds.resolution.tolist()), method=Image.AFFINE,
                                                                data=tuple(inv.reshape(-1).tolist()), resample=Image.BILINEAR)
        t4 = time.perf_counter()
        ((np.array(res).astype(np.float32) / 255.0 - ds.mean) / ds.std).transpose(2, 0, 1)
        t5 = time.perf_counter()
        for k, d in zip(t, (t1 - t0, t3 - t2, t4 - t3, t5 - t4, t2 - t1)):
            t[k] += d
    out["stages_ms"] = {k: v / args.images * 1e3 for k, v in t.items()}
    for aug_pd in (False, True):
        for flag in (False, True):
            ds = KITTI_Dataset("train", dataset_cfg(root, aug_pd, flag))
            np.random.seed(1)
            t0 = time.perf_counter()
            samples = [ds[i] for i in range(args.images)]
            key = "aug_pd %s, device_aug %s" % ("on" if aug_pd else "off", "on" if flag else "off")
            out["getitem_ms"][key] = (time.perf_counter() - t0) / args.images * 1e3
            t0 = time.perf_counter()
            for _ in range(3):
                (collate_raw if flag else default_collate)(samples[:16])
            out["collate16_ms_per_sample"][key] = (time.perf_counter() - t0) / 3 / 16 * 1e3
    return out


def kernel(args, root):
    import torch
    from monosowa_amd._lib import raw_stream
    from monosowa_amd.image_prep import MEAN, STD, _device_lut, load, make_record, prepare
    from monosowa_amd.kitti_dataset import get_affine_transform
    from monosowa_amd.photometric import PhotometricDistort
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    out = {"mode": "kernel", "batch": 16, "launches": args.launches, "cases": {}}
    for size in ((1242, 375), (1920, 1280)):
        img = make_image(rng, *size)
        raw = torch.from_numpy(np.stack([np.roll(img, 37 * i, axis=1) for i in range(16)])).to(dev)
        for aug_pd in (False, True):
            recs = []
            np.random.seed(3)
            for i in range(16):
                pd = PhotometricDistort().draw() if aug_pd else None
                scale = float(np.clip(np.random.randn() * 0.05 + 1, 0.95, 1.05))
                s = np.array(size)
                _, inv = get_affine_transform(s / 2 + s * np.clip(np.random.randn(2) * 0.05, -0.1, 0.1), s * scale, 0, np.array([1280, 384]), inv=1)
                recs.append(make_record(size, inv, i % 2 == 1, pd))
            rec = torch.from_numpy(np.stack(recs)).to(dev)
            y = prepare(raw, rec, dev)
            # the launch alone, straight through the C ABI into the same output: the host side of prepare() (allocation, argument
            # checks) would otherwise sit between two events of a sub-millisecond kernel
            lut, stream = _device_lut(dev, MEAN, STD), raw_stream()
            launch = lambda: load().mono_image_prep_f32(raw.data_ptr(), rec.data_ptr(), lut.data_ptr(), y.data_ptr(), 16, size[1], size[0],
                                                        384, 1280, stream)
            for _ in range(10):
                assert launch() == 0
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.launches + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(args.launches):
                launch()
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.launches))
            touched = raw.numel() + y.numel() * 4                        # raw bytes read once + 4 * B * 3 * H * W written
            out["cases"]["%dx%d, aug_pd %s" % (size + ("on" if aug_pd else "off",))] = {
                "ms_median": ms[len(ms) // 2], "ms_p10": ms[len(ms) // 10], "ms_p90": ms[len(ms) * 9 // 10], "bytes": touched,
                "ms_at_hbm_peak": touched / HBM_PEAK * 1e3}
    return out


def train(args, root):
    import torch
    import yaml
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import prepare_targets
    dev = torch.device("cuda", 0)
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        cfg = yaml.safe_load(f)
    torch.manual_seed(0)
    model, crit = build_model(dict(cfg["model"], device="cuda"))
    model = to_mi355x_layout(model.to(dev)).train()
    crit = crit.to(dev).train()
    opt = build_optimizer(cfg["optimizer"], model)
    B = args.batch

    def step(batch):
        inputs, calibs, targets, info = batch
        tl = prepare_targets(targets, B)
        opt.zero_grad(set_to_none=True)
        weighted_total(crit(model(inputs, calibs, tl, targets["img_size"]), tl), crit.weight_dict).backward()
        opt.step()

    def fed(aug_pd, flag):
        loader, _ = build_dataloader(dataset_cfg(root, aug_pd, flag, B), workers=args.workers, drop_last=True, test=False)
        it, n, t0 = iter(loader), 0, None
        for k in range(args.warm + args.steps):
            step(stage_batch(next(it), dev))
            if k == args.warm - 1:               # the workers' prefetch queues (2 batches each, filled while the first step ran) have
                torch.cuda.synchronize()         # drained to their steady state by now: a loader-bound leg shows the loader's rate
                t0 = time.perf_counter()
            elif k >= args.warm:
                n += B
        torch.cuda.synchronize()
        rate = n / (time.perf_counter() - t0)
        del it, loader
        return rate

    out = {"mode": "train", "batch": B, "workers": args.workers, "steps": args.steps, "warm_steps": args.warm, "images": args.images,
           "img_per_s": {}}
    loader, _ = build_dataloader(dataset_cfg(root, False, True, B), workers=0, drop_last=True, test=False)
    resident = stage_batch(next(iter(loader)), dev)
    for _ in range(3):
        step(resident)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(resident)
    torch.cuda.synchronize()
    out["img_per_s"]["resident batch"] = args.steps * B / (time.perf_counter() - t0)
    for aug_pd in (True, False):
        for flag in (False, True, False, True):                          # alternated; the second pair shows the spread
            key = "aug_pd %s, device_aug %s" % ("on" if aug_pd else "off", "on" if flag else "off")
            out["img_per_s"].setdefault(key, []).append(fed(aug_pd, flag))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["host", "kernel", "train"])
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40, help="timed train steps per leg")
    ap.add_argument("--warm", type=int, default=24, help="untimed steps before them (train mode)")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        if args.mode != "kernel":
            write_kitti_dir(root, args.images, max(args.images, (args.warm + args.steps + 1) * args.batch) if args.mode == "train" else None)
        result = {"host": host, "kernel": kernel, "train": train}[args.mode](args, root)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
