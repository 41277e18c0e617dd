"""Rate of the object-cloud stage (monosowa_amd/lift.py) at a KITTI-sized shape: 16 frames of 375 x 1242 with 8 synthetic masks each
(ellipses of about 60 x 60 to 200 x 120 px over objects 6 to 45 m away), then one gather of 8 tracks over the 16 frames.

    python tools/lift_rate.py [--frames 16] [--masks 8] [--host-seconds 60] [--out FILE.json]
    python tools/lift_rate.py --host-only [--out FILE.json]                                  (no GPU: lift_host alone)

Device time between event pairs around back-to-back ``lift`` calls, median of 5 after one warm-up; the four stages and the gather
between event pairs of their own in a second set of 5 calls.  The bytes a lift cannot avoid reading (the depth maps once, every mask
once) are set against a device-to-device copy, timed in the same run: of as many bytes (89 MB, which stay in the 256 MiB Infinity
Cache) and of 1 GiB buffers, whose rate is what HBM streams and is scaled to the lift's bytes.  ``lift_host`` is timed frame by frame on as
many of the frames as fit in ``--host-seconds``; the record says how many that was.  One JSON line on stdout, also written to
``--out`` (default ``profiles/lift_rate_<date>.json``)."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

H, W = 375, 1242
INTRINSICS = (721.5377, 721.5377, 609.5593, 172.854)


def frames(F, M, rng):
    """-> depth float32 [F, H, W], intrinsics [F, 4], masks bool [F, M, H, W], poses [F, 3, 4]: a road-like background (depth falling
    with the row), and per mask an ellipse with a noisy object plane painted a few pixels inside it."""
    v, u = np.mgrid[0:H, 0:W]
    depth = np.empty((F, H, W), dtype=np.float32)
    masks = np.zeros((F, M, H, W), dtype=bool)
    poses = np.tile(np.eye(3, 4), (F, 1, 1))
    for f in range(F):
        depth[f] = np.clip(1.65 * INTRINSICS[1] / np.maximum(v - INTRINSICS[3], 4.0), 3.0, 80.0) + rng.uniform(-0.05, 0.05, (H, W))
        poses[f, :, 3] = (rng.uniform(-0.2, 0.2), 0.0, 0.8 * (f - F // 2))
        for m in range(M):
            a, b = rng.uniform(30, 100), rng.uniform(30, 60)           # half axes: 60 .. 200 px wide, 60 .. 120 px high
            cu, cv = rng.uniform(a, W - a), rng.uniform(b + 40, H - b)
            inside = ((u - cu) / a) ** 2 + ((v - cv) / b) ** 2
            masks[f, m] = inside < 1.0
            core = inside < 0.85
            depth[f][core] = (rng.uniform(6, 45) + rng.uniform(-0.3, 0.3, int(core.sum()))).astype(np.float32)
    return depth, np.tile(np.array(INTRINSICS), (F, 1)), masks, poses


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--masks", type=int, default=8)
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_rate_%s.json" % datetime.date.today().isoformat()))
    args = ap.parse_args(argv)
    import torch
    from monosowa_amd.lift import ObjectLifter, lift_host, OK
    F, M = args.frames, args.masks
    depth, intr, masks, poses = frames(F, M, np.random.default_rng(0))
    cfg = {"frames_creation": {"nscans_before": F // 2}}
    tracks = [[(f, m) for f in range(F)] for m in range(M)]
    areas = masks.reshape(F * M, -1).sum(axis=1)
    bytes_per_frame = H * W * 4 + M * H * W
    out = {"frames": F, "masks_per_frame": M, "image": [H, W], "max_points": 16384, "mask_area_px": [int(areas.min()), int(areas.max())],
           "bytes_read_per_frame": bytes_per_frame}

    t0, done, host = time.perf_counter(), 0, []
    while done < F and time.perf_counter() - t0 < args.host_seconds:
        host.append(lift_host(depth[done:done + 1], intr[done:done + 1], masks[done:done + 1], None, poses[done:done + 1], cfg))
        done += 1
    seconds = time.perf_counter() - t0
    out["lift_host"] = {"frames_timed": done, "seconds": seconds, "ms_per_frame": 1e3 * seconds / done,
                        "note": "%d of the %d frames fitted into the %.0f s allowed" % (done, F, args.host_seconds)}

    if not args.host_only:
        dev = torch.device("cuda", torch.cuda.current_device())
        lifter = ObjectLifter(cfg, device=dev)
        d = [torch.from_numpy(a).to(dev) for a in (depth, intr, masks)] + [None, torch.from_numpy(poses).to(dev)]
        res = lifter.lift(*d)                                  # warm-up: the library, the allocator's blocks
        res.gather(tracks)
        torch.cuda.synchronize()
        assert not res.host

        def timed(call):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end)
        totals = [timed(lambda: lifter.lift(*d)) for _ in range(5)]
        gathers = [timed(lambda: res.gather(tracks)) for _ in range(5)]
        stages = {}
        for _ in range(5):
            lifter.timing = []
            lifter.lift(*d).gather(tracks)
            torch.cuda.synchronize()
            for name, start, end in lifter.timing:
                stages.setdefault(name, []).append(start.elapsed_time(end))
        lifter.timing = None
        src = torch.empty(F * bytes_per_frame, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        copies = [timed(lambda: dst.copy_(src)) for _ in range(5)]
        del src, dst
        # the same copy between buffers four times the 256 MiB Infinity Cache each: what HBM streams, scaled to the lift's bytes
        big_src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
        big_dst = torch.empty_like(big_src)
        big_dst.copy_(big_src)
        hbm_gb_per_s = (1 << 30) / (statistics.median([timed(lambda: big_dst.copy_(big_src)) for _ in range(5)]) * 1e6)
        del big_src, big_dst
        hbm_copy = F * bytes_per_frame / (hbm_gb_per_s * 1e6)
        total, copy = statistics.median(totals), statistics.median(copies)
        got = res.numpy()
        for f in range(done):                                  # the same answers as the host routine on the frames it timed
            want = host[f].numpy()
            assert all(np.array_equal(got[k][f], want[k][0]) for k in ("status", "counts", "total", "shrink"))
            assert np.array_equal(got["centres"][f].view(np.uint64), want["centres"][0].view(np.uint64))
        out.update({"device": torch.cuda.get_device_name(dev), "lift_ms": total, "lift_ms_runs": totals,
                    "lift_ms_per_frame": total / F, "stage_ms": {k: statistics.median(v) for k, v in stages.items()},
                    "gather_ms": statistics.median(gathers), "gather": {"tracks": M, "views": F, "max_views": 10, "max_points": 10000},
                    "copy_ms_same_bytes_cache_resident": copy, "copy_gb_per_s_cache_resident": F * bytes_per_frame / (copy * 1e6),
                    "copy_gb_per_s_hbm_1gib": hbm_gb_per_s, "copy_ms_same_bytes_at_hbm_rate": hbm_copy,
                    "lift_gb_per_s_of_bytes_read": F * bytes_per_frame / (total * 1e6), "lift_over_copy_at_hbm_rate": total / hbm_copy,
                    "lift_over_copy_cache_resident": total / copy,
                    "slots_ok": int(((got["status"] & 7) == OK).sum()), "points_total": int(got["total"].sum()),
                    "host_over_device": out["lift_host"]["ms_per_frame"] / (total / F)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
