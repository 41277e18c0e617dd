"""Rate of the object-track stage (monosowa_amd/track.py) at the workload's window: F = 61 frames of M = 8 slots, about half of them
OK (six cars on lines, each seen in two frames of three, some of them driving), S = 1 and S = 16 windows in one launch.

    python tools/track_rate.py [--frames 61] [--slots 8] [--lift-frames 61] [--out FILE.json]
    python tools/track_rate.py --host-only [--out FILE.json]                                  (no GPU: track_host alone)

Device time between event pairs around 20 back-to-back launches, median of 5 sets after one warm-up: the whole launch, and each of
its two stages alone (the association; the per-track summary, which reads the table the association left).  ``track_host``'s wall time on
the same windows.  Then the chain on one lifted window (tools/lift_rate.py's KITTI-sized frames): lift, track and gather each between
event pairs of their own, and the three enqueued back to back between one pair, beside the host's wall time to enqueue them and the
number of host synchronisations counted on the way.  One JSON line on stdout, also written to ``--out`` (default
``profiles/track_rate_<date>.json``)."""
import argparse
import datetime
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

LAUNCHES, SETS = 20, 5


def window(F, M, rng, cars=6, seen=2.0 / 3.0):
    """-> centres float64 [F, M, 3], status int32 [F, M]: ``cars`` cars 40 m apart, about half of them driving (up to 1.5 m a frame),
    each seen with probability ``seen`` in a frame, in shuffled slots; the other slots ABSENT"""
    from monosowa_amd.lift import ABSENT, OK
    centres, status = np.zeros((F, M, 3)), np.full((F, M), ABSENT, dtype=np.int32)
    starts = np.stack([40.0 * np.arange(cars), np.ones(cars), 30.0 + rng.uniform(0, 10, cars)], axis=1)
    steps = rng.uniform(-1.5, 1.5, (cars, 3)) * [1.0, 0.02, 1.0] * (rng.uniform(size=(cars, 1)) < 0.5)
    for f in range(F):
        slots = rng.permutation(M)
        for j in range(cars):
            if rng.uniform() < seen:
                centres[f, slots[j]], status[f, slots[j]] = starts[j] + f * steps[j] + rng.normal(0, 0.05, 3), OK
    return centres, status


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--lift-frames", type=int, default=61)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_rate_%s.json" % datetime.date.today().isoformat()))
    args = ap.parse_args(argv)
    import torch
    from monosowa_amd.lift import OK, LiftResult, ObjectLifter, lift_config
    from monosowa_amd.track import ObjectTracker, track_host
    F, M = args.frames, args.slots
    cfg = {"frames_creation": {"nscans_before": F // 2}}
    rng = np.random.default_rng(0)
    windows = [window(F, M, rng) for _ in range(16)]
    centres, status = np.stack([w[0] for w in windows]), np.stack([w[1] for w in windows])
    out = {"frames": F, "slots": M, "launches_per_set": LAUNCHES, "sets": SETS,
           "slots_ok_fraction": float(((status & 7) == OK).mean())}
    host = {}
    for S in (1, 16):
        t0 = time.perf_counter()
        host[S] = track_host(centres[:S], status[:S], cfg)
        out["track_host_ms_S%d" % S] = 1e3 * (time.perf_counter() - t0)
    out["tracks_per_window"] = host[16].count.tolist()
    out["moving_per_window"] = host[16].moving.sum(dim=1).tolist()

    if not args.host_only:
        dev = torch.device("cuda", torch.cuda.current_device())
        out["device"] = torch.cuda.get_device_name(dev)

        def event_ms(call, n=1):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                call()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) / n

        def lifted(c, s):
            z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
            fields = {"points": z((F, M, 1, 3), torch.float32), "counts": z((F, M), torch.int32), "total": z((F, M), torch.int32),
                      "centres": torch.from_numpy(c).to(dev), "range": z((F, M), torch.float64), "truncated": z((F, M), torch.bool),
                      "status": torch.from_numpy(s).to(dev), "shrink": z((F, M), torch.int32)}
            return LiftResult(lift_config(cfg), False, **fields)
        tracker = ObjectTracker(cfg, device=dev)
        lifts = [lifted(*w) for w in windows]
        for S in (1, 16):
            arg = lifts[0] if S == 1 else lifts
            got = tracker.track(arg)                                # warm-up: the library, the allocator's blocks
            torch.cuda.synchronize()
            assert not got.host
            want, res = host[S].numpy(), got.numpy()
            for k in ("tracks", "length", "ref_mask", "moving", "visible", "keep", "count", "dropped"):
                assert np.array_equal(res[k], want[k]), k           # the same answers as the host routine
            whole = [event_ms(lambda: tracker.track(arg), LAUNCHES) for _ in range(SETS)]
            stages = {}
            for _ in range(SETS):
                tracker.timing = []
                for _ in range(LAUNCHES):
                    tracker.track(arg)
                torch.cuda.synchronize()
                per = {}
                for name, start, end in tracker.timing:
                    per.setdefault(name, []).append(start.elapsed_time(end))
                tracker.timing = None
                for name, v in per.items():
                    stages.setdefault(name, []).append(sum(v) / len(v))
            out["track_ms_S%d" % S] = statistics.median(whole)
            out["track_ms_S%d_sets" % S] = whole
            out["stage_ms_S%d" % S] = {k: statistics.median(v) for k, v in stages.items()}
            out["host_over_device_S%d" % S] = out["track_host_ms_S%d" % S] / out["track_ms_S%d" % S]
            out["max_tracks_S%d" % S] = int(got.tracks.shape[1])

        # the chain on one lifted window
        spec = importlib.util.spec_from_file_location("lift_rate", os.path.join(ROOT, "tools", "lift_rate.py"))
        lift_rate = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(lift_rate)
        LF = args.lift_frames
        chain_cfg = {"frames_creation": {"nscans_before": LF // 2}}
        depth, intr, masks, poses = lift_rate.frames(LF, M, np.random.default_rng(1))
        d = [torch.from_numpy(a).to(dev) for a in (depth, intr, masks)] + [None, torch.from_numpy(poses).to(dev)]
        lifter, chain_tracker = ObjectLifter(chain_cfg, device=dev), ObjectTracker(chain_cfg, device=dev)

        def chain():
            res = lifter.lift(*d)
            tr = chain_tracker.track(res)
            return res, tr, res.gather(*tr.gather_args())
        res, tr, _ = chain()                                       # warm-up
        torch.cuda.synchronize()
        assert not res.host and not tr.host
        waits, real = [], torch.cuda.synchronize
        torch.cuda.synchronize = lambda *a, **k: (waits.append(1), real(*a, **k))[1]
        try:
            t0 = time.perf_counter()
            chain()
            enqueue_ms = 1e3 * (time.perf_counter() - t0)
            counted = len(waits)
        finally:
            torch.cuda.synchronize = real
        torch.cuda.synchronize()
        table, flags = tr.gather_args()
        out["chain"] = {
            "frames": LF, "slots": M, "image": [lift_rate.H, lift_rate.W], "max_tracks": int(tr.tracks.shape[1]),
            "tracks": int(tr.count.item()), "slots_ok": int(((res.status & 7) == OK).sum().item()),
            "lift_ms": statistics.median([event_ms(lambda: lifter.lift(*d)) for _ in range(SETS)]),
            "track_ms": statistics.median([event_ms(lambda: chain_tracker.track(res)) for _ in range(SETS)]),
            "gather_ms": statistics.median([event_ms(lambda: res.gather(table, flags)) for _ in range(SETS)]),
            "chain_ms": statistics.median([event_ms(chain) for _ in range(SETS)]),
            "enqueue_wall_ms": enqueue_ms, "synchronisations_in_the_chain": counted}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
