"""Rate of the template-pose search (monosowa_amd/template_fit.py) at the reference's shipped shape: B = 16 objects, a 1,000-point
template, 10,000 scan points each, the 40 x 40 x 40 coarse grid and the 360-angle fine stage.

    python tools/template_fit_rate.py [--objects 16] [--points 10000] [--template 1000] [--iters 40] [--out FILE.json]
    python tools/template_fit_rate.py --host [--host-iters 3 3 4] [--out FILE.json]        (no GPU: fit_host alone)

Device time between event pairs around back-to-back ``fit`` calls, median of 5 after one warm-up; the stages (grid build, the two
searches, the two reduces) between event pairs of their own in a second set of 5 calls.  ``--host`` times ``fit_host``'s search on
the first cloud over a small grid and scales it by the placement count to the full shape: an extrapolation, labelled as one (the
cost of a placement does not depend on the grid it belongs to).  VGPRs, scratch and static LDS per kernel come from hipcc's resource
remarks for the translation unit (the search kernel's LDS is sized by the launch and reported beside them).  One JSON line on stdout, also written to ``--out``."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

DIMS = (1.526, 1.63, 3.88)


def box_template(T, rng):
    """``T`` points on the surface of the template box."""
    h, w, l = DIMS
    half = np.array([w / 2, h / 2, l / 2])
    pts = rng.uniform(-1, 1, (T, 3)) * half
    axis = rng.integers(0, 3, T)
    pts[np.arange(T), axis] = np.where(rng.random(T) < 0.5, -1, 1) * half[axis]
    return pts.astype(np.float32)


def cloud(tmpl, N, rng):
    """An aggregated scan: ``N`` noisy template points (sigma 3 cm) seen from one side, at a pose inside the search range 8..60 m
    ahead, one in ten of them clutter within 3 m."""
    t = tmpl.astype(np.float64)[rng.integers(0, len(tmpl), N)]
    th = rng.uniform(0, 2 * np.pi)
    place = np.array([rng.uniform(-15, 15), 1.6, rng.uniform(8, 60)])
    c, s = np.cos(th), np.sin(th)
    pts = np.stack([c * t[:, 0] + s * t[:, 2], t[:, 1], c * t[:, 2] - s * t[:, 0]], axis=1) + rng.normal(0, 0.03, (N, 3))
    clutter = rng.random(N) < 0.1
    pts[clutter] = rng.uniform(-3, 3, (int(clutter.sum()), 3)) * np.array([1, 0.3, 1])
    return (pts + place + np.array([rng.uniform(-1, 1), 0, rng.uniform(0, 2)])).astype(np.float32)


def kernel_resources():
    """{kernel: {vgprs, scratch, lds, occupancy}} from hipcc's remarks, or None when hipcc is not there."""
    from monosowa_amd import build
    src = os.path.join(build.CSRC, "template_fit.hip")
    try:
        cmd = [build.hipcc()] + [f for f in build.FLAGS if f != "-shared"] + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                            "-o", os.devnull, src]
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
    except Exception:
        return None
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN3fit\d+", "", m.group(1)).split("E")[0]
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--template", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-iters", type=int, nargs=3, default=[3, 3, 4])
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    import torch
    from monosowa_amd.template_fit import TemplateFitter, search_host, coarse_angles, FINE_ANGLES
    rng = np.random.default_rng(0)
    tmpl = box_template(args.template, rng)
    clouds = [cloud(tmpl, args.points, rng) for _ in range(args.objects)]
    per_object = args.iters ** 3 + FINE_ANGLES
    out = {"objects": args.objects, "template_points": args.template, "scan_points": args.points,
           "grid": [args.iters] * 3, "fine_angles": FINE_ANGLES, "placements_per_object": per_object}
    if args.host:
        I, J, K = args.host_iters
        f = TemplateFitter(tmpl, {"optimization": {"opt_param1_iters": I, "opt_param2_iters": J, "opt_param3_iters": K}}, device="cpu")
        c = np.median(clouds[0].astype(np.float64), axis=0)
        tx, tz = (np.linspace(-2, 2, I) + c[0]).astype(np.float32), (np.linspace(-1, 3, J) + c[2]).astype(np.float32)
        th = coarse_angles(K)
        cs = np.stack([np.cos(th), np.sin(th)], axis=1).astype(np.float32)
        t0 = time.perf_counter()
        search_host(f.template, clouds[0], tx, np.float32(c[1]), tz, cs, f.config.r, False)
        seconds = time.perf_counter() - t0
        out["fit_host"] = {"measured_placements": I * J * K, "measured_s": seconds, "s_per_placement": seconds / (I * J * K),
                           "extrapolated_total_s": seconds / (I * J * K) * per_object * args.objects,
                           "note": "EXTRAPOLATION: one cloud, %d placements, scaled by the placement count to %d objects x %d placements"
                                   % (I * J * K, args.objects, per_object)}
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        f = TemplateFitter(tmpl, {"optimization": {"opt_param1_iters": args.iters, "opt_param2_iters": args.iters,
                                                   "opt_param3_iters": args.iters}}, device=dev)
        padded = torch.from_numpy(np.stack(clouds)).to(dev)
        counts = torch.full((args.objects,), args.points, dtype=torch.int32, device=dev)
        centres = torch.from_numpy(np.array([np.median(p.astype(np.float64), axis=0) for p in clouds])).to(dev)
        result = f.fit((padded, counts), centres)             # warm-up: the library, the template, the allocator's blocks
        torch.cuda.synchronize()
        assert not result.host
        totals = []
        for _ in range(5):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            f.fit((padded, counts), centres)
            end.record()
            torch.cuda.synchronize()
            totals.append(start.elapsed_time(end))
        stages = {}
        for _ in range(5):
            f.timing = []
            f.fit((padded, counts), centres)
            torch.cuda.synchronize()
            for name, start, end in f.timing:
                stages.setdefault(name, []).append(start.elapsed_time(end))
        f.timing = None
        total = statistics.median(totals)
        got = result.numpy()
        out.update({"device": torch.cuda.get_device_name(dev), "total_ms": total, "total_ms_runs": totals,
                    "stage_ms": {k: statistics.median(v) for k, v in stages.items()},
                    "placements_per_s": args.objects * per_object / (total * 1e-3),
                    "mean_score": float(got["score"].mean()), "kernels": kernel_resources(),
                    "search_kernel_dynamic_lds_bytes": (3 * args.template + f.grid.ncell + 1) * 4})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
