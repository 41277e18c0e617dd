"""Two BUILDS of libmonosowa_pointwise.so against each other inside ONE process, alternating (A, B, A, B, ...) as tools/ab_step.py
does for a module-level setting: box-to-box and run-to-run noise cancels.  A = e.g. a build of the parent commit's csrc.

    python tools/pointwise_lib_ab.py --a /path/to/parent/libmonosowa_pointwise.so [--b <this tree's>] [--kernels] [--step] [--steps 60] [--out x.json]

--kernels  the ReLU-bearing kernels at the train step's largest shapes, 7 rounds of 20 launches per library (CUDA events)
--step     the shipped train step (per-GPU batch 16), every step timed with a device sync, the library handle swapped per step
Reports medians, and for A its own spread (max - min over the rounds / the two halves of its steps): the yardstick for B - A.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monosowa_amd import miopen_tuning   # noqa: E402
miopen_tuning.use_shipped_db(0)

import torch   # noqa: E402

from monosowa_amd import pointwise   # noqa: E402
from monosowa_amd._lib import raw_stream   # noqa: E402


def load_lib(path):
    """A ctypes handle with the argument types ``pointwise.load`` sets, for the library at ``path`` (None: this tree's)."""
    was = os.environ.pop("MONOSOWA_POINTWISE_LIB", None)
    if path:
        os.environ["MONOSOWA_POINTWISE_LIB"] = path
    pointwise._lib = None
    try:
        return pointwise.load()
    finally:
        os.environ.pop("MONOSOWA_POINTWISE_LIB", None)
        if was is not None:
            os.environ["MONOSOWA_POINTWISE_LIB"] = was


def kernel_cases():
    dev = "cuda"
    M = 16 * 96 * 320
    r = lambda *s: torch.randn(*s, device=dev)
    x64, x0, x256, res = r(M, 64), r(M, 64), r(M, 256), r(M, 256)
    y256, y64 = torch.empty(M, 256, device=dev), torch.empty(M, 64, device=dev)
    w, wd, wh, wh256 = r(64, 256) * .05, r(64, 256) * .05, r(64, 64) * .05, r(256, 64) * .05
    b64, b256 = r(64), r(256)
    stem, stem_out = r(16, 192, 640, 64), torch.empty(16, 96, 320, 64, device=dev)
    mask = torch.empty(M * 256 // 4, dtype=torch.uint8, device=dev)
    B, HW = 16, 48 * 160
    gx, gy, gyo, gnx = r(B, HW, 256), r(B, HW, 256), torch.empty(B, HW, 256, device=dev), torch.empty(B, HW, 256, device=dev)
    stats, part = torch.zeros(B * 64, dtype=torch.float64, device=dev), torch.zeros(B * 512, dtype=torch.float64, device=dev)
    mr, gwb = torch.empty(B * 64, device=dev), torch.empty(512, device=dev)
    p = lambda t: t.data_ptr()
    s = raw_stream()
    return {
        "conv1x1_tail [491520 px]": lambda L: L.mono_conv1x1_tail_f32(p(x64), p(b64), p(w), p(b256), p(res), p(y256), M, 64, 256, s),
        "conv1x1_tail_ds [491520 px]": lambda L: L.mono_conv1x1_tail_ds_f32(p(x64), p(b64), p(w), p(x0), p(wd), p(b256), p(y256), M, 64, 256, s),
        "conv1x1_head<64> [491520 px]": lambda L: L.mono_conv1x1_head_f32(p(x64), p(wh), p(b64), p(y64), M, 64, 64, s),
        "conv1x1_head<256> [491520 px]": lambda L: L.mono_conv1x1_head_f32(p(x256), p(wh256), p(b64), p(y64), M, 256, 64, s),
        "bias_relu_maxpool [16,64,192,640]": lambda L: L.mono_bias_relu_maxpool_nhwc_f32(p(stem), p(b64), p(stem_out), 16, 192, 640, 64, s),
        "bias_relu_mask + residual [491520,256]": lambda L: L.mono_bias_relu_mask_f32(p(y256), p(b256), p(res), p(mask), M, 256, s),
        "relu_grad_mask<two> [491520,256]": lambda L: L.mono_relu_grad_mask_f32(p(x256), p(res), p(mask), p(y256), M * 256, s),
        "relu_grad2 [491520,256]": lambda L: L.mono_relu_grad2_f32(p(x256), p(res), p(x256), p(y256), M * 256, s),
        "relu_dropout_fwd [491520,256]": lambda L: L.mono_relu_dropout_fwd_f32(p(x256), p(y256), M * 256, 0.1, 7, s),
        "groupnorm+relu fwd [16,256,48,160]": lambda L: (stats.zero_(), L.mono_groupnorm_nhwc_fwd_f32(
            p(gx), None, p(b256), p(b256), p(gyo), p(stats), p(mr), B, HW, 256, 32, 1e-5, 1, s))[1],
        "groupnorm+relu bwd [16,256,48,160]": lambda L: (part.zero_(), L.mono_groupnorm_nhwc_bwd_f32(
            p(gy), p(gx), None, p(gyo), p(mr), p(b256), p(gnx), p(part), None, None, p(gwb), B, HW, 256, 32, 1, s))[1],
    }


def time_us(fn, n=20):
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def run_kernels(libs, rounds=7):
    out = {}
    for name, fn in kernel_cases().items():
        ts = {"A": [], "B": []}
        for _ in range(rounds):
            for k in ("A", "B"):
                ts[k].append(time_us(lambda: fn(libs[k])))
        row = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in ts.items()}
        row["B_minus_A_median_us"] = round(row["B"]["median_us"] - row["A"]["median_us"], 2)
        row["A_spread_us"] = round(row["A"]["max_us"] - row["A"]["min_us"], 2)
        out[name] = row
        print("%-40s A %8.2f us  B %8.2f us  B - A %+6.2f  (A's spread %.2f)" % (
            name, row["A"]["median_us"], row["B"]["median_us"], row["B_minus_A_median_us"], row["A_spread_us"]), flush=True)
    return out


def run_step(libs, steps):
    import yaml
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    dev = torch.device("cuda:0")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    model, crit = build_model(cfg["model"])
    model = to_mi355x_layout(model.to(dev)).train()
    crit.to(dev).train()
    opt = build_optimizer(cfg["optimizer"], model)
    inputs, calibs, targets, _ = make_batch(16, dev)
    inputs = inputs.contiguous(memory_format=torch.channels_last)

    def step():
        tl = prepare_targets(targets, 16)
        opt.zero_grad(set_to_none=True)
        o = model(inputs, calibs, tl, targets["img_size"])
        weighted_total(crit(o, tl), crit.weight_dict).backward()
        opt.step()
    for k in "AB" * 8:
        pointwise._lib = libs[k]
        step()
    torch.cuda.synchronize()
    times = {"A": [], "B": []}
    for i in range(steps):
        k = "AB"[i & 1]
        pointwise._lib = libs[k]
        torch.cuda.synchronize()
        t = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    half = len(times["A"]) // 2
    a_halves = [statistics.median(times["A"][:half]), statistics.median(times["A"][half:])]
    out = {"steps_per_library": len(times["A"]), "A_median_ms": round(med["A"], 3), "B_median_ms": round(med["B"], 3),
           "B_minus_A_median_ms": round(med["B"] - med["A"], 3), "A_first_half_median_ms": round(a_halves[0], 3),
           "A_second_half_median_ms": round(a_halves[1], 3), "A_spread_ms": round(abs(a_halves[0] - a_halves[1]), 3),
           "A_min_ms": round(min(times["A"]), 3), "B_min_ms": round(min(times["B"]), 3)}
    print("train step: " + json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True)
    ap.add_argument("--b", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    libs = {"A": load_lib(os.path.abspath(args.a)), "B": load_lib(os.path.abspath(args.b) if args.b else None)}
    assert libs["A"] is not libs["B"]
    out = {"A": args.a, "B": args.b or "this tree's monosowa_amd/lib/libmonosowa_pointwise.so"}
    if args.kernels:
        out["kernels"] = run_kernels(libs)
    if args.step:
        out["train_step"] = run_step(libs, args.steps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
