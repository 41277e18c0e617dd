"""Whole train steps of the shipped model under torch.use_deterministic_algorithms(True) (README "Deterministic training").

Builds the model of configs/monodetr.yaml from a fixed seed, runs `--steps` AdamW steps on a synthetic KITTI-size batch and
reports on one JSON line:
  repeat   two fresh instances in this process: losses, every gradient and every updated parameter bit-identical?
  digest   SHA-256 of the same tensors (compare the digests of two processes)
  ddp      the second instance wrapped in DistributedDataParallel at world size 1 (RANK / WORLD_SIZE / MASTER_* set)
  time     paired A/B of the step at per-GPU batch 16, flag off / on, alternating (ms per step, medians)
`--warn-only` turns the mode on with warn_only=True and lists the ops that warned instead of raising.
Used by tests/test_deterministic_step_gpu.py in child processes."""
import argparse
import hashlib
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["repeat", "digest", "ddp", "time"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--warn-only", action="store_true")
    args = ap.parse_args()

    import torch
    import yaml
    # does this torch build demand CUBLAS_WORKSPACE_CONFIG in the mode? (CUDA builds raise in the first BLAS call without it)
    cublas_env = os.environ.pop("CUBLAS_WORKSPACE_CONFIG", None)
    torch.use_deterministic_algorithms(True)
    try:
        torch.randn(64, 64, device="cuda") @ torch.randn(64, 64, device="cuda")
        demands_cublas_config = False
    except RuntimeError:
        demands_cublas_config = True
    if cublas_env is not None:
        os.environ["CUBLAS_WORKSPACE_CONFIG"] = cublas_env
    torch.use_deterministic_algorithms(args.mode != "time", warn_only=args.warn_only)

    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    from monosowa_amd import flash_attn, pointwise

    dev = torch.device("cuda", 0)
    if args.mode == "ddp":
        import torch.distributed as dist
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    batch = 16 if args.mode == "time" else args.batch

    def build():
        torch.manual_seed(444)
        model, crit = build_model(dict(cfg["model"], device="cuda"))
        model = to_mi355x_layout(model.to(dev)).train()
        return model, crit.to(dev).train(), build_optimizer(cfg["optimizer"], model)

    inputs, calibs, targets, _ = make_batch(batch, dev, seed=3)
    inputs = inputs.contiguous(memory_format=torch.channels_last)
    tl = prepare_targets(targets, batch)

    def step(net, crit, opt):
        torch.manual_seed(7)                       # the same dropout masks: torch's generator and the HIP kernels' seed counters
        pointwise._seed_counter[0] = flash_attn._seed_counter[0] = 0
        opt.zero_grad(set_to_none=True)
        total = weighted_total(crit(net(inputs, calibs, tl, targets["img_size"]), tl), crit.weight_dict)
        total.backward()
        return total.detach()

    def run(net, crit, opt, core):
        """-> {name: tensor}: the losses of every step, the last step's gradients and the parameters after the last update."""
        out = {}
        for k in range(args.steps):
            out["loss.%d" % k] = step(net, crit, opt).clone()
            if k == args.steps - 1:
                out.update({"grad." + n: p.grad.clone() for n, p in core.named_parameters() if p.grad is not None})
            opt.step()
        out.update({"param." + n: p.detach().clone() for n, p in core.named_parameters()})
        torch.cuda.synchronize()
        return out

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if args.mode == "time":
            net, crit, opt = build()
            times = {False: [], True: []}
            for r in range(12):
                on = bool(r % 2)
                torch.use_deterministic_algorithms(on)
                step(net, crit, opt)                       # (the first call of a mode selects its kernels)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    step(net, crit, opt)
                torch.cuda.synchronize()
                if r >= 2:
                    times[on].append((time.perf_counter() - t0) / 3 * 1e3)
            med = lambda v: sorted(v)[len(v) // 2]
            result = {"ms_per_step_off": med(times[False]), "ms_per_step_on": med(times[True]), "batch": batch}
        else:
            net_a, crit_a, opt_a = build()
            a = run(net_a, crit_a, opt_a, net_a)
            result = {}
            if args.mode == "digest":
                h = hashlib.sha256()
                for n in sorted(a):
                    h.update(n.encode())
                    h.update(a[n].cpu().contiguous().numpy().tobytes())
                result["sha256"] = h.hexdigest()
            else:
                net_b, crit_b, opt_b = build()
                if args.mode == "ddp":
                    from monosowa_amd.helpers.trainer_helper import wrap_ddp
                    wrapped = wrap_ddp(net_b, dev)
                    assert isinstance(wrapped, torch.nn.parallel.DistributedDataParallel)
                    b = run(wrapped, crit_b, opt_b, net_b)
                else:
                    b = run(net_b, crit_b, opt_b, net_b)
                assert set(a) == set(b), sorted(set(a) ^ set(b))[:5]
                result["differ"] = sorted(n for n in a if not torch.equal(a[n], b[n]))
            result["n_tensors"] = len(a)
            result["loss"] = float(a["loss.0"])
    result["alerts"] = sorted({str(w.message).split(" does not have")[0] for w in caught if "deterministic" in str(w.message)})
    result["demands_cublas_workspace_config"] = demands_cublas_config
    print(json.dumps(result))
    if args.mode == "ddp":
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
