"""dataset.device_aug on the GPU: ``image_prep.prepare`` (csrc/image_prep.hip, one launch per batch) against the live CPU
pipeline of the machine -- ``torch.equal`` on whole tensors, no tolerance and no excluded elements -- and the raw-mode loader
through ``stage_batch``, a train step and ``Tester.inference``.  Cases and helpers: tests/test_image_prep_cpu.py."""
import logging
import os

import numpy as np
import pytest
import torch

from test_image_prep_cpu import (FIXTURE_RUNS, assert_cases_take_every_branch, case_record, cpu_pipeline, fixture_cfg, generated_cases,
                                 write_kitti_root)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture()
def kitti(golden_dir, tmp_path):
    return write_kitti_root(golden_dir, tmp_path), tmp_path


def _canvas(raws, fill):
    out = np.full((len(raws), max(r.shape[0] for r in raws), max(r.shape[1] for r in raws), 3), fill, dtype=np.uint8)
    for i, r in enumerate(raws):
        out[i, :r.shape[0], :r.shape[1]] = r
    return torch.from_numpy(out)


def _assert_equal(got, want, what):
    """got: device tensor [B, 3, H, W]; want: list of CPU-pipeline images.  Whole tensors, bit for bit."""
    want = torch.from_numpy(np.stack(want))
    assert got.dtype == torch.float32 and got.shape == want.shape and got.is_cuda
    assert got.is_contiguous(memory_format=torch.channels_last)
    got = got.cpu()
    if not torch.equal(got, want):
        diff = got != want
        per_image = diff.flatten(1).sum(1).tolist()
        first = diff.nonzero()[0].tolist()
        raise AssertionError("%s: %d elements differ (per image %s); first at %s: got %r, want %r"
                             % (what, int(diff.sum()), per_image, first, float(got[tuple(first)]), float(want[tuple(first)])))


def test_fixture_samples_equal_the_default_mode_on_the_device(kitti):
    """Item 6 / 2: every fixture sample (val seed 0, train seeds 11-13, aug_pd + aug_crop seeds 21, 22) prepared on the device
    equals the default mode's image and the reference's fixture entries (``img_sub`` exactly, ``img_sum`` to 1e-9)."""
    from monosowa_amd.image_prep import prepare
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    fixtures, root = kitti
    for name, split, seeds in FIXTURE_RUNS:
        g = fixtures[name]
        ds = KITTI_Dataset(split, fixture_cfg(fixtures, name, root))
        ds_raw = KITTI_Dataset(split, fixture_cfg(fixtures, name, root, device_aug=True))
        for seed in seeds:
            want, raws, recs = [], [], []
            for item in range(len(ds)):
                np.random.seed(seed * 100 + item)
                want.append(ds[item][0])
                np.random.seed(seed * 100 + item)
                raw, _, _, info = ds_raw[item]
                raws.append(raw)
                recs.append(info["prep"])
            got = prepare(_canvas(raws, 0), torch.from_numpy(np.stack(recs)), _dev())
            _assert_equal(got, want, "%s %s seed %d" % (name, split, seed))
            got = got.cpu().numpy()
            for item in range(len(ds)):
                key = "%s_s%d_i%d__" % (split, seed, item)
                assert np.array_equal(got[item][:, ::8, ::8], g[key + "img_sub"]), key
                want_sum = float(g[key + "img_sum"])
                assert abs(got[item].astype(np.float64).sum() - want_sum) <= 1e-9 * max(1.0, abs(want_sum))


def test_generated_cases_equal_the_cpu_pipeline_on_the_device():
    """Item 6 / 3: the generated cases (six source sizes, noise and smooth, flips, crops that leave the image on every side, 60
    photometric draws that take every branch and wrap both ways) in batches that mix sizes and flips, on a canvas whose padding
    is 255 (never read), B = 16 and the remainder; one more launch on a non-default stream and one with B = 1."""
    from monosowa_amd.image_prep import prepare
    cases = generated_cases()
    assert_cases_take_every_branch(cases)
    want = [cpu_pipeline(c) for c in cases]
    recs = [case_record(c)[0] for c in cases]
    for s in range(0, len(cases), 16):
        chunk = cases[s:s + 16]
        assert len({c["size"] for c in chunk}) > 1 and len({c["flip"] for c in chunk}) == 2
        got = prepare(_canvas([c["raw"] for c in chunk], 255), torch.from_numpy(np.stack(recs[s:s + 16])), _dev())
        _assert_equal(got, want[s:s + 16], "cases %d..%d" % (s, s + len(chunk) - 1))
    assert len(cases[:16]) == 16
    # a non-default stream: the launch goes to the caller's current stream, pinned sources, non-blocking copies
    stream = torch.cuda.Stream(device=_dev())
    raw = _canvas([c["raw"] for c in cases[16:32]], 255).pin_memory()
    rec = torch.from_numpy(np.stack(recs[16:32])).pin_memory()
    with torch.cuda.stream(stream):
        got = prepare(raw, rec, _dev())
    stream.synchronize()
    _assert_equal(got, want[16:32], "non-default stream")
    # B = 1, and the same image from device-resident inputs
    one = prepare(_canvas([cases[3]["raw"]], 255), torch.from_numpy(recs[3][None]), _dev())
    _assert_equal(one, want[3:4], "B = 1")
    again = prepare(_canvas([cases[3]["raw"]], 255).to(_dev()), torch.from_numpy(recs[3][None]).to(_dev()), _dev())
    _assert_equal(again, want[3:4], "B = 1, device-resident inputs")


def test_prepare_adds_no_host_synchronisation():
    """No device -> host synchronisation in ``prepare`` (torch's sync debug mode raises on one), pinned inputs as the loader gives."""
    from monosowa_amd.image_prep import prepare
    cases = generated_cases()[:4]
    raw = _canvas([c["raw"] for c in cases], 0).pin_memory()
    rec = torch.from_numpy(np.stack([case_record(c)[0] for c in cases])).pin_memory()
    prepare(raw, rec, _dev())                                            # warm: library load, the table's one-time upload
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = prepare(raw, rec, _dev())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _assert_equal(got, [cpu_pipeline(c) for c in cases], "sync-free launch")


def _loaders(fixtures, root, batch_size, **extra):
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    cfg = fixture_cfg(fixtures, "kitti_dataset_pd.npz", root, type="KITTI", train_split="train", test_split="val", batch_size=batch_size, **extra)
    return build_dataloader(cfg, workers=0, drop_last=True)


def _train_batch(loader, seed):
    np.random.seed(seed)                                                 # workers=0: the augmentation draws come from this stream
    torch.manual_seed(seed)                                              # the shuffle
    return next(iter(loader))


def test_staged_raw_loader_batch_equals_the_default_loader_batch(kitti):
    """Item 7: a raw-mode loader batch staged on the device == the default-mode loader batch staged on the device, inputs
    (channels-last, what stage_batch returns) and every target; train (aug_pd + flip + crop draws) and val loaders."""
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.image_prep import is_raw_batch
    from monosowa_amd.synthetic import prepare_targets
    fixtures, root = kitti
    default_train, default_val = _loaders(fixtures, root, 3)
    raw_train, raw_val = _loaders(fixtures, root, 3, device_aug=True)
    pairs = [(_train_batch(default_train, seed), _train_batch(raw_train, seed)) for seed in (31, 32)]
    pairs.append((next(iter(default_val)), next(iter(raw_val))))
    for want_raw, got_raw in pairs:
        assert is_raw_batch(got_raw[0]) and not is_raw_batch(want_raw[0])
        assert got_raw[0].is_pinned() and got_raw[3]["prep"].is_pinned()                 # pinning is still on
        want, got = stage_batch(want_raw, _dev()), stage_batch(got_raw, _dev())
        assert got[0].is_cuda and got[0].dtype == torch.float32 and got[0].shape == (3, 3, 384, 1280)
        assert got[0].is_contiguous(memory_format=torch.channels_last) and want[0].is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert set(got[2]) == set(want[2]) and all(torch.equal(got[2][k], want[2][k]) for k in want[2])
        assert len(prepare_targets(got[2], 3)) == 3                                      # the host mask travels as before


def test_train_step_and_inference_from_a_raw_loader(kitti, tmp_path):
    """Item 8: under torch.use_deterministic_algorithms(True) one train step (per-GPU batch 2) fed by the raw-mode loader gives
    the same losses bit for bit as fed by the default-mode loader; one Tester.inference pass runs from a raw-mode loader."""
    import yaml
    from monosowa_amd import flash_attn, pointwise
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.helpers.tester_helper import Tester
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import prepare_targets
    fixtures, root = kitti
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        cfg = yaml.safe_load(f)
    dev = _dev()

    def build():
        torch.manual_seed(444)
        model, crit = build_model(dict(cfg["model"], device="cuda"))
        model = to_mi355x_layout(model.to(dev)).train()
        return model, crit.to(dev).train(), build_optimizer(cfg["optimizer"], model)

    def step(loader):
        model, crit, opt = build()
        inputs, calibs, targets, info = stage_batch(_train_batch(loader, 41), dev)
        torch.manual_seed(7)                                             # the same dropout masks (tools/deterministic_step.py)
        pointwise._seed_counter[0] = flash_attn._seed_counter[0] = 0
        tl = prepare_targets(targets, 2)
        opt.zero_grad(set_to_none=True)
        losses = crit(model(inputs, calibs, tl, targets["img_size"]), tl)
        total = weighted_total(losses, crit.weight_dict)
        total.backward()
        opt.step()
        torch.cuda.synchronize()
        return model, {"total": total.detach().clone(), **{k: v.detach().clone() for k, v in losses.items()}}

    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        _, want = step(_loaders(fixtures, root, 2)[0])
        model, got = step(_loaders(fixtures, root, 2, device_aug=True)[0])
    finally:
        torch.use_deterministic_algorithms(was)
    assert set(got) == set(want) and torch.isfinite(got["total"]).item()
    differ = sorted(k for k in want if not torch.equal(got[k], want[k]))
    assert not differ, [(k, float(got[k]), float(want[k])) for k in differ]

    raw_val = _loaders(fixtures, root, 2, device_aug=True)[1]
    tester = Tester({"type": "KITTI", "topk": 50, "threshold": 0.0}, model, raw_val, logging.getLogger("image_prep"),
                    {"save_path": str(tmp_path / "out") + "/"}, "m")
    tester.output_dir = str(tmp_path / "out")
    results = tester.inference()
    assert sorted(results) == sorted(int(i) for i in raw_val.dataset.idx_list) and tester.last_img_per_s > 0
