"""Duplicate suppression and flip-view fusion (monosowa_amd/fuse.py) on the CPU: ``fuse_rows_host`` against the independent
restatement of tests/fuse_reference.py (overlaps from oracle/rotate_iou_oracle.py), the un-mirroring, textbook NMS, the 'mean' mode's
properties, the configuration keys, and the engine / Detector plumbing with the stub model of test_detector_cpu.py."""
import math

import numpy as np
import pytest
import torch

import fuse_reference as FR
from test_detector_cpu import StubModel, _stub_batch
from test_image_prep_cpu import fixture_cfg, write_kitti_root


@pytest.mark.parametrize("K,views", [(7, 1), (7, 2), (50, 1), (50, 2), (128, 2)])
def test_generator_terminates_and_covers_what_the_kernel_test_needs(K, views):
    case = FR.kernel_case(K, views, 0.5)
    above, below = FR.in_cluster_split(case)
    print("K %d, V %d: seed %d, in-cluster pairs above / below the threshold: %d / %d" % (K, views, case["tries"], above, below))
    assert case["tries"] <= 20 and above >= 0.3 * (above + below) and below > 0
    B = 3
    count = case["count"].reshape(views, B)
    assert (count[:, 0] == K).all() and (count[:, 1] == 0).all() and (0 < count[:, 2]).all() and (count[:, 2] < K).all()
    cands = np.concatenate([img["cands"] for img in case["images"]])
    assert np.isnan(cands[:, 13]).sum() == 1 and np.isnan(cands[:, 12]).sum() == 1 and (cands[:, 7] == 0).sum() == 1
    rows0 = case["rows"][0, :K]
    assert any(rows0[i].tobytes() == rows0[j].tobytes() for i in range(K) for j in range(i + 1, K))       # the bit-identical pair
    img = case["images"][0]                                              # the same box in two classes
    boxes = img["cands"][:, FR.BEV]
    assert any((boxes[i] == boxes[j]).all() and img["cands"][i, 0] != img["cands"][j, 0] for i in range(K) for j in range(i + 1, K))
    for img in case["images"]:                                           # every same-class pair keeps the margin
        assert all(math.isnan(v) or abs(v - 0.5) > FR.MARGIN for v in img["ious"].values())


@pytest.mark.parametrize("mode", ["seed", "mean"])
@pytest.mark.parametrize("K,views", [(7, 1), (7, 2), (50, 1), (50, 2)])
def test_host_fuse_equals_the_restatement(K, views, mode):
    from monosowa_amd.fuse import fuse_rows_host
    case = FR.kernel_case(K, views, 0.5)
    rows, count, support = fuse_rows_host(case["rows"], case["count"], case["geom"], 0.5, mode, views)
    assert rows.shape == (3, views * K, 14) and rows.dtype == np.float64 and count.dtype == np.int32 and support.dtype == np.int32
    for b, (seeds, want, members) in enumerate(FR.reference(case, mode)):
        n = len(seeds)
        assert count[b] == n and support[b, :n].tolist() == members.tolist() and members.sum() == len(case["images"][b]["ids"])
        assert not rows[b, n:].any() and not support[b, n:].any()
        np.testing.assert_allclose(rows[b, :n], want, rtol=0, atol=1e-9, equal_nan=True)
        if mode == "seed":
            for s, q in enumerate(seeds):                                # a seed of view 0 is the input row, byte for byte
                if case["images"][b]["ids"][q] < K:
                    assert rows[b, s].tobytes() == case["rows"][b, case["images"][b]["ids"][q]].tobytes()
    assert count[1] == 0


@pytest.mark.parametrize("mode", ["seed", "mean"])
def test_near_twin_scene_merges_every_pair(mode):
    """FR.twin_case, the scene of the kernel test: every pair's oracle IoU is above the threshold, the restatement and the host
    function make one cluster of two of each."""
    from monosowa_amd.fuse import fuse_rows_host
    case = FR.twin_case()
    pairs = len(FR.TWIN_KINDS)
    assert case["count"].tolist() == [2 * pairs, 0, 2 * pairs]
    rows, count, support = fuse_rows_host(case["rows"], case["count"], case["geom"], case["iou"], mode, 1)
    for b, (seeds, want, members) in enumerate(FR.reference(case, mode)):
        img = case["images"][b]
        n = len(seeds)
        assert n == len(img["ids"]) // 2 and members.tolist() == [2] * n
        assert not any(img["cands"][2 * k, FR.BEV].tobytes() == img["cands"][2 * k + 1, FR.BEV].tobytes() for k in range(n))
        assert count[b] == n and support[b, :n].tolist() == members.tolist()
        np.testing.assert_allclose(rows[b, :n], want, rtol=0, atol=1e-9, equal_nan=True)
    above = [case["images"][0]["ious"][(2 * k, 2 * k + 1)] for k in range(pairs)]
    assert min(above[:6]) > 0.999 and abs(above[7] - 0.9) < 1e-6 and 0.85 < above[6] < 0.93, above


def test_unmirror_inverts_the_mirror_map():
    """Rows mirrored with the inverse map (u -> W - u, calibration unchanged) come back to within 1e-9: double arithmetic on
    magnitudes up to 1e4 over a few operations rounds at about 1e-12."""
    from monosowa_amd.fuse import unmirror_rows
    rng = np.random.default_rng(3)
    for g in FR.GEOM:
        rows = np.array([FR._row(rng, g, rng.integers(0, 3), rng.uniform(-40, 40), rng.uniform(3, 80), rng.uniform(0.5, 12), rng.uniform(0.4, 3),
                                 rng.uniform(-math.pi, math.pi) * 0.999, rng.uniform(0, 1)) for _ in range(200)])
        mirrored = np.array([FR.flip_row(r, g) for r in rows])
        assert np.abs(mirrored[:, [1, 2, 4, 9, 12]] - rows[:, [1, 2, 4, 9, 12]]).max() > 1.0           # the map does move them
        back = unmirror_rows(mirrored, g)
        err = np.abs(back - rows).max()
        print("un-mirror round trip: %.3e" % err)
        assert err <= 1e-9
        assert back[:, [0, 3, 5, 6, 7, 8, 10, 11, 13]].tobytes() == rows[:, [0, 3, 5, 6, 7, 8, 10, 11, 13]].tobytes()


def test_one_view_seed_mode_is_textbook_nms():
    from monosowa_amd.fuse import fuse_rows_host
    case = FR.kernel_case(50, 1, 0.5)
    drop = ~np.isnan(case["rows"][..., 13]).any(1)                       # (textbook NMS has no rule for a NaN score)
    rows, count, support = fuse_rows_host(case["rows"], case["count"], case["geom"], 0.5, "seed", 1)
    checked = 0
    for b in np.nonzero(drop)[0]:
        img = case["images"][b]
        keep = FR.textbook_nms(img["cands"], lambda i, j: img["ious"][(min(i, j), max(i, j))], 0.5)
        assert count[b] == len(keep) and rows[b, :count[b]].tobytes() == img["cands"][keep].tobytes()
        checked += len(keep)
    assert checked > 20


def _pair(score_a, score_b, shift=0.0, K=2):
    """View 0 holds one box; view 1 holds the mirrored row of the same box moved by `shift` metres."""
    g = FR.GEOM[0]
    rng = np.random.default_rng(11)
    a = FR._row(rng, g, 1, 3.0, 20.0, 4.0, 1.8, 0.3, score_a)
    b = list(a)
    b[9], b[13] = b[9] + shift, score_b
    rows = np.zeros((2, K, 14))
    rows[0, 0], rows[1, 0] = a, FR.flip_row(b, g)
    return rows, np.array([1, 1], dtype=np.int32), g[None], np.array(a)


def test_mean_of_two_identical_members_is_the_member_and_an_unconfirmed_detection_keeps_half_its_score():
    from monosowa_amd.fuse import fuse_rows_host
    rows, count, geom, a = _pair(0.8, 0.8)
    out, n, support = fuse_rows_host(rows, count, geom, 0.5, "mean", 2)
    assert n.tolist() == [1] and support[0, 0] == 2
    np.testing.assert_allclose(out[0, 0], a, rtol=0, atol=1e-9)
    rows, count, geom, a = _pair(0.8, 0.6, shift=30.0)                    # the second view's box is elsewhere: two clusters of one
    out, n, support = fuse_rows_host(rows, count, geom, 0.5, "mean", 2)
    assert n.tolist() == [2] and support[0, :2].tolist() == [1, 1]
    assert out[0, 0, 13] == 0.4 and out[0, 1, 13] == 0.3
    np.testing.assert_allclose(out[0, 0, :13], a[:13], rtol=0, atol=1e-9)
    out, n, support = fuse_rows_host(rows, count, geom, 0.5, "seed", 2)   # 'seed' leaves the scores alone
    assert out[0, 0, 13] == 0.8 and out[0, 1, 13] == 0.6
    rows, count, geom, a = _pair(0.8, 0.6)                                # confirmed: (0.8 + 0.6) / 2
    out, n, support = fuse_rows_host(rows, count, geom, 0.5, "mean", 2)
    assert n.tolist() == [1] and abs(out[0, 0, 13] - 0.7) < 1e-15


def test_configuration_keys():
    from monosowa_amd.fuse import fuse_config
    for off in ({}, {"nms_iou": None}, {"nms_iou": 0}, {"nms_iou": 0.0, "flip_tta": False}, {"flip_tta": None, "fuse": "mean"}):
        assert fuse_config(off) is None
    assert fuse_config({"nms_iou": 0.5}) == (0.5, False, "seed")
    assert fuse_config({"nms_iou": 1, "flip_tta": True, "fuse": "mean"}) == (1.0, True, "mean")
    for bad in ({"nms_iou": -0.1}, {"nms_iou": 1.5}, {"nms_iou": "0.5"}, {"nms_iou": True}, {"nms_iou": float("nan")},
                {"nms_iou": 0.5, "flip_tta": 1}, {"nms_iou": 0.5, "flip_tta": "yes"}, {"flip_tta": True}, {"flip_tta": True, "nms_iou": 0},
                {"nms_iou": 0.5, "fuse": "max"}, {"fuse": None}):
        with pytest.raises(ValueError):
            fuse_config(bad)


def test_detector_and_tester_refuse_bad_keys(golden_dir, tmp_path):
    import logging
    from monosowa_amd import Detector
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.tester_helper import Tester
    root = write_kitti_root(golden_dir, tmp_path)
    dataset_cfg = fixture_cfg(root, "kitti_dataset.npz", tmp_path, type="KITTI", train_split="train", test_split="val", batch_size=2)
    loader = build_dataloader(dataset_cfg, workers=0)[1]
    for bad in ({"nms_iou": 2.0}, {"flip_tta": True}, {"nms_iou": 0.5, "fuse": "best"}, {"nms_iou": 0.5, "flip_tta": "on"}):
        tester_cfg = dict({"type": "KITTI", "topk": 50, "threshold": 0.2}, **bad)
        with pytest.raises(ValueError, match="tester"):
            Detector({"dataset": dataset_cfg, "tester": tester_cfg, "model": {}}, model=StubModel(), device="cpu")
        with pytest.raises(ValueError, match="tester"):
            Tester(tester_cfg, StubModel(), loader, logging.getLogger("fuse"), {"save_path": "unused/"}, "m")


def _geom(B):
    return torch.from_numpy(np.repeat(FR.GEOM[:1], B, 0).copy())


def test_engine_fuses_on_the_cpu_device():
    """With ``fuse=`` a batch's rows are ``fuse_rows_host`` of the rows the same engine decodes without it; ``support`` comes
    along; a batch without geometry, and prepared images with flip_tta, are refused."""
    from monosowa_amd.fuse import fuse_rows_host
    from monosowa_amd.inference import InferenceEngine
    cms = np.zeros((3, 3))
    plain = InferenceEngine(StubModel(), "cpu", topk=50, decode=(cms, 0.3))
    fused = InferenceEngine(StubModel(), "cpu", topk=50, decode=(cms, 0.3), fuse=(0.05, False, "mean"))
    for n, B in enumerate((3, 2)):
        want = (plain.submit(*_stub_batch(n, B), geom=_geom(B), tag=n) + plain.drain())[0]
        got = (fused.submit(*_stub_batch(n, B), geom=_geom(B), tag=n) + fused.drain())[0]
        assert want.support is None and got.tag == n
        rows, count, support = fuse_rows_host(want.rows, want.count, _geom(B).numpy(), 0.05, "mean", 1)
        assert got.rows.tobytes() == rows.tobytes() and got.count.tolist() == count.tolist() and got.support.tobytes() == support.tobytes()
        assert (count <= want.count).all() and support.sum() == want.count.sum()
    with pytest.raises(ValueError, match="geom"):
        fused.submit(*_stub_batch(5, 2), tag=5)
        fused.drain()
    flip = InferenceEngine(StubModel(), "cpu", topk=50, decode=(cms, 0.3), fuse=(0.5, True, "seed"))
    with pytest.raises(ValueError, match="flip_tta"):
        flip.submit(*_stub_batch(0, 2), geom=_geom(2), tag=0)
        flip.drain()
    with pytest.raises(ValueError, match="decode"):
        InferenceEngine(StubModel(), "cpu", fuse=(0.5, False, "seed"))


class ViewsStub(torch.nn.Module):
    """Canned outputs for B = batch / views images (every object predicted by two queries), repeated for every view: what the engine hands the model with flip_tta is
    2 B images, the second half mirrored."""

    def __init__(self, views):
        super().__init__()
        self.views, self.halves_differ = views, None

    def forward(self, images, calibs, targets, img_sizes, dn_args=None):
        B = images.shape[0] // self.views
        assert B * self.views == images.shape[0] and calibs.shape[0] == img_sizes.shape[0] == images.shape[0]
        g = torch.Generator().manual_seed(7)
        rnd = lambda *s: torch.rand(*s, generator=g)
        out = {"pred_logits": rnd(B, 50, 3) * 4 - 2, "pred_boxes": rnd(B, 50, 6) * 0.2 + 0.3, "pred_angle": rnd(B, 50, 24),
               "pred_3d_dim": rnd(B, 50, 3), "pred_depth": torch.cat([rnd(B, 50, 1) * 40 + 2, rnd(B, 50, 1)], 2)}
        for v in out.values():                                           # queries 25 .. 49 repeat 0 .. 24, a little less sure
            v[:, 25:] = v[:, :25]
        out["pred_logits"][:, 25:] -= 0.01
        if self.views == 2:
            self.halves_differ = not torch.equal(images[:B], images[B:])
            self.mirror_error = float((images[:B] - images[B:].flip(-1)).abs().mean() / (images[:B] - images[B:]).abs().mean())
        return {k: torch.cat([v] * self.views) for k, v in out.items()}


def test_detector_on_the_cpu_with_the_keys(golden_dir, tmp_path):
    """Detector plumbing on the CPU device: nms_iou alone equals fuse_rows_host of the keys-off rows; with flip_tta the model sees
    the batch twice, mirrored the second time, and ``detect(..., support=True)`` returns the members per row."""
    from monosowa_amd import Detector
    from monosowa_amd.fuse import fuse_rows_host
    root = write_kitti_root(golden_dir, tmp_path)
    dataset_cfg = fixture_cfg(root, "kitti_dataset.npz", tmp_path, meanshape=True)
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((48, 160), (40, 128), (48, 160))]
    P2 = np.array([[700.0, 0, 80.0, 40.0], [0, 700.0, 24.0, 0.2], [0, 0, 1, 0.003]])
    tester = {"topk": 50, "threshold": 0.3}
    off = Detector({"dataset": dataset_cfg, "tester": tester, "model": {}}, model=ViewsStub(1), device="cpu")
    base = off.detect(frames, P2, batch_size=2)
    rows, members = off.detect(frames, P2, batch_size=2, support=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, base)) and all((m == 1).all() and len(m) == len(r) for m, r in zip(members, rows))
    on = Detector({"dataset": dataset_cfg, "tester": dict(tester, nms_iou=0.05), "model": {}}, model=ViewsStub(1), device="cpu")
    got, members = on.detect(frames, P2, batch_size=2, support=True)
    streamed = [r for _, rr in on.stream([(frames[:2], P2), (frames[2:], P2)]) for r in rr]
    for k, frame in enumerate(frames):
        geom = off._batch([frame], P2, 0)[3].numpy()
        want, count, support = fuse_rows_host(base[k][None], np.array([len(base[k])]), geom, 0.05, "seed", 1)
        assert got[k].tobytes() == want[0, :count[0]].tobytes() and members[k].tolist() == support[0, :count[0]].tolist()
        assert 0 < len(got[k]) < len(base[k]) and members[k].sum() == len(base[k])
        assert streamed[k].tobytes() == got[k].tobytes()
    model = ViewsStub(2)
    flip = Detector({"dataset": dataset_cfg, "tester": dict(tester, nms_iou=0.05, flip_tta=True, fuse="mean"), "model": {}}, model=model,
                    device="cpu")
    rows, members = flip.detect(frames[:2], P2, batch_size=2, support=True)
    print("second half against the mirrored first half, relative to the unmirrored one: %.3g" % model.mirror_error)
    assert model.halves_differ and model.mirror_error < 0.05            # the second half is the first, mirrored (up to resampling)
    single = Detector({"dataset": dataset_cfg, "tester": tester, "model": {}}, model=ViewsStub(1), device="cpu").detect(frames[:2], P2, batch_size=2)
    both, count = np.zeros((4, 50, 14)), np.zeros(4, dtype=np.int32)
    for v in range(2):                                                   # the stub gives both views the same detections
        for b in range(2):
            both[2 * v + b, :len(single[b])], count[2 * v + b] = single[b], len(single[b])
    geom = off._batch(frames[:2], P2, 0)[3].numpy()
    want, n, support = fuse_rows_host(both, count, geom, 0.05, "mean", 2)
    for b in range(2):
        assert rows[b].tobytes() == want[b, :n[b]].tobytes() and members[b].tolist() == support[b, :n[b]].tolist()
        assert members[b].sum() == 2 * len(single[b]) > 0
