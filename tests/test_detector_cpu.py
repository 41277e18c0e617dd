"""The public Detector and the inference engine, on the CPU: the per-frame helper against the dataset, the engine's queueing with
a stub model, the result writer against the Tester's."""
import logging
import os

import numpy as np
import pytest
import torch
from PIL import Image

import test_detector_gpu as G
from test_image_prep_cpu import fixture_cfg, write_kitti_root

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def kitti(golden_dir, tmp_path):
    return write_kitti_root(golden_dir, tmp_path), tmp_path


def _bits(a):
    a = np.asarray(a)
    return a.dtype, a.shape, a.tobytes()


def test_frame_helper_equals_the_dataset_on_validation_images(kitti):
    """img_size, height_crop, canonical_scale, the prep record, tx and ty of ``frame_geometry(size, P2, settings)`` against
    ``KITTI_Dataset("val", device_aug=True)[i]`` and ``get_calib``: same dtypes, same bits; with and without the canonical module."""
    from monosowa_amd.detector import frame_geometry
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    fixtures, root = kitti
    for extra in ({}, {"use_canonical_module": False}, {"meanshape": True, "canonical_focal_length": 1000.0}):
        cfg = fixture_cfg(fixtures, "kitti_dataset.npz", root, device_aug=True, **extra)
        ds = KITTI_Dataset("val", cfg)
        settings = KITTI_Dataset.settings({k: v for k, v in cfg.items() if k != "root_dir"})       # no directory behind it
        assert _bits(settings.cls_mean_size) == _bits(ds.cls_mean_size) and settings.class_name == ds.class_name
        assert len(ds) >= 2
        for i in range(len(ds)):
            raw, P2, _, info = ds[i]
            got = frame_geometry((raw.shape[1], raw.shape[0]), P2, settings)
            for key in ("img_size", "height_crop", "canonical_scale", "prep"):
                assert type(got[key]) is type(info[key]) and _bits(got[key]) == _bits(info[key]), (extra, i, key, got[key], info[key])
            cal = ds.get_calib(int(info["img_id"]))
            for key in ("cu", "cv", "fu", "fv", "tx", "ty"):
                assert _bits(getattr(got["calib"], key)) == _bits(getattr(cal, key)), (extra, i, key)
            assert _bits(got["calib"].P2) == _bits(P2)
            # a float64 copy of the same matrix (what a caller who computed P2 holds) gives the same frame quantities
            again = frame_geometry((raw.shape[1], raw.shape[0]), P2.astype(np.float64), settings)
            assert _bits(again["height_crop"]) == _bits(got["height_crop"]) and _bits(again["calib"].tx) == _bits(got["calib"].tx)


class StubModel(torch.nn.Module):
    """Returns canned output dicts: batch n's logits carry n, so that every result can be traced to its submission."""

    def __init__(self, fail_on=None):
        super().__init__()
        self.calls, self.fail_on = 0, fail_on

    def forward(self, images, calibs, targets, img_sizes, dn_args=None):
        n, B = self.calls, images.shape[0]
        self.calls += 1
        if n == self.fail_on:
            raise RuntimeError("stub failure in batch %d" % n)
        g = torch.Generator().manual_seed(100 + n)
        rnd = lambda *s: torch.rand(*s, generator=g)
        return {"pred_logits": rnd(B, 50, 3) * 4 - 2, "pred_boxes": rnd(B, 50, 6) * 0.2 + 0.3, "pred_angle": rnd(B, 50, 24),
                "pred_3d_dim": rnd(B, 50, 3), "pred_depth": torch.cat([rnd(B, 50, 1) * 40 + 2, rnd(B, 50, 1)], 2),
                "seen": (images[:, 0, 0, 0].clone(), img_sizes.clone())}


def _stub_batch(n, B):
    images = torch.full((B, 3, 8, 16), float(n))
    calibs = torch.eye(3, 4).repeat(B, 1, 1)
    img_size = torch.tensor([[1242, 375]] * B)
    height_crop = torch.full((B,), 1.0 + 0.01 * n, dtype=torch.float64)
    return images, calibs, img_size, height_crop


def test_engine_on_the_cpu_keeps_order_bounds_and_errors():
    from monosowa_amd.helpers.decode_helper import extract_dets_from_outputs
    from monosowa_amd.inference import InferenceEngine
    sizes = [4, 4, 3, 4, 1, 4, 2]                                   # full and partial batches
    model = StubModel()
    engine = InferenceEngine(model, "cpu", topk=50, in_flight=2)
    got, most = [], 0
    for n, B in enumerate(sizes):
        got += engine.submit(*_stub_batch(n, B), tag=n)
        most = max(most, len(engine.queue))
        assert len(engine.queue) <= engine.in_flight
    rest = engine.drain()
    assert not engine.queue and engine.drain() == []
    got += rest
    assert [r.tag for r in got] == list(range(len(sizes))) and most <= 2
    want_model = StubModel()
    for r, B in zip(got, sizes):
        images, calibs, img_size, height_crop = _stub_batch(r.tag, B)
        sizes_arg = img_size.clone()
        sizes_arg[:, 1] = sizes_arg[:, 1] / height_crop                # Tester.inference's expression
        out = want_model(images, calibs, None, sizes_arg)
        want = extract_dets_from_outputs(out, K=50, topk=50).numpy()
        assert r.dets.dtype == np.float32 and r.dets.shape == (B, 50, 37) and np.array_equal(r.dets, want)
        assert r.rows is None and r.count is None
    assert engine.images == sum(sizes) and engine.model_seconds > 0 and engine.eager_forwards == len(sizes) and engine.replays == 0
    engine.close()

    # the integer assignment reaches the model
    seen = {}

    class Spy(StubModel):
        def forward(self, images, calibs, targets, img_sizes, dn_args=None):
            seen["img_sizes"] = img_sizes.clone()
            return super().forward(images, calibs, targets, img_sizes, dn_args)

    engine = InferenceEngine(Spy(), "cpu")
    engine.submit(*_stub_batch(7, 2), tag=0)
    assert seen["img_sizes"].dtype == torch.int64 and seen["img_sizes"].tolist() == [[1242, int(375 / 1.07)]] * 2
    engine.close()

    # an exception inside a batch: the batches before it are delivered, it surfaces at the next call -- submit or drain -- once
    for next_call in ("submit", "drain"):
        engine = InferenceEngine(StubModel(fail_on=2), "cpu", in_flight=2)
        got = []
        for n in range(3):
            got += engine.submit(*_stub_batch(n, 2), tag=n)
        assert [r.tag for r in got] == [0, 1]
        with pytest.raises(RuntimeError, match="stub failure in batch 2"):
            engine.submit(*_stub_batch(3, 2), tag=3) if next_call == "submit" else engine.drain()
        assert engine.drain() == []                                      # raised once, nothing left behind
        got = engine.submit(*_stub_batch(4, 2), tag=4) + engine.drain()  # and the engine goes on
        assert [r.tag for r in got] == [4]
        engine.close()


def test_engine_decodes_rows_on_the_cpu_like_decode_detections(golden_dir):
    """A batch submitted with geometry comes back as rows [B, K, 14] + count: the kept rows of ``decode_detections`` first, zeros
    behind them (the contract of mono_decode_dets_f64, which the CPU device fulfils through decode_detections)."""
    from monosowa_amd.helpers.decode_helper import PinholeCalib, decode_detections
    from monosowa_amd.inference import decode_rows_host
    g = np.load(os.path.join(golden_dir, "decode.npz"), allow_pickle=False)
    cams = [PinholeCalib(p) for p in g["P2"]]
    geom = np.array([[s[0], s[1], hc, cs, c.cu, c.cv, c.fu, c.fv, c.tx, c.ty] for s, hc, cs, c in
                     zip(g["info_img_size"], g["info_height_crop"], g["info_canonical_scale"], cams)], dtype=np.float64)
    info = {"img_id": list(g["info_img_id"]), "img_size": g["info_img_size"], "height_crop": g["info_height_crop"],
            "canonical_scale": g["info_canonical_scale"]}
    median = float(np.median(g["dets"][:, :, 1]))                       # the fixture's own threshold keeps every row
    for threshold in (float(g["threshold"]), median):
        rows, count = decode_rows_host(g["dets"], geom, g["cls_mean_size"], threshold)
        want = decode_detections(g["dets"], info, cams, g["cls_mean_size"], threshold)
        assert count.tolist() == [len(want[i]) for i in info["img_id"]]
        for b, i in enumerate(info["img_id"]):
            assert np.array_equal(rows[b, :count[b]], np.asarray(want[i], dtype=np.float64)) and not rows[b, count[b]:].any()
        if threshold == median:
            assert 0 < count.min() < 50                                  # rows are dropped, and not all of them
        else:
            assert count.tolist() == g["counts"].tolist()


def test_write_kitti_writes_the_testers_bytes(kitti, tmp_path, golden_dir):
    from monosowa_amd import Detector
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.tester_helper import Tester
    fixtures, root = kitti
    g = np.load(os.path.join(golden_dir, "decode.npz"), allow_pickle=False)
    rows = [g["decoded"][b, :int(g["counts"][b])] for b in range(3)] + [np.zeros((0, 14))]
    rng = np.random.default_rng(5)
    rows.append(np.concatenate([rng.integers(0, 3, (7, 1)).astype(np.float64), rng.normal(0, 30, (7, 13))], 1))   # every class, negative values
    ids = [3, 7, 12, 25, 40]
    dataset_cfg = fixture_cfg(fixtures, "kitti_dataset.npz", root, type="KITTI", train_split="train", test_split="val", batch_size=2)
    cfg = {"dataset": dataset_cfg, "tester": {"type": "KITTI", "topk": 50, "threshold": 0.2}, "model": {}}
    det = Detector(cfg, model=StubModel(), device="cpu")
    det.write_kitti(rows, ids, tmp_path / "detector")
    loader = build_dataloader(dataset_cfg, workers=0)[1]
    tester = Tester(cfg["tester"], StubModel(), loader, logging.getLogger("detector"), {"save_path": "unused/"}, "m")
    tester.output_dir = str(tmp_path / "tester")
    tester.save_results({i: [[int(r[0])] + [float(v) for v in r[1:]] for r in rr] for i, rr in zip(ids, rows)})   # decode_detections' row type
    names = sorted(os.listdir(tmp_path / "detector"))
    assert names == ["%06d.txt" % i for i in ids] == sorted(os.listdir(tmp_path / "tester" / "outputs" / "data"))
    for name in names:
        a, b = (tmp_path / "detector" / name).read_bytes(), (tmp_path / "tester" / "outputs" / "data" / name).read_bytes()
        assert a == b
    assert (tmp_path / "detector" / "000025.txt").read_bytes() == b"" and len((tmp_path / "detector" / "000040.txt").read_bytes().splitlines()) == 7


def test_detector_on_the_cpu_streams_frames_in_order_and_checks_them(kitti):
    """End to end on the CPU device with the stub model: mixed frame sizes in one batch, partial last batch, ids in order, rows
    equal to decode_detections on the same detections; what is not 8-bit RGB raises ValueError."""
    from monosowa_amd import Detector
    from monosowa_amd.detector import frame_geometry
    from monosowa_amd.helpers.decode_helper import decode_detections, extract_dets_from_outputs
    from monosowa_amd.image_prep import prepare_reference
    fixtures, root = kitti
    dataset_cfg = fixture_cfg(fixtures, "kitti_dataset.npz", root, meanshape=True)
    cfg = {"dataset": dataset_cfg, "tester": {"topk": 50, "threshold": 0.75}, "model": {}}
    det = Detector(cfg, model=StubModel(), device="cpu")
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((48, 160), (40, 128), (48, 160), (30, 100), (48, 160))]
    P2 = np.array([[700.0, 0, 80.0, 40.0], [0, 700.0, 24.0, 0.2], [0, 0, 1, 0.003]])
    rows = det.detect(frames, np.broadcast_to(P2, (5, 3, 4)), batch_size=2)
    assert len(rows) == 5 and all(r.dtype == np.float64 and r.ndim == 2 and r.shape[1] == 14 for r in rows)
    want_model, k = StubModel(), 0
    for lo in (0, 2, 4):
        chunk = frames[lo:lo + 2]
        geos = [frame_geometry((f.shape[1], f.shape[0]), P2, det.dataset) for f in chunk]
        images = torch.from_numpy(np.stack([prepare_reference(f, g["prep"]) for f, g in zip(chunk, geos)]))
        out = want_model(images, None, None, torch.zeros(len(chunk), 2))
        dets = extract_dets_from_outputs(out, K=50, topk=50).numpy()
        info = {"img_id": list(range(len(chunk))), "img_size": np.stack([g["img_size"] for g in geos]),
                "height_crop": np.array([g["height_crop"] for g in geos]), "canonical_scale": np.array([g["canonical_scale"] for g in geos])}
        want = decode_detections(dets, info, [g["calib"] for g in geos], det.dataset.cls_mean_size, 0.75)
        for i in range(len(chunk)):
            assert 0 < len(want[i]) < 50 and np.array_equal(rows[k], np.asarray(want[i], dtype=np.float64)), k
            k += 1
    ids = [i for got_ids, _ in det.stream([(frames[:3], P2), (frames[3:], P2)]) for i in got_ids]
    assert ids == [0, 1, 2, 3, 4]
    for bad in (frames[0].astype(np.float32), frames[0][:, :, 0], np.zeros((8, 8, 4), np.uint8), frames[0].astype(np.uint16), [[1, 2, 3]]):
        with pytest.raises(ValueError, match="8-bit RGB"):
            det.detect([frames[0], bad], P2)
    with pytest.raises(ValueError, match="P2"):
        det.detect(frames, np.zeros((2, 3, 4)))
    assert det.detect(frames[:1], P2)[0].shape[1] == 14                  # the detector goes on after a refused call
    assert Image.fromarray(frames[0]).mode == "RGB"


def test_case_coverage_and_the_reference_alone_near_pi(golden_dir):
    """What the cases must cover, and that rows with a reference ry within 1e-9 of +-pi are at most 1 % of each case -- a property
    of the numpy reference and the seeds alone."""
    classes, bins, wrapped_alpha, wrapped_ry, dropped, nan = set(), set(), 0, 0, 0, 0
    for kind, seed, meanshape in G.CASES:
        dets, info, cams, cms, thr = G.fixture_case(golden_dir) if kind == "fixture" else G.random_case(seed, meanshape)
        ref = G.reference_rows(dets, info, cams, cms, thr)
        assert G.near_pi_fraction(ref) <= 0.01, (kind, seed)
        classes |= set(dets[:, :, 0].astype(int).ravel().tolist())
        bins |= set(np.argmax(dets[:, :, 7:19], axis=2).ravel().tolist())
        raw_alpha = np.argmax(dets[:, :, 7:19], 2) * (2 * np.pi / 12) + np.take_along_axis(dets[:, :, 19:31], np.argmax(dets[:, :, 7:19], 2)[..., None], 2)[..., 0]
        wrapped_alpha += int((raw_alpha > np.pi).sum())
        all_rows = G.reference_rows(dets, info, cams, cms, -1.0)
        for b, r in enumerate(all_rows):
            keep = ~np.isnan(dets[b, :, 1])
            a = r[keep, 1] + np.arctan2(dets[b, keep, 2].astype(np.float64) * info["img_size"][b][0] - cams[b].cu, cams[b].fu)
            wrapped_ry += int(((a > np.pi) | (a < -np.pi)).sum())
        dropped += sum(dets.shape[1] - len(r) for r in ref)
        nan += int(np.isnan(dets[:, :, 1]).sum())
        if kind == "random":
            assert len({tuple(s) for s in info["img_size"]}) > 3 and bool(np.any(cms)) == meanshape
    assert classes == {0, 1, 2} and bins == set(range(12)) and wrapped_alpha > 50 and wrapped_ry > 20 and dropped > 100 and nan >= 1
