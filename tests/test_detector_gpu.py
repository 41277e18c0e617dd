"""The public Detector, the inference engine and mono_decode_dets_f64 on the GPU.

The end-to-end comparisons run under torch.use_deterministic_algorithms(True): the shipped mode's GroupNorm atomics make two runs
of ANY path differ in the last bits, and an untrained model's near-equal scores then reorder the top-k -- comparing there would
test noise.  ``threshold: 0.0`` keeps all K rows."""
import contextlib
import glob
import logging
import os
import time

import numpy as np
import pytest
import torch
import tqdm
from PIL import Image

from test_image_prep_cpu import fixture_cfg, write_kitti_root

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RY = 12                                                                  # the column that passes through atan2
EXACT = [c for c in range(14) if c != RY]
NEAR_PI = 1e-9                                                           # reference ry this close to +-pi: one last bit flips the wrap


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def deterministic():
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was)


# ================================================================================================ 4. the decode kernel
def random_case(seed, meanshape):
    """Seeded detections [B, K, 37] with every class, scores on both sides of the threshold, one NaN score, headings whose bin +
    residual wraps past pi, cameras that push ry past +-pi, mixed image sizes and crops."""
    from monosowa_amd.helpers.decode_helper import PinholeCalib
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    rng = np.random.default_rng(seed)
    B, K = 6, 64
    dets = np.zeros((B, K, 37), dtype=np.float32)
    dets[:, :, 0] = rng.integers(0, 3, (B, K))
    dets[:, :, 1] = np.sort(rng.uniform(0.02, 0.98, (B, K)).astype(np.float32), axis=1)[:, ::-1]
    dets[2, 5, 1] = np.nan
    dets[:, :, 2:4] = rng.uniform(0.02, 0.98, (B, K, 2))
    dets[:, :, 4:6] = rng.uniform(0.01, 0.4, (B, K, 2))
    dets[:, :, 6] = rng.uniform(2, 70, (B, K))
    dets[:, :, 7:19] = rng.normal(0, 2, (B, K, 12))
    dets[:, :, 19:31] = rng.uniform(-0.6, 0.6, (B, K, 12))
    dets[0, :12, 7:19] = -5.0                                             # every bin wins once ...
    dets[0, np.arange(12), 7 + np.arange(12)] = 5.0
    dets[1, 0, 7:19] = 1.5                                                # ... and an exact tie goes to the lowest index
    dets[:, :, 31:34] = rng.normal(0, 0.3, (B, K, 3))
    dets[:, :, 34:36] = dets[:, :, 2:4] + rng.normal(0, 0.01, (B, K, 2)).astype(np.float32)
    dets[:, :, 36] = rng.uniform(0.2, 1.0, (B, K))
    sizes = np.array([(1242, 375), (1224, 370), (1408, 376), (1920, 1280), (640, 200), (1280, 384)])
    info = {"img_id": list(range(B)), "img_size": sizes, "height_crop": rng.uniform(0.85, 1.15, B),
            "canonical_scale": rng.uniform(0.5, 1.6, B)}
    info["height_crop"][3] = 1.0                                          # no crop: the padding is exactly zero
    P2 = np.zeros((B, 3, 4), dtype=np.float32)
    P2[:, 0, 0] = P2[:, 1, 1] = rng.uniform(500, 1100, B)
    P2[:, 0, 2], P2[:, 1, 2] = sizes[:, 0] * rng.uniform(0.3, 0.7, B), sizes[:, 1] * rng.uniform(0.4, 0.6, B)
    P2[:, 0, 3], P2[:, 1, 3], P2[:, 2, 2], P2[:, 2, 3] = rng.uniform(-50, 50, B), rng.uniform(-1, 1, B), 1.0, 0.003
    ds = KITTI_Dataset.settings({"meanshape": meanshape})
    return dets, info, [PinholeCalib(p) for p in P2], ds.cls_mean_size, 0.4


def fixture_case(golden_dir):
    from monosowa_amd.helpers.decode_helper import PinholeCalib
    g = np.load(os.path.join(golden_dir, "decode.npz"), allow_pickle=False)
    info = {"img_id": list(range(3)), "img_size": g["info_img_size"], "height_crop": g["info_height_crop"],
            "canonical_scale": g["info_canonical_scale"]}
    return g["dets"], info, [PinholeCalib(p) for p in g["P2"]], g["cls_mean_size"], float(np.median(g["dets"][:, :, 1]))


def case_geom(info, cams):
    return np.array([[s[0], s[1], hc, cs, c.cu, c.cv, c.fu, c.fv, c.tx, c.ty] for s, hc, cs, c in
                     zip(info["img_size"], info["height_crop"], info["canonical_scale"], cams)], dtype=np.float64)


def reference_rows(dets, info, cams, cls_mean_size, threshold):
    from monosowa_amd.helpers.decode_helper import decode_detections
    with np.errstate(invalid="ignore"):
        res = decode_detections(dets, info, cams, cls_mean_size, threshold)
    return [np.asarray(res[i], dtype=np.float64).reshape(-1, 14) for i in info["img_id"]]


def device_rows(dets, info, cams, cls_mean_size, threshold):
    from monosowa_amd.kitti_eval import decode_dets_device
    dev = _dev()
    rows, count = decode_dets_device(torch.from_numpy(dets).to(dev), torch.from_numpy(case_geom(info, cams)).to(dev),
                                     torch.from_numpy(np.ascontiguousarray(cls_mean_size, dtype=np.float64)).to(dev), threshold)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), count.cpu().numpy()


def atan2_difference(dets, info, cams):
    """max |device atan2 - numpy arctan2| over the very arguments the decode feeds it, (x - cu, fu): once through torch.atan2 in
    float64 on the device, once through the kernel itself with all-zero headings (alpha = 0, so the ry column IS atan2)."""
    geom = case_geom(info, cams)
    x = dets[:, :, 2].astype(np.float64) * geom[:, 0:1]
    want = np.arctan2(x - geom[:, 4:5], np.broadcast_to(geom[:, 6:7], x.shape))
    dev = _dev()
    by_torch = torch.atan2(torch.from_numpy(x - geom[:, 4:5]).to(dev), torch.from_numpy(np.broadcast_to(geom[:, 6:7], x.shape).copy()).to(dev))
    plain = dets.copy()
    plain[:, :, 7:31] = 0.0
    plain[:, :, 1] = 1.0
    rows, count = device_rows(plain, info, cams, np.zeros((3, 3)), 0.0)
    assert (count == dets.shape[1]).all()
    return max(float(np.abs(by_torch.cpu().numpy() - want).max()), float(np.abs(rows[:, :, RY] - want).max()))


def near_pi_fraction(ref):
    ry = np.concatenate([r[:, RY] for r in ref])
    return float((np.abs(np.abs(ry) - np.pi) <= NEAR_PI).mean())


CASES = [("fixture", None, None), ("random", 3, True), ("random", 4, False), ("random", 5, True)]


def test_decode_kernel_equals_decode_detections(golden_dir):
    """count and every column but ry bit for bit; ry within 4 x the difference of atan2 alone on the same arguments (device
    against numpy).  Measured on MI355X (ROCm's OCML against glibc): see ATAN2_MEASURED below, printed by this test."""
    worst = 0.0
    for kind, seed, meanshape in CASES:
        dets, info, cams, cms, thr = fixture_case(golden_dir) if kind == "fixture" else random_case(seed, meanshape)
        ref = reference_rows(dets, info, cams, cms, thr)
        measured = atan2_difference(dets, info, cams)
        bound = 4 * measured
        rows, count = device_rows(dets, info, cams, cms, thr)
        print("%s %s: atan2 alone differs by at most %.3e -> ry bound %.3e" % (kind, seed, measured, bound))
        assert measured <= 4 * np.finfo(np.float64).eps, "atan2 on the device is further from numpy's than a few last bits: %g" % measured
        assert count.dtype == np.int32 and count.tolist() == [len(r) for r in ref]
        left_out = total = 0
        for b, want in enumerate(ref):
            got = rows[b, :count[b]]
            assert not rows[b, count[b]:].any(), (kind, seed, b, "the tail must be zero")
            assert got[:, EXACT].tobytes() == want[:, EXACT].tobytes(), (kind, seed, b, np.argwhere(got[:, EXACT] != want[:, EXACT])[:5])
            near = np.abs(np.abs(want[:, RY]) - np.pi) <= NEAR_PI
            left_out, total = left_out + int(near.sum()), total + len(want)
            err = np.abs(got[~near, RY] - want[~near, RY])
            worst = max(worst, float(err.max()) if err.size else 0.0)
            assert (err <= bound).all(), (kind, seed, b, float(err.max()), bound)
        assert left_out <= 0.01 * total
    print("worst ry difference %.3e" % worst)


# ATAN2_MEASURED on MI355X (ROCm's OCML against glibc, float64), max |device atan2 - numpy arctan2| on the decode's own arguments:
# 1.110e-16 in each of the four cases (one last bit of a value in [0.5, 1)), through torch.atan2 and through the kernel alike
# -> ry bound 4.441e-16; worst ry difference seen 4.441e-16 (one last bit of an ry in [2, 4)).


# ================================================================================================ the end-to-end pieces
@pytest.fixture()
def kitti(golden_dir, tmp_path):
    return write_kitti_root(golden_dir, tmp_path), tmp_path


def _yaml():
    import yaml
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        return yaml.safe_load(f)


def _model(seed=444):
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    cfg = _yaml()
    torch.manual_seed(seed)
    model, crit = build_model(dict(cfg["model"], device="cuda"))
    return to_mi355x_layout(model.to(_dev())).eval(), crit.to(_dev()), cfg


def _dataset_cfg(fixtures, root, batch_size, **extra):
    return fixture_cfg(fixtures, "kitti_dataset.npz", root, type="KITTI", train_split="train", test_split="val", batch_size=batch_size, **extra)


def _val_loader(fixtures, root, batch_size, **extra):
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    return build_dataloader(_dataset_cfg(fixtures, root, batch_size, **extra), workers=0)[1]


TESTER_CFG = {"type": "KITTI", "topk": 50, "threshold": 0.0}


def _tester(cls, model, loader, out):
    tester = cls(dict(TESTER_CFG), model, loader, logging.getLogger("detector"), {"save_path": str(out) + "/"}, "m")
    tester.output_dir = str(out)
    return tester


def _parent_tester_class():
    """``Tester`` with the ``inference`` and ``save_results`` of the commit before the engine, verbatim: the reference of tests 5
    and 6."""
    from monosowa_amd.helpers.decode_helper import PinholeCalib, decode_detections, extract_dets_from_outputs
    from monosowa_amd.helpers.tester_helper import Tester
    from monosowa_amd.image_prep import is_raw_batch, prepare

    class ParentTester(Tester):
        @torch.no_grad()
        def inference(self):
            self.model.eval()
            results, model_time, n_img = {}, 0.0, 0
            bar = tqdm.tqdm(total=len(self.dataloader), leave=True, desc="Evaluation Progress")
            for inputs, calibs, targets, info in self.dataloader:
                if is_raw_batch(inputs):                                  # dataset.device_aug: one launch prepares the batch
                    inputs = prepare(inputs, info["prep"], self.device)
                else:
                    inputs = inputs.to(self.device)
                calibs_dev = calibs.to(self.device)
                img_sizes = info["img_size"].to(self.device).clone()
                img_sizes[:, 1] = img_sizes[:, 1] / info["height_crop"].to(self.device)
                if self.device.type == "cuda":
                    torch.cuda.synchronize()
                t0 = time.time()
                outputs = self.model(inputs, calibs_dev, targets, img_sizes, dn_args=0)
                if self.device.type == "cuda":
                    torch.cuda.synchronize()
                model_time += time.time() - t0
                n_img += inputs.shape[0]
                dets = extract_dets_from_outputs(outputs=outputs, K=self.max_objs, topk=self.cfg["topk"]).cpu().numpy()
                dataset = self.dataloader.dataset
                if hasattr(dataset, "get_calib"):
                    cal = [dataset.get_calib(int(i)) for i in info["img_id"]]
                else:
                    cal = [PinholeCalib(p) for p in calibs.numpy()]
                info_np = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in info.items()}
                results.update(decode_detections(dets=dets, info=info_np, calibs=cal, cls_mean_size=dataset.cls_mean_size,
                                                 threshold=self.cfg.get("threshold", 0.2)))
                bar.update()
            bar.close()
            self.last_img_per_s = n_img / max(model_time, 1e-9)
            print("inference on {} images: {:.2f} img/s (model only)".format(n_img, self.last_img_per_s))
            self.logger.info("==> Saving ...")
            self.save_results(results)
            return results

        def save_results(self, results):
            """One KITTI label file per image: 'Class 0.0 0 alpha x1 y1 x2 y2 h w l x y z ry score', '%.2f'."""
            output_dir = os.path.join(self.output_dir, "outputs", "data")
            os.makedirs(output_dir, exist_ok=True)
            for img_id, preds in results.items():
                with open(os.path.join(output_dir, "{:06d}.txt".format(int(img_id))), "w") as f:
                    for p in preds:
                        f.write("{} 0.0 0".format(self.class_name[int(p[0])]))
                        for j in range(1, len(p)):
                            f.write(" {:.2f}".format(p[j]))
                        f.write("\n")

    return ParentTester


def _frames_of(loader):
    """The validation images and cameras of a loader's dataset as a caller of the Detector holds them."""
    ds = loader.dataset
    ids = [int(i) for i in ds.idx_list]
    frames = [np.array(Image.open(os.path.join(ds.image_dir, "%06d.png" % i))) for i in ids]
    return ids, frames, np.stack([ds.get_calib(i).P2 for i in ids])


def _ry_bound(frames, P2, dataset, rows_like):
    """Test 4's bound on these frames' own atan2 arguments: 4 x max |device atan2 - numpy arctan2| over (x - cu, fu)."""
    from monosowa_amd.detector import frame_geometry
    worst = 0.0
    for f, p, rows in zip(frames, P2, rows_like):
        c = frame_geometry((f.shape[1], f.shape[0]), p, dataset)["calib"]
        x = (rows[:, 2] + rows[:, 4]) / 2                                # any abscissae in the image's range serve the measurement
        a, b = x - np.float64(c.cu), np.full_like(x, np.float64(c.fu))
        got = torch.atan2(torch.from_numpy(a).to(_dev()), torch.from_numpy(b).to(_dev())).cpu().numpy()
        worst = max(worst, float(np.abs(got - np.arctan2(a, b)).max()))
    return 4 * worst


def _assert_rows(got, want, bound, what):
    want = np.asarray(want, dtype=np.float64).reshape(-1, 14)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert got[:, EXACT].tobytes() == want[:, EXACT].tobytes(), (what, np.argwhere(got[:, EXACT] != want[:, EXACT])[:5])
    near = np.abs(np.abs(want[:, RY]) - np.pi) <= NEAR_PI
    assert near.mean() <= 0.01, what
    err = np.abs(got[~near, RY] - want[~near, RY])
    assert (err <= bound).all(), (what, float(err.max()), bound)


@pytest.mark.parametrize("batch_size", [4, 5])
def test_detect_equals_the_parents_inference_loop(kitti, tmp_path, batch_size):
    """Detector.detect(frames, P2) against the parent commit's Tester.inference loop over a device_aug val loader of the same
    directory: six frames of four different sizes, so batches mix sizes and the last one is partial (4 + 2, 5 + 1)."""
    from monosowa_amd import Detector
    fixtures, root = kitti
    model, _, cfg = _model()
    loader = _val_loader(fixtures, root, batch_size, device_aug=True)
    ids, frames, P2 = _frames_of(loader)
    assert len({f.shape for f in frames[:batch_size]}) >= 2 and len(frames) % batch_size
    with deterministic():
        want = _tester(_parent_tester_class(), model, loader, tmp_path / "parent").inference()
        det = Detector({"dataset": _dataset_cfg(fixtures, root, batch_size), "tester": dict(TESTER_CFG), "model": cfg["model"]}, model=model)
        got_ids, got = [], []
        for i, rows in det.stream((frames[k:k + batch_size], P2[k:k + batch_size]) for k in range(0, len(frames), batch_size)):
            got_ids += i
            got += rows
        again = det.detect(frames, P2, batch_size=batch_size)
        replays, eager = det.engine.replays, det.engine.eager_forwards
        det.close()
    assert list(want) == ids and got_ids == list(range(len(ids)))        # ids and order: frame k is the loader's k-th image
    assert replays == 4 and eager == 0                                   # the forward ran from graphs
    bound = _ry_bound(frames, P2, det.dataset, got)
    print("ry bound %.3e" % bound)
    for k, img_id in enumerate(ids):
        assert len(want[img_id]) == 50
        _assert_rows(got[k], want[img_id], bound, ("stream", img_id))
        assert again[k].tobytes() == got[k].tobytes()


@pytest.mark.parametrize("device_aug", [True, False])
def test_tester_inference_on_the_engine_equals_the_parents_loop(kitti, tmp_path, device_aug):
    """Tester.inference() against the parent's loop: the returned dict equal, the written files byte-identical."""
    from monosowa_amd.helpers.tester_helper import Tester
    fixtures, root = kitti
    model, _, _ = _model()
    loader = _val_loader(fixtures, root, 4, device_aug=device_aug)
    with deterministic():
        want = _tester(_parent_tester_class(), model, loader, tmp_path / "parent").inference()
        tester = _tester(Tester, model, loader, tmp_path / "engine")
        got = tester.inference()
    assert list(got) == list(want) and tester.last_img_per_s > 0
    for k in want:
        assert len(got[k]) == len(want[k]) == 50
        for a, b in zip(got[k], want[k]):
            assert [type(v) for v in a] == [type(v) for v in b]
            assert np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes(), k
    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "parent" / "outputs" / "data" / "*.txt")))
    assert names == ["%06d.txt" % int(i) for i in loader.dataset.idx_list]
    assert names == sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "engine" / "outputs" / "data" / "*.txt")))
    for name in names:
        a = open(os.path.join(str(tmp_path / "parent" / "outputs" / "data"), name), "rb").read()
        assert a and a == open(os.path.join(str(tmp_path / "engine" / "outputs" / "data"), name), "rb").read(), name


def _eager_rows(det, frames, P2):
    """An eager eval forward + extract_dets_from_outputs on the detector's model as it is now, decoded by the same kernel."""
    from monosowa_amd.helpers.decode_helper import extract_dets_from_outputs
    from monosowa_amd.image_prep import prepare
    from monosowa_amd.kitti_eval import decode_dets_device
    canvas, calibs, info, geom = det._batch(frames, P2, 0)
    dev = det.device
    with torch.no_grad():
        images = prepare(canvas, info["prep"], dev)
        img_sizes = info["img_size"].to(dev).clone()
        img_sizes[:, 1] = img_sizes[:, 1] / info["height_crop"].to(dev)
        out = det.model.eval()(images, calibs.to(dev), None, img_sizes, dn_args=0)
        dets = extract_dets_from_outputs(outputs=out, K=50, topk=det.topk)
        rows, count = decode_dets_device(dets, geom.to(dev), det.engine.decode[0], det.engine.decode[1])
    torch.cuda.synchronize()
    return [rows[i, :int(count[i])].cpu().numpy() for i in range(len(frames))]


def _train_steps(model, crit, cfg, n):
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    opt = build_optimizer(cfg["optimizer"], model)
    model.train()
    crit.train()
    for k in range(n):
        inputs, calibs, targets, _ = make_batch(2, _dev(), seed=70 + k, resolution=(320, 96))
        tl = prepare_targets(targets, 2)
        opt.zero_grad(set_to_none=True)
        weighted_total(crit(model(inputs.contiguous(memory_format=torch.channels_last), calibs, tl, targets["img_size"]), tl), crit.weight_dict).backward()
        opt.step()
    model.eval()


def test_weights_changed_in_place_reach_the_next_detect(kitti):
    """detect, two AdamW train steps on the same module, detect: the second result is the eager forward on the updated weights,
    bit for bit, and differs from the first."""
    from monosowa_amd import Detector
    fixtures, root = kitti
    model, crit, cfg = _model()
    ids, frames, P2 = _frames_of(_val_loader(fixtures, root, 3, device_aug=True))
    frames, P2 = frames[:3], P2[:3]
    with deterministic():
        det = Detector({"dataset": _dataset_cfg(fixtures, root, 3), "tester": dict(TESTER_CFG), "model": cfg["model"]}, model=model)
        first = det.detect(frames, P2, batch_size=3)
        assert det.engine.replays == 1
        _train_steps(model, crit, cfg, 2)
        second = det.detect(frames, P2, batch_size=3)
        assert det.engine.replays == 2 and det.engine.eager_forwards == 0          # from a graph again, a recaptured one
        want = _eager_rows(det, frames, P2)
        det.close()
    for k in range(3):
        assert second[k].shape == (50, 14) and second[k].tobytes() == want[k].tobytes(), k
    assert any(a.tobytes() != b.tobytes() for a, b in zip(first, second))


def test_stream_does_not_synchronise_the_device_per_batch(kitti, monkeypatch):
    """torch.cuda.synchronize is called as often in a 6-batch run of Detector.stream as in a 2-batch run."""
    from monosowa_amd import Detector
    fixtures, root = kitti
    model, _, cfg = _model()
    ids, frames, P2 = _frames_of(_val_loader(fixtures, root, 2, device_aug=True))
    det = Detector({"dataset": _dataset_cfg(fixtures, root, 2), "tester": dict(TESTER_CFG), "model": cfg["model"]}, model=model)
    batches = lambda n: [([frames[(2 * k) % 6], frames[(2 * k + 1) % 6]], P2[[(2 * k) % 6, (2 * k + 1) % 6]]) for k in range(n)]
    assert sum(len(r) for _, r in det.stream(batches(2))) == 4           # warm: the capture of this batch size
    calls = [0]
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    counts, replays = [], []
    for n in (2, 6):
        before, r0 = calls[0], det.engine.replays
        assert sum(len(r) for _, r in det.stream(batches(n))) == 2 * n
        counts.append(calls[0] - before)
        replays.append(det.engine.replays - r0)
    monkeypatch.undo()
    det.close()
    print("torch.cuda.synchronize calls: %s" % counts)
    assert counts[0] == counts[1] and replays == [2, 6]


def test_input_checks_and_graph_bookkeeping(kitti):
    """What is not 8-bit RGB raises ValueError; four batch sizes in a row leave at most three graphs, the fourth runs eagerly, and
    every one of them gives the eager result."""
    from monosowa_amd import Detector
    from monosowa_amd.inference import MAX_GRAPHS
    fixtures, root = kitti
    model, _, cfg = _model()
    ids, frames, P2 = _frames_of(_val_loader(fixtures, root, 2, device_aug=True))
    with deterministic():
        det = Detector({"dataset": _dataset_cfg(fixtures, root, 2), "tester": dict(TESTER_CFG), "model": cfg["model"]}, model=model)
        for bad in (frames[0].astype(np.float32), frames[0][:, :, 0], frames[0].astype(np.uint16), np.zeros((8, 8, 4), np.uint8)):
            with pytest.raises(ValueError, match="8-bit RGB"):
                det.detect([frames[0], bad], P2[:2])
        sizes = (3, 2, 1, 4)
        got = [rows for _, rows in det.stream((frames[:n], P2[:n]) for n in sizes)]
        assert MAX_GRAPHS == 3 and len(det.engine.graphs) == 3 and det.engine.replays == 3 and det.engine.eager_forwards == 1
        for n, rows in zip(sizes, got):
            want = _eager_rows(det, frames[:n], P2[:n])
            assert len(rows) == n and all(a.tobytes() == b.tobytes() for a, b in zip(rows, want)), n
        det.close()
        assert not det.engine.graphs
