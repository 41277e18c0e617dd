"""mono_fuse_dets_f64 (csrc/fuse_dets.h) and the tester.nms_iou / flip_tta / fuse keys on the GPU.

The kernel against the restatement of tests/fuse_reference.py on generated rows (test_fuse_cpu.py checks the generator); the Detector
and the Tester with the keys against a keys-off Detector whose rows go through the same restatement.  The end-to-end comparisons
run under torch.use_deterministic_algorithms(True) with ``threshold: 0.0``, for the reasons test_detector_gpu.py gives."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

import fuse_reference as FR
import test_detector_gpu as G

pytestmark = pytest.mark.gpu
MIRRORED = [1, 2, 4, 9, 12]                                              # the columns un-mirroring rewrites
KEPT = [c for c in range(14) if c not in MIRRORED]
CASES = [(7, 1), (7, 2), (50, 1), (50, 2), (128, 2)]                     # (128, 2): the 256 candidates the kernel takes at most


def _at_offset(array, offset, dev):
    """The array on the device, ``offset`` elements into a larger allocation."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _empty_at_offset(shape, dtype, offset, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), 77, dtype=dtype, device=dev)
    return buf[offset:offset + n].view(shape)


def _device_fuse(case, mode, offset=0):
    from monosowa_amd.fuse import fuse_rows_device
    dev = G._dev()
    B, K, V = 3, case["K"], case["views"]
    out = fuse_rows_device(_at_offset(case["rows"], offset, dev), _at_offset(case["count"], offset, dev), _at_offset(case["geom"], offset, dev),
                           case["iou"], mode, V, _empty_at_offset((B, V * K, 14), torch.float64, offset, dev),
                           _empty_at_offset((B,), torch.int32, offset, dev), _empty_at_offset((B, V * K), torch.int32, offset, dev))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_image(got_rows, got_n, got_support, img, K, want, mode, what, ry_bound=None):
    """One image's output against the restatement's (seeds, rows, support): selection, order, count and support exact; 'seed' rows
    of view 0 byte-equal to the input rows, of view 1 byte-equal in the columns un-mirroring keeps; everything within 1e-9."""
    seeds, rows, support = want
    n = len(seeds)
    assert got_n == n, (what, got_n, n)
    assert got_support[:n].tolist() == support.tolist() and not got_support[n:].any(), what
    assert not got_rows[n:].any(), (what, "the tail must be zero")
    np.testing.assert_allclose(got_rows[:n], rows, rtol=0, atol=1e-9, equal_nan=True, err_msg=str(what))
    if mode != "seed":
        return
    for s, q in enumerate(seeds):
        if img["ids"][q] < K:
            assert got_rows[s].tobytes() == img["cands"][q].tobytes(), (what, s)
        else:
            assert got_rows[s, KEPT].tobytes() == img["cands"][q, KEPT].tobytes(), (what, s)
        if ry_bound is not None and abs(abs(rows[s, 12]) - math.pi) > G.NEAR_PI:
            assert abs(got_rows[s, 12] - rows[s, 12]) <= ry_bound, (what, s, got_rows[s, 12] - rows[s, 12], ry_bound)


@pytest.mark.parametrize("mode", ["seed", "mean"])
@pytest.mark.parametrize("K,views", CASES)
def test_fuse_kernel_equals_the_restatement(K, views, mode):
    case = FR.kernel_case(K, views, 0.5)
    above, below = FR.in_cluster_split(case)
    assert above >= 0.3 * (above + below) and below > 0
    rows, count, support = _device_fuse(case, mode)
    assert count.dtype == np.int32 and support.dtype == np.int32 and rows.shape == (3, views * K, 14)
    merged = 0
    for b, want in enumerate(FR.reference(case, mode)):
        _assert_image(rows[b], count[b], support[b], case["images"][b], K, want, mode, (K, views, mode, b))
        merged += int((want[2] > 1).sum())
    assert count[1] == 0 and merged >= 2
    print("K %d, V %d, %s: %s rows from %s candidates, %d clusters of more than one" % (K, views, mode, count.tolist(),
                                                                                       [len(i["ids"]) for i in case["images"]], merged))


@pytest.mark.parametrize("mode", ["seed", "mean"])
def test_fuse_kernel_merges_near_twins_as_the_restatement_does(mode):
    """Pairs one ulp apart, turned by float32 pi, collinear and of the same width (FR.twin_case): no two rows are bit-equal, so
    every flag comes from the overlap routine, and each pair must end as one cluster of two."""
    case = FR.twin_case()
    rows, count, support = _device_fuse(case, mode)
    for b, want in enumerate(FR.reference(case, mode)):
        img = case["images"][b]
        pairs = len(img["ids"]) // 2
        assert [img["labels"][q] for q in want[0]] == list(range(pairs)) and want[2].tolist() == [2] * pairs, (b, want[0], want[2])
        _assert_image(rows[b], count[b], support[b], img, case["K"], want, mode, ("twins", mode, b))
    assert count.tolist() == [len(FR.TWIN_KINDS), 0, len(FR.TWIN_KINDS)]


@pytest.mark.parametrize("mode", ["seed", "mean"])
def test_fuse_kernel_writes_the_same_bytes_wherever_the_buffers_lie(mode):
    case = FR.kernel_case(50, 2, 0.5)
    first = _device_fuse(case, mode, offset=0)
    for offset in (1, 3):                                                # 8 / 24 bytes (rows), 4 / 12 bytes (counts) off the allocation
        again = _device_fuse(case, mode, offset=offset)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), offset


def test_fuse_entry_point_refuses_null_pointers_and_bad_sizes():
    from monosowa_amd.fuse import fuse_rows_device
    from monosowa_amd.kitti_eval import load
    fn = load().mono_fuse_dets_f64
    dev = G._dev()
    r, c, g = torch.zeros((2, 4, 14), dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros((2, 10), dtype=torch.float64, device=dev)
    o, n, s = torch.zeros((2, 4, 14), dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros((2, 4), dtype=torch.int32, device=dev)
    ptrs = [t.data_ptr() for t in (r, c, g)], [t.data_ptr() for t in (o, n, s)]
    call = lambda a=ptrs[0], b=ptrs[1], iou=0.5, mode=0, B=2, K=4, V=1: fn(a[0], a[1], a[2], iou, mode, b[0], b[1], b[2], B, K, V, None)
    for k in range(3):
        assert call(a=[p if i != k else None for i, p in enumerate(ptrs[0])]) == -1
        assert call(b=[p if i != k else None for i, p in enumerate(ptrs[1])]) == -1
    for bad in ({"B": 0}, {"K": 0}, {"V": 0}, {"V": 3}, {"K": 257}, {"K": 129, "V": 2}, {"mode": 2}, {"mode": -1}, {"iou": 0.0}, {"iou": 1.5},
                {"iou": float("nan")}):
        assert call(**bad) == -2, bad
    assert call() == 0
    torch.cuda.synchronize()
    assert n.tolist() == [0, 0] and not o.any()
    with pytest.raises(ValueError, match="at most 256"):
        fuse_rows_device(torch.zeros((2, 129, 14), dtype=torch.float64, device=dev), c, g[:1], 0.5, "seed", 2)
    assert isinstance(fn, ctypes._CFuncPtr)


# ================================================================================================ end to end
@pytest.fixture(scope="module")
def world(golden_dir, tmp_path_factory):
    """The fixtures, model and validation frames of test_detector_gpu.py, once for this module."""
    root = tmp_path_factory.mktemp("fuse_kitti")
    fixtures = G.write_kitti_root(golden_dir, root)
    model, _, cfg = G._model()
    loader = G._val_loader(fixtures, root, 3, device_aug=True)
    ids, frames, P2 = G._frames_of(loader)
    return {"fixtures": fixtures, "root": root, "model": model, "cfg": cfg, "loader": loader, "ids": ids, "frames": frames[:3], "P2": P2[:3],
            "all_frames": frames, "all_P2": P2}


@pytest.fixture(scope="module")
def keys_off(world):
    """The references of the end-to-end tests, computed once and left unchanged: a keys-off Detector's rows of the three frames
    (one batch of B) and of frames + mirrored frames (ONE batch of 2 B: the same forward as a flip_tta batch), under
    use_deterministic_algorithms; per number of views the restatement's candidates and overlaps and the threshold they admit."""
    frames, P2 = world["frames"], world["P2"]
    B = len(frames)
    with G.deterministic():
        off = _detector(world)
        one = off.detect(frames, P2, batch_size=B)
        two = off.detect(frames + [np.ascontiguousarray(f[:, ::-1]) for f in frames], np.concatenate([P2, P2]), batch_size=2 * B)
        geom = _geom(off, frames, P2)
        off.close()
    assert all(len(r) == 50 for r in one + two)
    out = {"geom": geom, "dataset": off.dataset, "rows": {1: one, 2: two}, "images": {}, "threshold": {}}
    for views, rows in out["rows"].items():
        out["images"][views] = _restated(rows, geom, views)
        out["threshold"][views] = _threshold(out["images"][views])
    return out


def _detector(world, **keys):
    from monosowa_amd import Detector
    return Detector({"dataset": G._dataset_cfg(world["fixtures"], world["root"], 3), "tester": dict(G.TESTER_CFG, **keys),
                     "model": world["cfg"]["model"]}, model=world["model"])


def _restated(rows_by_view, geom, views):
    """Keys-off rows (a list per view and image, [n, 14]) -> per image the generator's dict (ids, cands, ious)."""
    B, K = len(rows_by_view) // views, 50
    rows, count = np.zeros((views * B, K, 14)), np.zeros(views * B, dtype=np.int32)
    for k, r in enumerate(rows_by_view):
        rows[k, :len(r)], count[k] = r, len(r)
    images = []
    for b in range(B):
        ids, cands = FR.candidates(rows, count, geom, b, views)
        images.append({"ids": ids, "cands": cands, "ious": FR.same_class_ious(cands)})
    return images


def _threshold(images):
    """The first of 0.05, 0.1, ..., 0.7 that every same-class pair keeps the margin from."""
    for k in range(1, 15):
        thr = round(0.05 * k, 2)
        if all(math.isnan(v) or abs(v - thr) > FR.MARGIN for img in images for v in img["ious"].values()):
            return thr
    raise AssertionError("no threshold in 0.05 .. 0.7 keeps every pair %g away" % FR.MARGIN)


def _geom(det, frames, P2):
    return det._batch(frames, P2, 0)[3].numpy()


@pytest.mark.parametrize("mode", ["seed", "mean"])
def test_flip_tta_equals_the_restatement_on_the_keys_off_rows_of_both_views(world, keys_off, mode):
    """Reference: a keys-off Detector on frames + mirrored frames in ONE batch of 2 B (the same forward as the flip_tta batch), its
    rows through the restatement.  In 'seed' mode ry is also held to test_detector_gpu.py's bound (4 x the atan2 difference
    alone); 'mean' sends ry through sin, cos and a second atan2, so 1e-9 is its bound."""
    frames, P2 = world["frames"], world["P2"]
    B = len(frames)
    images, geom, thr = keys_off["images"][2], keys_off["geom"], keys_off["threshold"][2]
    with G.deterministic():
        on = _detector(world, nms_iou=thr, flip_tta=True, fuse=mode)
        got, members = on.detect(frames, P2, batch_size=B, support=True)
        assert on.engine.replays == 1 and on.engine.eager_forwards == 0 and len(on.engine.graphs) == 1
        on.close()
    bound = G._ry_bound(frames, P2, keys_off["dataset"], keys_off["rows"][2][:B])
    merged = mirrored = 0
    for b in range(B):
        want = FR.fuse(images[b]["ids"], images[b]["cands"], images[b]["ious"], 50, geom[b], thr, mode, 2)
        rows, support = np.zeros((100, 14)), np.zeros(100, dtype=np.int32)
        rows[:len(got[b])], support[:len(got[b])] = got[b], members[b]
        _assert_image(rows, len(got[b]), support, images[b], 50, want, mode, ("flip", mode, b), ry_bound=bound)
        merged += int((want[2] > 1).sum())
        mirrored += sum(1 for q in want[0] if images[b]["ids"][q] >= 50)
    print("flip_tta, %s: threshold %.2f, ry bound %.3e, %s rows, %d clusters of more than one, %d seeds from the mirrored view"
          % (mode, thr, bound, [len(r) for r in got], merged, mirrored))


def test_nms_only_equals_the_restatement_on_the_keys_off_rows(world, keys_off):
    frames, P2 = world["frames"], world["P2"]
    images, geom, thr = keys_off["images"][1], keys_off["geom"], keys_off["threshold"][1]
    with G.deterministic():
        on = _detector(world, nms_iou=thr)
        got, members = on.detect(frames, P2, batch_size=3, support=True)
        on.close()
    for b in range(3):
        want = FR.fuse(images[b]["ids"], images[b]["cands"], images[b]["ious"], 50, geom[b], thr, "seed", 1)
        rows, support = np.zeros((50, 14)), np.zeros(50, dtype=np.int32)
        rows[:len(got[b])], support[:len(got[b])] = got[b], members[b]
        _assert_image(rows, len(got[b]), support, images[b], 50, want, "seed", ("nms", b))
    print("nms_iou %.2f: %s rows of 50" % (thr, [len(r) for r in got]))


def test_more_candidates_than_the_kernel_takes_are_fused_on_the_host(world):
    """topk 150 with flip_tta: 300 candidates per image, over the kernel's 256 -- the engine fuses the unfused rows with
    ``fuse_rows_host`` when the batch completes, and gives what that function gives on a keys-off Detector's rows of both views."""
    from monosowa_amd import Detector
    from monosowa_amd.fuse import MAX_CANDIDATES, fuse_rows_host
    frames, P2 = world["frames"][:2], world["P2"][:2]
    make = lambda **keys: Detector({"dataset": G._dataset_cfg(world["fixtures"], world["root"], 2), "tester": dict(G.TESTER_CFG, topk=150, **keys),
                                    "model": world["cfg"]["model"]}, model=world["model"])
    assert 2 * 150 > MAX_CANDIDATES
    with G.deterministic():
        off = make()
        base = off.detect(frames + [np.ascontiguousarray(f[:, ::-1]) for f in frames], np.concatenate([P2, P2]), batch_size=4)
        geom = _geom(off, frames, P2)
        off.close()
        on = make(nms_iou=0.3, flip_tta=True, fuse="mean")
        got, members = on.detect(frames, P2, batch_size=2, support=True)
        on.close()
    assert all(r.shape == (150, 14) for r in base)
    want, count, support = fuse_rows_host(np.stack(base), np.full(4, 150, dtype=np.int32), geom, 0.3, "mean", 2)
    for b in range(2):
        assert got[b].tobytes() == want[b, :count[b]].tobytes() and members[b].tolist() == support[b, :count[b]].tolist()
        assert members[b].sum() == 300


def test_tester_inference_with_the_keys_writes_the_detectors_files(world, tmp_path):
    from monosowa_amd.helpers.tester_helper import Tester
    keys = {"nms_iou": 0.3, "flip_tta": True, "fuse": "mean"}
    with G.deterministic():
        det = _detector(world, **keys)
        rows = det.detect(world["all_frames"], world["all_P2"], batch_size=3)
        det.write_kitti(rows, world["ids"], tmp_path / "detector")
        det.close()
        tester = Tester(dict(G.TESTER_CFG, **keys), world["model"], world["loader"], G.logging.getLogger("fuse"), {"save_path": str(tmp_path) + "/"}, "m")
        tester.output_dir = str(tmp_path / "tester")
        results = tester.inference()
    assert [int(k) for k in results] == world["ids"]
    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "detector" / "*.txt")))
    assert names == ["%06d.txt" % i for i in world["ids"]]
    assert names == sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "tester" / "outputs" / "data" / "*.txt")))
    for name in names:
        a = (tmp_path / "detector" / name).read_bytes()
        assert a and a == (tmp_path / "tester" / "outputs" / "data" / name).read_bytes(), name


def test_stream_with_the_keys_does_not_synchronise_the_device(world, monkeypatch):
    frames, P2 = world["all_frames"], world["all_P2"]
    det = _detector(world, nms_iou=0.3, flip_tta=True, fuse="mean")
    batches = [([frames[2 * k], frames[2 * k + 1]], P2[[2 * k, 2 * k + 1]]) for k in range(2)]
    assert sum(len(r) for _, r in det.stream(batches)) == 4              # warm: the capture of this batch size
    calls = [0]
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), real(*a, **k))[1])
    replays = det.engine.replays
    assert sum(len(r) for _, r in det.stream(batches)) == 4
    monkeypatch.undo()
    assert calls[0] == 0 and det.engine.replays - replays == 2
    det.close()


def _kernel_names(det, frames, P2):
    from torch.profiler import ProfilerActivity, profile
    det.detect(frames, P2, batch_size=len(frames))                       # warm: capture
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        det.detect(frames, P2, batch_size=len(frames))
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_no_fuse_launch_with_the_keys_absent(world):
    frames, P2 = world["frames"][:2], world["P2"][:2]
    off = _detector(world)
    names_off = _kernel_names(off, frames, P2)
    off.close()
    on = _detector(world, nms_iou=0.3)
    names_on = _kernel_names(on, frames, P2)
    on.close()
    count = lambda names, what: sum(what in n for n in names)
    assert count(names_off, "decode_dets_kernel") == count(names_on, "decode_dets_kernel") == 1      # the profiler sees the library's launches
    assert count(names_off, "fuse_dets") == 0 and count(names_on, "fuse_dets_kernel") == 1
