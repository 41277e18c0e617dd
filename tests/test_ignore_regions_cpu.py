"""Ignore regions (``dataset.ignore_regions``, ``model.ignore_ioa``) without a GPU: the dataset keys, their way through staging, the flags
from torch operations against the numpy float32 restatement of tests/ignore_reference.py, and the criterion's two formulations that
run on the CPU (``forward_fast`` through plain PyTorch, ``forward_layerwise``) against the float64 reference under a frozen matching.
The routes with HIP kernels are tests/test_ignore_regions_gpu.py's.

Bounds of the float32-against-float64 comparisons: those of tests/test_label_weights_cpu.py, from the arithmetic and not from a run -- a
loss is a sum of at most 3 * 110 * 3 non-negative float32 terms (leaving cells out makes them fewer), each a handful of roundings and
one exp / log (<= 2 ulp each), added pairwise: 32 ulp = 1.9e-6 -> VALUE 2e-6; a gradient row is a few products of such terms: 64 ulp ->
ROW 4e-6; the class logits' rows carry (1 - p_t)**2 log p_t with p_t from a float32 sigmoid: ROW_LOGITS 2e-5."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import criterion_reference as CR
import ignore_reference as IR
import label_weights_reference as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE, ROW, ROW_LOGITS = 2e-6, 4e-6, 2e-5
TINY = 1e-30
MAP_WH = (80, 24)
IOA = 0.5


# ================================================================================================ 1. the dataset
@pytest.fixture()
def kitti_root(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "kitti_dataset.npz"), allow_pickle=False)
    for i, name in enumerate(g["file_names"]):
        path = tmp_path / str(name)
        os.makedirs(path.parent, exist_ok=True)
        path.write_bytes(g["file_%03d" % i].tobytes())
    cfg = dict(json.loads(str(g["cfg_json"])), root_dir=str(tmp_path), writelist=["Car"])
    # two label files rewritten: per file a DontCare, a Van, a Car at depth 80, a Car with truncation 0.8, a Car at the left image
    # border (its box and its 3D centre leave the resampled image under some crops), a Tram, and Cars that are plain targets
    edge = "Car 0.00 0 -1.50 0.00 180.00 %.2f 230.00 1.50 1.60 3.90 %.2f 1.70 20.00 -1.60"
    files = {
        "000003": ["DontCare -1 -1 -10 434.76 165.47 585.85 250.78 -1 -1 -1 -1000 -1000 -1000 -10",
                   "Car 0.00 0 -1.83 583.34 182.67 668.75 217.29 1.47 1.71 4.22 1.30 1.89 30.72 -1.79",
                   "Van 0.00 0 0.65 731.99 183.64 850.66 229.53 1.45 1.59 4.47 4.66 1.79 22.73 0.86",
                   "Car 0.00 0 -1.30 672.90 180.55 753.30 208.30 1.37 1.83 3.76 6.12 1.75 80.00 -1.13",
                   "Tram 0.00 0 -0.52 100.00 150.00 300.00 220.00 3.50 2.50 15.00 -12.00 1.78 25.00 -0.32",
                   "Car 0.80 0 -0.52 900.00 174.00 1100.00 260.00 1.66 1.51 3.84 6.00 1.78 12.00 -0.32",
                   edge % (70.0, -16.9)],
        "000007": [edge % (50.0, -17.1),
                   "Tram 0.00 0 -0.52 100.00 150.00 300.00 220.00 3.50 2.50 15.00 -12.00 1.78 25.00 -0.32",
                   "Car 0.00 0 1.73 373.23 175.80 670.04 297.07 1.51 1.50 3.83 -0.17 1.55 8.83 1.71",
                   "Car 0.80 1 2.36 834.37 170.43 861.08 218.62 1.64 1.54 3.20 20.83 1.43 33.81 2.67",
                   "Van 0.45 2 -1.63 766.94 171.11 814.61 200.40 1.58 1.45 4.23 9.36 1.49 38.74 -1.39",
                   "Car 0.00 0 1.37 547.73 178.10 571.82 222.01 1.29 1.52 3.60 -4.36 1.79 90.00 1.30",
                   "DontCare -1 -1 -10 875.06 168.14 948.42 215.70 -1 -1 -1 -1000 -1000 -1000 -10"],
    }
    for name, lines in files.items():
        (tmp_path / "training" / "label_2" / (name + ".txt")).write_text("\n".join(lines) + "\n")
    return cfg, tmp_path, files


def _expected_boxes(lines, take, info, resolution=(1280, 384)):
    """The ignore boxes of label lines ``take`` from the label text, ``info["flip"]`` and ``info["affine"]``: the 2D box mirrored in
    the image's width, both corners through the affine map, divided by the resolution, clipped to [0, 1]; empty boxes dropped."""
    out = np.zeros((50, 4), np.float32)
    mask = np.zeros(50, bool)
    k = 0
    W = float(info["img_size"][0])
    for i in take:
        box = np.array([float(v) for v in lines[i].split(" ")[4:8]], np.float32)
        if info["flip"]:
            x1, x2 = box[0], box[2]
            box[0], box[2] = W - float(x2), W - float(x1)
        t = np.asarray(info["affine"], np.float64)
        box[:2] = np.dot(t, np.array([box[0], box[1], 1.0], np.float32))[:2]
        box[2:] = np.dot(t, np.array([box[2], box[3], 1.0], np.float32))[:2]
        box = np.clip(box / np.array(resolution * 2, np.float32), 0, 1).astype(np.float32)
        if box[2] <= box[0] or box[3] <= box[1]:
            continue
        out[k], mask[k] = box, True
        k += 1
    return out, mask


def test_dataset_adds_the_boxes_of_known_objects_that_are_no_targets_and_nothing_else(kitti_root):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    cfg, tmp, files = kitti_root
    base = KITTI_Dataset("train", cfg)
    ds = KITTI_Dataset("train", dict(cfg, ignore_regions=True))
    assert ds.ignore_classes == ["DontCare", "Van", "Person_sitting"]
    ids = [i.strip() for i in base.idx_list]
    flips, edge_target, edge_ignored, seen = 0, 0, 0, 0
    for seed in range(8):
        for item, name in enumerate(ids):
            np.random.seed(seed * 100 + item)
            img0, p0, t0, i0 = base[item]
            after0 = np.random.random()
            np.random.seed(seed * 100 + item)
            img1, p1, t1, i1 = ds[item]
            assert np.random.random() == after0                                    # the same draws were consumed
            assert set(t1) == set(t0) | {"ignore_boxes", "ignore_mask"} and set(i1) == set(i0)
            assert all(np.array_equal(t0[k], t1[k]) for k in t0) and np.array_equal(img0, img1) and np.array_equal(p0, p1)
            assert all(np.array_equal(np.asarray(i0[k]), np.asarray(i1[k])) for k in i0)
            boxes, mask = t1["ignore_boxes"], t1["ignore_mask"]
            assert boxes.dtype == np.float32 and boxes.shape == (50, 4) and mask.dtype == bool and mask.shape == (50,)
            lines = files.get(name) or open(os.path.join(base.label_dir, name + ".txt")).read().splitlines()
            cls = [l.split(" ")[0] for l in lines]
            take = [i for i, c in enumerate(cls) if c in ("DontCare", "Van", "Person_sitting") or (c == "Car" and not t0["mask_2d"][i])]
            assert not any(cls[i] in ("Tram", "Pedestrian", "Cyclist", "Misc") for i in take)
            want, want_mask = _expected_boxes(lines, take, i1)
            assert np.array_equal(mask, want_mask) and np.array_equal(boxes, want), (name, seed)
            assert (boxes[~mask] == 0).all() and (boxes >= 0).all() and (boxes <= 1).all()
            flips += int(i1["flip"])
            if name in files:
                seen += 1
                assert t0["mask_2d"].sum() >= 1                                    # the plain Car is a target, so it is no ignore box
                e = [i for i, l in enumerate(lines) if l.startswith("Car 0.00 0 -1.50 0.00")][0]
                edge_target += int(t0["mask_2d"][e])
                edge_ignored += int(e in take)
                assert int(mask.sum()) >= 4                                        # DontCare, Van, far Car, truncated Car
    assert 0 < flips < 8 * len(ids) and seen == 16
    assert edge_target > 0 and edge_ignored > 0, (edge_target, edge_ignored)       # the border Car is both, depending on the crop


def test_dataset_key_is_a_bool_for_the_training_splits_and_the_writelist_wins(kitti_root):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    cfg, tmp, files = kitti_root
    for bad in (1, "true", 0.5, [True]):
        with pytest.raises(ValueError, match="ignore_regions"):
            KITTI_Dataset("train", dict(cfg, ignore_regions=bad))
    with pytest.raises(ValueError, match="ignore_classes"):
        KITTI_Dataset("train", dict(cfg, ignore_regions=True, ignore_classes="Van"))
    for off in (None, False):
        np.random.seed(3)
        assert "ignore_boxes" not in KITTI_Dataset("train", dict(cfg, ignore_regions=off))[0][2]
    assert "ignore_boxes" not in KITTI_Dataset("val", dict(cfg, ignore_regions=True))[0][2]
    assert KITTI_Dataset("val", dict(cfg, ignore_regions="x")).ignore_regions is False
    assert "ignore_regions" not in yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["dataset"]
    # class_merging puts Van into the writelist: the Van of 000003 becomes a target and leaves the ignore boxes
    plain = KITTI_Dataset("train", dict(cfg, ignore_regions=True, random_flip=0.0, random_crop=0.0))
    merged = KITTI_Dataset("train", dict(cfg, ignore_regions=True, random_flip=0.0, random_crop=0.0, class_merging=True))
    assert "Van" not in merged.ignore_classes and "DontCare" in merged.ignore_classes
    item = [i.strip() for i in plain.idx_list].index("000003")
    van = [i for i, l in enumerate(files["000003"]) if l.startswith("Van")][0]
    _, _, tp, ip = plain[item]
    _, _, tm, im = merged[item]
    assert not tp["mask_2d"][van] and tm["mask_2d"][van]
    assert int(tp["ignore_mask"].sum()) == int(tm["ignore_mask"].sum()) + 1
    van_box = _expected_boxes(files["000003"], [van], ip)[0][0]
    assert (tp["ignore_boxes"] == van_box).all(1).any() and not (tm["ignore_boxes"] == van_box).all(1).any()
    # use_dontcare does the same for DontCare
    assert "DontCare" not in KITTI_Dataset("train", dict(cfg, ignore_regions=True, use_dontcare=True)).ignore_classes


def test_loader_batches_carry_the_boxes_to_the_criterion_batchwise(kitti_root):
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.synthetic import prepare_targets
    cfg, tmp, files = kitti_root
    cfg = dict(cfg, type="KITTI", train_split="train", test_split="val", batch_size=3, ignore_regions=True)
    train_loader, test_loader = build_dataloader(cfg, workers=0)
    np.random.seed(0)
    raw = next(iter(train_loader))
    assert raw[2]["ignore_boxes"].shape == (3, 50, 4) and raw[2]["ignore_boxes"].dtype == torch.float32
    assert raw[2]["ignore_mask"].shape == (3, 50) and raw[2]["ignore_mask"].dtype == torch.bool and raw[2]["ignore_mask"].any()
    staged = stage_batch(raw, torch.device("cpu"))[2]
    tl = prepare_targets(staged, 3)
    assert torch.equal(tl.ignore[0], raw[2]["ignore_boxes"]) and torch.equal(tl.ignore[1], raw[2]["ignore_mask"])
    assert all("ignore_boxes" not in t and "ignore_mask" not in t for t in tl) and "ignore_boxes" not in tl.flat
    plain = prepare_targets({k: v for k, v in staged.items() if not k.startswith("ignore_")}, 3)
    assert plain.ignore is None and [len(t["labels"]) for t in plain] == [len(t["labels"]) for t in tl]
    # a batch in which no image has an ignore box is a batch without the keys
    empty = dict(raw[2], ignore_mask=torch.zeros_like(raw[2]["ignore_mask"]))
    assert prepare_targets(stage_batch((raw[0], raw[1], empty, raw[3]), torch.device("cpu"))[2], 3).ignore is None
    assert "ignore_boxes" not in next(iter(test_loader))[2]


# ================================================================================================ 2. the flags
_FLAG_CASES = {"single": (1, 1, 5, 1, None), "three_images": (2, 3, 70, 3, 1), "full_slots": (3, 3, 400, 50, None)}


@pytest.mark.parametrize("name", list(_FLAG_CASES))
def test_torch_flags_equal_the_numpy_float32_restatement(name):
    from monosowa_amd.pointwise import ignore_flags
    NL, B, Q, M, empty = _FLAG_CASES[name]
    boxes, ign, mask = IR.make_flag_case(40 + NL, NL, B, Q, M, empty_image=empty)
    want, want_n = IR.flags(boxes, ign, mask, IOA)
    got, got_n = ignore_flags(torch.from_numpy(boxes), torch.from_numpy(ign), torch.from_numpy(mask), IOA)
    assert got.dtype == torch.uint8 and got.shape == (NL, B, Q) and got_n.shape == (NL,)
    assert np.array_equal(got.numpy(), want) and np.array_equal(got_n.numpy(), want_n)
    if M == 1:
        assert tuple(want[0, 0, :5]) == IR.PLANTED_FLAGS              # == ioa A: in; one ulp below: out; zero area, NaN: out
    assert 0 < want.sum() < want.size
    if empty is not None:
        assert not want[:, empty].any() and want[:, [b for b in range(B) if b != empty]].any()
    # random (non-dyadic) boxes, where products and sums round
    rng = np.random.default_rng(7)
    rb = np.concatenate([rng.uniform(0.1, 0.9, (NL, B, Q, 2)), rng.uniform(0.0, 0.15, (NL, B, Q, 4))], -1).astype(np.float32)
    lo = rng.uniform(0, 0.7, (B, M, 2))
    rg = np.concatenate([lo, lo + rng.uniform(0.02, 0.3, (B, M, 2))], -1).astype(np.float32)
    for ioa in (0.5, 0.3, 1.0):
        want, want_n = IR.flags(rb, rg, mask, ioa)
        got, got_n = ignore_flags(torch.from_numpy(rb), torch.from_numpy(rg), torch.from_numpy(mask), ioa)
        assert np.array_equal(got.numpy(), want) and np.array_equal(got_n.numpy(), want_n)
    # an all-false mask, and a NaN in every ignore box
    none, n0 = ignore_flags(torch.from_numpy(rb), torch.from_numpy(rg), torch.zeros((B, M), dtype=torch.bool), IOA)
    assert not none.any() and not n0.any() and not IR.flags(rb, rg, np.zeros((B, M), bool), IOA)[0].any()
    bad = rg.copy()
    bad[..., 0] = np.nan
    assert not ignore_flags(torch.from_numpy(rb), torch.from_numpy(bad), torch.from_numpy(mask), IOA)[0].any()
    assert not IR.flags(rb, bad, mask, IOA)[0].any()


# ================================================================================================ 3. the criterion
class _Replay(torch.nn.Module):
    """Records the [3, NL, K] triples of the first ``forward_fast`` matching and replays them to both formulations."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.idx, self.calls = inner, None, 0

    def match_layers_begin(self, *args, **kwargs):
        return self.inner.match_layers_begin(*args, **kwargs)

    def match_layers_end_flat(self, handle):
        got = self.inner.match_layers_end_flat(handle)
        if self.idx is None:
            self.idx = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).copy()
        return self.idx.copy()

    def forward(self, outputs, targets, group_num=1):
        layer = self.calls % self.idx.shape[1]
        self.calls += 1
        offs = np.concatenate([[0], np.cumsum([len(t["labels"]) for t in targets])])
        b, q, t = self.idx[:, layer]
        return [(torch.from_numpy(q[b == i]), torch.from_numpy(t[b == i] - offs[i])) for i in range(len(targets))]


def _criterion(fast, train=True, **model_cfg):
    from monosowa_amd.monodetr import build_weight_dict
    from monosowa_amd.monodetr.criterion import SetCriterion
    from monosowa_amd.monodetr.matcher import build_matcher
    cfg = dict(yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["model"], **model_cfg)
    losses = ["labels", "boxes", "cardinality", "depths", "dims", "angles", "center", "depth_map", "tfl"]
    crit = SetCriterion(cfg["num_classes"], _Replay(build_matcher(cfg)), build_weight_dict(cfg), cfg["focal_alpha"], losses, cfg=cfg,
                        fast=fast, depth_map_size=MAP_WH)
    return crit.train(train)


def _evaluate(crit, outputs, targets, ignore=None, dtype=torch.float32):
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import TargetList
    out, tg = CR.cast_case(outputs, targets, "cpu", dtype)
    tg = TargetList(tg)
    if ignore is not None:
        tg.ignore = (torch.from_numpy(ignore[0]), torch.from_numpy(ignore[1]))
    losses = crit(out, tg)
    total = weighted_total(losses, crit.weight_dict)
    leaves = CR.leaves_of(out)
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
    return {k: losses[k].detach().clone() for k in losses.keys()}, total.detach(), grads


def _reference(crit, outputs, targets, idx, group_num, ignore):
    out, tg = CR.cast_case(outputs, targets, "cpu", torch.float64)
    w = torch.cat([t["label_weight"] for t in targets]) if "label_weight" in targets[0] else torch.ones(sum(len(t["labels"]) for t in targets))
    n = LW.num_boxes(w, group_num)
    want, ignored = IR.criterion_losses(out, tg, torch.from_numpy(idx), n, crit.focal_alpha, MAP_WH, ignore[0], ignore[1], IOA)
    total = sum(want[k] * float(crit.weight_dict[k]) for k in want if k in crit.weight_dict)
    leaves = CR.leaves_of(out)
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {n_: (torch.zeros_like(v) if g is None else g).detach() for (n_, v), g in zip(leaves.items(), grads)}
    return {k: float(v.detach()) for k, v in want.items()}, float(total.detach()), grads, ignored


def ignore_boxes_for(outputs, seed, empty_image=1, M=6, valid=3):
    """[B, M, 4] ignore boxes with ``valid`` filled slots per image (none in ``empty_image``): windows of 0.15 .. 0.35 of the image."""
    B = outputs["pred_boxes"].shape[0]
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.05, 0.6, (B, M, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(0.15, 0.35, (B, M, 2))], -1).astype(np.float32)
    mask = np.zeros((B, M), bool)
    mask[:, :valid] = True
    if empty_image is not None:
        mask[empty_image] = False
    boxes[~mask] = 0
    return boxes, mask


def _is_ce(key):
    return key == "loss_ce" or key.startswith("loss_ce_")


# name -> (targets per image, queries, train mode, seed)
_LAYOUTS = {"mixed_train": ([0, 9, 1, 4], 110, True, 310), "eval_q50": ([5, 0, 10], 50, False, 311)}


def _case(name, weighted):
    sizes, Q, train, seed = _LAYOUTS[name]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    if weighted:
        targets = LW.with_weights(targets, LW.draw_weights(seed + 1000, sum(sizes)))
    return outputs, targets, train, ignore_boxes_for(outputs, seed + 2000)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_both_cpu_formulations_equal_the_float64_reference_under_a_frozen_matching(name, weighted):
    outputs, targets, train, ignore = _case(name, weighted)
    fast = _criterion(True, train)
    vF, tF, gF = _evaluate(fast, outputs, targets, ignore)
    idx = fast.matcher.idx
    groups = fast.group_num if train else 1
    slow = _criterion(False, train)
    slow.matcher.idx = idx
    vL, tL, gL = _evaluate(slow, outputs, targets, ignore)
    assert slow.matcher.calls == 3
    vR, tR, gR, ignored = _reference(fast, outputs, targets, idx, groups, ignore)
    n_ignored = ignored.sum((1, 2)).tolist()
    assert min(n_ignored) > 0 and not ignored[:, 1].any()                    # image 1 has no ignore box
    assert fast.ignore_report() == (n_ignored, ignored[0].numel()) == slow.ignore_report()
    bad = []
    for tag, v, t, g in (("fast", vF, tF, gF), ("layerwise", vL, tL, gL)):
        assert set(vR) <= set(v)
        for k, ref in vR.items():
            if k.startswith(("class_error", "cardinality_error")):
                assert abs(float(v[k]) - ref) <= 2.0 ** -22 * 100.0, (tag, k)
            else:
                e = abs(float(v[k]) - ref) / max(abs(ref), TINY)
                if e > VALUE:
                    bad.append((tag, k, e))
        if abs(float(t) - tR) / max(abs(tR), TINY) > VALUE:
            bad.append((tag, "total", float(t), tR))
        for n, ref in gR.items():
            rows = (lambda x: x.permute(0, 2, 3, 1)) if n == "depth_map_logits" else (lambda x: x)
            e = CR.row_error(rows(g[n]), rows(ref))
            print("MEASURED %s %-10s %-24s row error %.3e" % (name, tag, n, e))
            if e > (ROW_LOGITS if n.endswith("pred_logits") else ROW):
                bad.append((tag, n, e))
        for l in range(3):                                                   # an ignored cell's logit gradients are +0.0
            rows = g["l%d.pred_logits" % l][ignored[l]]
            assert rows.numel() and (rows == 0).all() and not torch.signbit(rows).any(), (tag, l)
    assert not bad, bad


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "layerwise"])
def test_boxes_that_flag_nothing_leave_every_loss_and_gradient_bit_for_bit(fast, weighted):
    outputs, targets, train, ignore = _case("mixed_train", weighted)
    crit = _criterion(True, train)
    _evaluate(crit, outputs, targets)                                        # records the matching
    idx = crit.matcher.idx
    if not fast:
        crit = _criterion(False, train)
        crit.matcher.idx = idx
    v0, t0, g0 = _evaluate(crit, outputs, targets)
    assert crit.ignore_report() is None
    # valid boxes that no query box reaches with half its area: slivers, and boxes outside the unit square
    far = (np.array([[[0.0, 0.0, 1.0, 2.0 ** -12], [1.5, 1.5, 2.0, 2.0]]] * 4, np.float32), np.ones((4, 2), bool))
    assert not IR.flags(CR.stack_layers(outputs)["pred_boxes"].detach().numpy(), far[0], far[1], IOA)[0].any()
    v1, t1, g1 = _evaluate(crit, outputs, targets, far)
    assert crit.ignore_report() == ([0, 0, 0], 4 * 110)
    assert set(v0) == set(v1) and len(v0) > 20
    assert all(torch.equal(v0[k], v1[k]) for k in v0) and torch.equal(t0, t1)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    # boxes that do flag change loss_ce of every layer and nothing else in the dictionary
    v2, _, g2 = _evaluate(crit, outputs, targets, ignore)
    for k in v0:
        assert torch.equal(v0[k], v2[k]) != _is_ce(k), k
    assert all(torch.equal(g0[n], g2[n]) != n.endswith("pred_logits") for n in g0)


def test_a_flagged_cell_that_is_matched_keeps_its_terms_and_the_logging_entries_see_every_cell():
    outputs, targets, train, _ = _case("mixed_train", False)
    crit = _criterion(True, train)
    v0, t0, g0 = _evaluate(crit, outputs, targets)
    idx = crit.matcher.idx
    everything = (np.array([[[-1.0, -1.0, 2.0, 2.0]]] * 4, np.float32), np.ones((4, 1), bool))      # every query box lies inside
    flag = IR.flags(CR.stack_layers(outputs)["pred_boxes"].detach().numpy(), everything[0], everything[1], IOA)[0]
    assert flag.all()
    v1, t1, g1 = _evaluate(crit, outputs, targets, everything)
    K = idx.shape[2]
    assert crit.ignore_report() == ([4 * 110 - K] * 3, 4 * 110)
    for k in v0:
        assert torch.equal(v0[k], v1[k]) != _is_ce(k), k                              # class / cardinality errors too
    # loss_ce is now the matched cells' terms alone: the float64 reference with every unmatched cell left out
    vR, _, gR, ignored = _reference(crit, outputs, targets, idx, crit.group_num, everything)
    for l in range(3):
        k = "loss_ce" if l == 0 else "loss_ce_%d" % (l - 1)
        assert abs(float(v1[k]) - vR[k]) <= VALUE * abs(vR[k]) and 0 < float(v1[k]) < float(v0[k])
        g = g1["l%d.pred_logits" % l]
        b, q = torch.from_numpy(idx[0, l]), torch.from_numpy(idx[1, l])
        assert torch.equal(g[b, q], g0["l%d.pred_logits" % l][b, q]) and (g[b, q].abs().sum(1) > 0).all()
        assert (g[ignored[l]] == 0).all() and int(ignored[l].sum()) == 4 * 110 - K
    # num_boxes is the label count, whatever the ignore boxes
    from monosowa_amd.synthetic import TargetList
    tl = TargetList(targets)
    n = crit._num_boxes(tl, 11, torch.device("cpu"))
    tl.ignore = (torch.from_numpy(everything[0]), torch.from_numpy(everything[1]))
    assert crit._num_boxes(tl, 11, torch.device("cpu")) == n == 14 * 11.0


def test_a_non_finite_logit_in_an_ignored_cell_reaches_nothing():
    outputs, targets, train, ignore = _case("mixed_train", False)
    crit = _criterion(True, train)
    _evaluate(crit, outputs, targets, ignore)
    idx = crit.matcher.idx
    flag = IR.flags(CR.stack_layers(outputs)["pred_boxes"].detach().numpy(), ignore[0], ignore[1], IOA)[0]
    ignored = IR.ignored_cells(flag, torch.from_numpy(idx))
    poisoned = {k: v.clone() if torch.is_tensor(v) else [dict(o) for o in v] for k, v in outputs.items()}
    b, q = [int(x[0]) for x in torch.nonzero(ignored[0], as_tuple=True)]
    poisoned["pred_logits"][b, q] = torch.tensor([float("inf"), float("nan"), -float("inf")])
    for fast in (True, False):
        c = _criterion(fast, train)
        c.matcher.idx = idx
        v, t, g = _evaluate(c, poisoned, targets, ignore)
        assert torch.isfinite(t) and all(torch.isfinite(v[k]) for k in v if k.startswith("loss_"))
        assert all(torch.isfinite(x).all() for x in g.values()) and (g["l0.pred_logits"][b, q] == 0).all()


def test_ignore_ioa_is_checked_when_the_criterion_is_built():
    assert _criterion(True).ignore_ioa == 0.5 and _criterion(True, ignore_ioa=1).ignore_ioa == 1.0
    assert _criterion(False, ignore_ioa=0.25).ignore_ioa == 0.25
    assert "ignore_ioa" not in yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["model"]
    for bad in (0, 0.0, -0.5, 1.5, "0.5", None, True, float("nan")):
        with pytest.raises(ValueError, match="ignore_ioa"):
            _criterion(True, ignore_ioa=bad)
