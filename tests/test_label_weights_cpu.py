"""Per-label loss weights (``label_weight``, ``dataset.label_weights``) without a GPU: the criterion's two formulations that run on
the CPU (``forward_fast`` through the plain PyTorch route and ``forward_layerwise``; the two routes with HIP kernels are
tests/test_label_weights_gpu.py's) against the float64 reference of tests/label_weights_reference.py under a frozen matching, the
all-ones identity, the weighted normaliser, the dataset key and the ``weights`` subcommand of tools/label_audit.py.

Bounds of the float32-against-float64 comparisons (metrics of tests/test_criterion_kernels_gpu.py), from the arithmetic, not from a run:
a loss is a sum of at most 3 * 110 * 3 non-negative float32 terms, each a handful of roundings and one exp / log (<= 2 ulp each), added
pairwise: 32 ulp = 32 * 2**-24 = 1.9e-6 -> VALUE 2e-6.  A gradient row is a few products of such terms: 64 ulp = 3.8e-6 -> ROW 4e-6;
the class logits' rows carry (1 - p_t)**2 * log p_t with p_t from a float32 sigmoid, whose relative error at |x| ~ 8 is e**8 ulp of
the 1 - p side: ROW_LOGITS 2e-5, the bound the unweighted expressions have there (C_LOGITS)."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import criterion_reference as CR
import label_weights_reference as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE, ROW, ROW_LOGITS = 2e-6, 4e-6, 2e-5
TINY = 1e-30
MAP_WH = (80, 24)


class _Replay(torch.nn.Module):
    """Records the [3, NL, K] triples of the first ``forward_fast`` matching and replays them to both formulations: the flat
    interface, and the per-layer call of ``forward_layerwise`` (final layer first, then the auxiliary ones)."""

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


def _criterion(fast, train=True):
    from monosowa_amd.monodetr import build_weight_dict
    from monosowa_amd.monodetr.criterion import SetCriterion
    from monosowa_amd.monodetr.matcher import build_matcher
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["model"]
    losses = ["labels", "boxes", "cardinality", "depths", "dims", "angles", "center", "depth_map", "tfl"]
    crit = SetCriterion(cfg["num_classes"], _Replay(build_matcher(cfg)), build_weight_dict(cfg), cfg["focal_alpha"], losses, cfg=cfg,
                        fast=fast, depth_map_size=MAP_WH)
    return crit.train(train)


def _rel(x, ref):
    return abs(float(x) - float(ref)) / max(abs(float(ref)), TINY)


def _evaluate(crit, outputs, targets, dtype):
    from monosowa_amd.monodetr.criterion import weighted_total
    out, tg = CR.cast_case(outputs, targets, "cpu", dtype)
    losses = crit(out, tg)
    total = weighted_total(losses, crit.weight_dict)
    leaves = CR.leaves_of(out)
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
    return {k: losses[k].detach().clone() for k in losses.keys()}, total.detach(), grads


def _reference(crit, outputs, targets, idx, group_num):
    out, tg = CR.cast_case(outputs, targets, "cpu", torch.float64)
    n = LW.num_boxes(torch.cat([t["label_weight"] for t in targets]), group_num)
    want = LW.criterion_losses(out, tg, torch.from_numpy(idx), n, crit.focal_alpha, MAP_WH)
    total = sum(want[k] * float(crit.weight_dict[k]) for k in want if k in crit.weight_dict)
    leaves = CR.leaves_of(out)
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {n_: (torch.zeros_like(v) if g is None else g).detach() for (n_, v), g in zip(leaves.items(), grads)}
    return {k: float(v.detach()) for k, v in want.items()}, float(total.detach()), grads


# name -> (targets per image, queries, train mode, seed)
_LAYOUTS = {"mixed_train": ([0, 9, 1, 4], 110, True, 300), "eval_q50": ([5, 0, 10], 50, False, 301)}


def _case(name):
    sizes, Q, train, seed = _LAYOUTS[name]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    w = LW.draw_weights(seed + 1000, sum(sizes))
    assert (w == 0).any() and (w > 1).any()
    return outputs, LW.with_weights(targets, w), train


# ================================================================================================ 1. both formulations against float64
@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_both_cpu_formulations_equal_the_float64_reference_under_a_frozen_matching(name):
    outputs, targets, train = _case(name)
    fast = _criterion(True, train)
    vF, tF, gF = _evaluate(fast, outputs, targets, torch.float32)
    idx = fast.matcher.idx
    groups = fast.group_num if train else 1
    assert idx.shape == (3, 3, groups * sum(len(t["labels"]) for t in targets))
    st, ft = CR.stack_layers(outputs), CR.flat_targets(targets)
    _, margins = CR.census(st["pred_boxes"], st["pred_depth"], st["pred_3d_dim"], st["pred_angle"], torch.from_numpy(idx), ft["boxes_3d"],
                           ft["depth"], ft["size_3d"], ft["heading_bin"], ft["heading_res"])
    assert min(margins.values()) >= CR.MARGIN, margins
    slow = _criterion(False, train)
    slow.matcher.idx = idx
    vL, tL, gL = _evaluate(slow, outputs, targets, torch.float32)
    assert slow.matcher.calls == 3
    vR, tR, gR = _reference(fast, outputs, targets, idx, groups)
    bad = []
    for tag, v, t, g in (("fast", vF, tF, gF), ("layerwise", vL, tL, gL)):
        assert set(vR) <= set(v)
        for k, ref in vR.items():
            if k.startswith(("class_error", "cardinality_error")):
                assert abs(float(v[k]) - ref) <= 2.0 ** -22 * 100.0, (tag, k)
            else:
                e = _rel(v[k], ref)
                if e > VALUE:
                    bad.append((tag, k, e))
        if _rel(t, tR) > VALUE:
            bad.append((tag, "total", _rel(t, tR)))
        for n, ref in gR.items():
            rows = (lambda x: x.permute(0, 2, 3, 1)) if n == "depth_map_logits" else (lambda x: x)
            e = CR.row_error(rows(g[n]), rows(ref))
            print("MEASURED %s %-10s %-24s row error %.3e" % (name, tag, n, e))
            if e > (ROW_LOGITS if n.endswith("pred_logits") else ROW):
                bad.append((tag, n, e))
    assert not bad, bad
    # a weight of 0: the label's queries get no gradient in any head, classification included (don't care, not background)
    w = torch.cat([t["label_weight"] for t in targets])
    zero = torch.from_numpy(idx[2]).apply_(lambda t: float(w[t]) == 0.0).bool()
    assert zero.any() and not zero.all()
    for g in (gF, gL):
        for l in range(3):
            b, q = torch.from_numpy(idx[0, l]), torch.from_numpy(idx[1, l])
            for key in CR.PRED_KEYS:
                rows = g["l%d.%s" % (l, key)][b, q]
                assert (rows[zero[l]] == 0).all(), (l, key)
                assert (rows[~zero[l]].abs().sum(1) > 0).all(), (l, key)


# ================================================================================================ 2. all ones == key absent
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "layerwise"])
def test_weights_of_one_leave_every_loss_and_gradient_bit_for_bit(fast):
    outputs, targets, train = _case("mixed_train")
    plain = [{k: v for k, v in t.items() if k != "label_weight"} for t in targets]
    ones = [dict(t, label_weight=torch.ones(len(t["labels"]))) for t in plain]
    crit = _criterion(True, train)
    _evaluate(crit, outputs, plain, torch.float32)              # records the matching
    if not fast:
        idx = crit.matcher.idx
        crit = _criterion(False, train)
        crit.matcher.idx = idx
    v0, t0, g0 = _evaluate(crit, outputs, plain, torch.float32)
    v1, t1, g1 = _evaluate(crit, outputs, ones, torch.float32)
    assert set(v0) == set(v1) and len(v0) > 20
    for k in v0:
        assert torch.equal(v0[k], v1[k]), k
    assert torch.equal(t0, t1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    # and other weights do change them
    v2, _, _ = _evaluate(crit, outputs, targets, torch.float32)
    assert not torch.equal(v0["loss_ce"], v2["loss_ce"]) and not torch.equal(v0["loss_depth_map"], v2["loss_depth_map"])


# ================================================================================================ 3. the normaliser
def _padded(weights, mask):
    from monosowa_amd.synthetic import make_batch
    inputs, calibs, targets, info = make_batch(len(mask), "cpu", seed=5, resolution=(320, 96))
    targets["mask_2d"] = torch.from_numpy(np.asarray(mask))
    targets["label_weight"] = torch.from_numpy(np.asarray(weights, np.float32))
    return inputs, calibs, targets, info


def test_num_boxes_is_the_weight_sum_plain_accumulated_and_clamped():
    from monosowa_amd.helpers.trainer_helper import Trainer, stage_batch
    from monosowa_amd.synthetic import prepare_targets
    rng = np.random.default_rng(3)
    mask = np.zeros((2, 50), bool)
    mask[0, :4], mask[1, [0, 2, 5]] = True, True
    w = rng.uniform(0, 2, (2, 50)).astype(np.float32)
    w[0, 1] = 0.0
    raw = _padded(w, mask)
    want = LW.weight_sum(w[mask])
    tl = prepare_targets(raw[2], 2)
    assert tl.weight_sum == want and "label_weight" in tl.flat and [len(t["label_weight"]) for t in tl] == [4, 3]
    assert torch.equal(tl.flat["label_weight"], torch.from_numpy(w[mask]))
    crit = _criterion(True)
    assert crit._num_boxes(tl, 11, torch.device("cpu")) == max(want * 11, 1.0) == LW.num_boxes(w[mask], 11)
    # per-image dicts without a TargetList: the host tensors are added up
    assert crit._num_boxes([dict(t) for t in tl], 11, torch.device("cpu")) == LW.num_boxes(w[mask], 11)
    # key absent: the label count, as before
    plain = {k: v for k, v in raw[2].items() if k != "label_weight"}
    tp = prepare_targets(plain, 2)
    assert tp.weight_sum is None and "label_weight" not in tp.flat and crit._num_boxes(tp, 11, torch.device("cpu")) == 77.0
    # all weights 0: the clamp
    zero = prepare_targets(_padded(np.zeros((2, 50)), mask)[2], 2)
    assert zero.weight_sum == 0.0 and crit._num_boxes(zero, 11, torch.device("cpu")) == 1.0
    # staging keeps the host copy beside the (here: same) device copy; the cycle adds the batches' sums
    staged = stage_batch(raw, torch.device("cpu"))
    assert np.array_equal(staged[2]["label_weight"]._host_weight, w)
    w2 = rng.uniform(0, 2, (2, 50)).astype(np.float32)
    raw2 = _padded(w2, mask)
    n = Trainer._host_box_count(raw) + Trainer._host_box_count(raw2)
    assert Trainer._host_box_count(raw) == want and n == want + LW.weight_sum(w2[mask])
    assert Trainer._host_box_count((None, None, plain, None)) == 7 and isinstance(Trainer._host_box_count((None, None, plain, None)), int)
    fake = type("T", (), {"detr_loss": crit, "device": torch.device("cpu")})()
    assert Trainer._cycle_num_boxes(fake, n, 2) == max(n * 11 / 2, 1.0) == LW.num_boxes(np.concatenate([w[mask], w2[mask]]), 11, ranks=2)
    assert Trainer._cycle_num_boxes(fake, 0.0, 2) == 1.0


# ================================================================================================ 4. the dataset
@pytest.fixture()
def kitti_root(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "kitti_dataset.npz"), allow_pickle=False)
    for i, name in enumerate(g["file_names"]):
        path = tmp_path / str(name)
        os.makedirs(path.parent, exist_ok=True)
        path.write_bytes(g["file_%03d" % i].tobytes())
    return dict(json.loads(str(g["cfg_json"])), root_dir=str(tmp_path)), tmp_path


def _write(path, text):
    with open(str(path), "w") as f:
        f.write(text)
    return str(path)


def test_dataset_reads_weights_from_a_csv_by_line_whatever_the_augmentation(kitti_root):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    cfg, tmp = kitti_root
    base = KITTI_Dataset("train", cfg)
    ids = [int(i) for i in base.idx_list]
    n_lines = [len(base.get_label(i)) for i in ids]
    assert max(n_lines) >= 2
    first = ids[int(np.argmax(n_lines))]
    path = _write(tmp / "w.csv", "img_id,line,weight\n%d,0,0.25\n%06d,1,0\n%d,0,2.5\n" % (first, first, ids[-1] if ids[-1] != first else ids[0]))
    ds = KITTI_Dataset("train", dict(cfg, label_weights=path, label_weight_default=0.75))
    flips = 0
    for seed in (11, 12, 13):
        for item in range(len(ds)):
            np.random.seed(seed * 100 + item)
            _, _, t0, _ = base[item]
            np.random.seed(seed * 100 + item)
            _, _, t1, info = ds[item]
            flips += int(info["flip"])
            assert set(t1) == set(t0) | {"label_weight"}
            assert all(np.array_equal(t0[k], t1[k]) for k in t0)                   # every other key is what it was
            w = t1["label_weight"]
            assert w.dtype == np.float32 and w.shape == (50,)
            want = np.full(50, 0.75, np.float32)
            if ids[item] == first:
                want[0], want[1] = 0.25, 0.0
            elif ids[item] == (ids[-1] if ids[-1] != first else ids[0]):
                want[0] = 2.5
            assert np.array_equal(w, want), (ids[item], w[:4])
    assert 0 < flips < 3 * len(ds)                                                 # slot i is line i with and without the flip
    # the key is read for the training splits only; absent / None: today's keys
    assert "label_weight" not in KITTI_Dataset("val", dict(cfg, label_weights=path))[0][2]
    assert KITTI_Dataset("val", dict(cfg, label_weights=str(tmp / "missing.csv"))).label_weights is None
    np.random.seed(1)
    assert "label_weight" not in KITTI_Dataset("train", dict(cfg, label_weights=None))[0][2]
    # default of the default
    np.random.seed(1)
    assert KITTI_Dataset("train", dict(cfg, label_weights=_write(tmp / "e.csv", "img_id,line,weight\n")))[0][2]["label_weight"].tolist() == [1.0] * 50


def test_dataset_score_route_takes_the_sixteenth_column(kitti_root):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    cfg, tmp = kitti_root
    base = KITTI_Dataset("train", cfg)
    idx = int(base.idx_list[0])
    label = os.path.join(base.label_dir, "%06d.txt" % idx)
    lines = open(label).read().splitlines()
    assert all(len(l.split(" ")) == 15 for l in lines)
    scored = [l + " %s" % (0.5 + i) if i % 2 == 0 else l for i, l in enumerate(lines)]
    _write(label, "\n".join(scored) + "\n")
    ds = KITTI_Dataset("train", dict(cfg, label_weights="score", label_weight_default=0.125))
    np.random.seed(4)
    w = ds[0][2]["label_weight"]
    want = np.full(50, 0.125, np.float32)
    want[0:len(lines):2] = [0.5 + i for i in range(0, len(lines), 2)]
    assert np.array_equal(w, want)
    _write(label, "\n".join([lines[0] + " -0.5"] + lines[1:]) + "\n")
    with pytest.raises(ValueError, match=r"%06d\.txt line 1" % idx):
        ds[0]


def test_dataset_refuses_bad_weight_files_naming_them(kitti_root):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    cfg, tmp = kitti_root
    make = lambda text, name="bad.csv": dict(cfg, label_weights=_write(tmp / name, text))
    with pytest.raises(ValueError, match="missing.csv"):
        KITTI_Dataset("train", dict(cfg, label_weights=str(tmp / "missing.csv")))
    with pytest.raises(ValueError, match=r"bad\.csv.*header"):
        KITTI_Dataset("train", make("img_id,line,w\n1,0,1\n"))
    with pytest.raises(ValueError, match=r"bad\.csv line 3.*twice"):
        KITTI_Dataset("train", make("img_id,line,weight\n1,0,1\n000001,0,0.5\n"))
    with pytest.raises(ValueError, match=r"bad\.csv line 2"):
        KITTI_Dataset("train", make("img_id,line,weight\n1,0,-0.5\n"))
    for text in ("nan", "inf", "x"):
        with pytest.raises(ValueError, match=r"bad\.csv line 3"):
            KITTI_Dataset("train", make("img_id,line,weight\n1,0,1\n1,1,%s\n" % text))
    with pytest.raises(ValueError, match="label_weight_default"):
        KITTI_Dataset("train", dict(make("img_id,line,weight\n"), label_weight_default=-1))
    with pytest.raises(ValueError, match="label_weights"):
        KITTI_Dataset("train", dict(cfg, label_weights=3))


def test_loader_batches_carry_the_weights_to_the_criterion(kitti_root):
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.synthetic import prepare_targets
    cfg, tmp = kitti_root
    path = _write(tmp / "w.csv", "img_id,line,weight\n")
    cfg = dict(cfg, type="KITTI", train_split="train", test_split="val", batch_size=3, label_weights=path, label_weight_default=0.5)
    train_loader, test_loader = build_dataloader(cfg, workers=0)
    np.random.seed(0)
    raw = next(iter(train_loader))
    assert raw[2]["label_weight"].shape == (3, 50) and raw[2]["label_weight"].dtype == torch.float32
    tl = prepare_targets(stage_batch(raw, torch.device("cpu"))[2], 3)
    assert tl.weight_sum == 0.5 * int(raw[2]["mask_2d"].sum())
    assert "label_weight" not in next(iter(test_loader))[2]


# ================================================================================================ 5. the tool
def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import label_audit as tool
    finally:
        sys.path.pop(0)
    return tool


def _npz(path, img_id, line, depth_abs):
    from monosowa_amd.label_audit import COLUMNS, save
    values = np.zeros((len(line), 9))
    values[:, 4], values[:, 8] = depth_abs, 3
    values[:, 0] = np.asarray(depth_abs) * 10.0
    save(path, {"epoch": np.zeros(len(line), np.int64), "img_id": np.asarray(img_id), "line": np.asarray(line),
                "cls": np.ones(len(line), np.int64), "values": values, "columns": np.asarray(COLUMNS)})


def test_weights_subcommand_gives_the_huber_and_the_drop_weights(tmp_path, kitti_root):
    from monosowa_amd.kitti_dataset import KITTI_Dataset, read_label_weights
    tool = _tool()
    d = str(tmp_path / "label_audit")
    _npz(os.path.join(d, "epoch_000.npz"), [7, 7, 9, 4], [0, 1, 3, 2], [1.0, 8.0, 2.0, float("nan")])
    _npz(os.path.join(d, "epoch_001.npz"), [7, 7], [0, 1], [3.0, 2.0])
    out = str(tmp_path / "w.csv")
    tool.main(["weights", d, "--out", out, "--huber", "2"])
    table = list(csv.reader(open(out)))
    assert table[0] == ["img_id", "line", "weight"]
    got = read_label_weights(out)
    assert got == {(4, 2): 0.0, (7, 1): 2.0 / 5.0, (7, 0): 1.0, (9, 3): 1.0}            # means 5, 2, 2; NaN -> 0; value == X -> 1
    tool.main(["weights", d, "--out", out, "--drop-above", "2", "--last", "1"])
    assert read_label_weights(out) == {(7, 0): 0.0, (7, 1): 1.0}
    tool.main(["weights", d, "--out", out, "--drop-above", "30", "--by", "center"])
    assert read_label_weights(out) == {(4, 2): 0.0, (7, 1): 0.0, (7, 0): 1.0, (9, 3): 1.0}           # center = 10 x depth_abs
    assert np.array_equal(tool.label_weights([1.0, 4.0, np.nan, 0.0], huber=2.0), [1.0, 0.5, 0.0, 1.0])
    assert np.array_equal(tool.label_weights([1.0, 4.0, np.nan, 2.0], drop_above=2.0), [1.0, 0.0, 0.0, 1.0])
    for bad in (["--huber", "0"], ["--drop-above", "-1"], [], ["--huber", "1", "--drop-above", "1"]):
        with pytest.raises(SystemExit):
            tool.main(["weights", d, "--out", out] + bad)
    with pytest.raises(ValueError):
        tool.label_weights([1.0], huber=0.0)
    # the CSV goes through the dataset
    cfg, _ = kitti_root
    ds0 = KITTI_Dataset("train", cfg)
    first = int(ds0.idx_list[0])
    _npz(os.path.join(d, "epoch_002.npz"), [first, first], [0, 1], [9.0, 1.0])
    tool.main(["weights", d, "--out", out, "--huber", "3", "--last", "1"])
    ds = KITTI_Dataset("train", dict(cfg, label_weights=out))
    np.random.seed(2)
    w = ds[0][2]["label_weight"]
    assert w[0] == np.float32(3.0 / 9.0) and w[1] == 1.0 and (w[2:] == 1.0).all()
