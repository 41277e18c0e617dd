"""``model.ignore_depth_map`` and ``tester.dontcare_below`` on the CPU: the plain formulation of monodetr/losses.py against the restatement
of tests/ignore_depth_reference.py in float64 (masks exact, values and gradients to 1e-12), the key, both formulations of the criterion
on CPU tensors with the key on and off, and the written result files.

Float32 CPU criterion against the float64 reference: VALUE / ROW of tests/test_ignore_regions_cpu.py (the same float32 formulation)."""
import os

import numpy as np
import pytest
import torch
import yaml

import criterion_reference as CR
import ignore_depth_reference as ID
import label_weights_reference as LW
from test_ignore_regions_cpu import MAP_WH, ROOT, ROW, VALUE, _case, _criterion, _evaluate, kitti_root      # noqa: F401  (fixture)

REL64 = 1e-12
_CASE_IDS = [(H, W, M) for H, W in ID.SIZES for M in ID.MS]


def _rel(x, ref):
    return abs(float(x) - float(ref)) / max(abs(float(ref)), 1e-300)


# ================================================================================================ 1. the plain formulation
def _plain(case, dtype, weighted, logits=None, channels_last=False):
    from monosowa_amd.monodetr.losses import DDNLoss
    lg = (case["logits"] if logits is None else logits).to(dtype)
    if channels_last:
        lg = lg.contiguous(memory_format=torch.channels_last)
    lg.requires_grad_(True)
    mod = DDNLoss()
    loss = mod.forward_padded(lg, case["boxes"].to(dtype), case["depth"].to(dtype), case["valid"],
                              box_weight=case["weight"].to(dtype) if weighted else None, ignore=(case["ign_boxes"], case["ign_valid"]))
    (grad,) = torch.autograd.grad(loss * 1.75, [lg])
    return loss.detach(), grad, mod.ign_count


def _reference(case, dtype, weighted, logits=None):
    lg = (case["logits"] if logits is None else logits).to(dtype).requires_grad_(True)
    loss, maps = ID.depth_map_loss(lg, case["boxes"].to(dtype), case["depth"].to(dtype), case["valid"],
                                   case["weight"].to(dtype) if weighted else None, case["ign_boxes"], case["ign_valid"])
    (grad,) = torch.autograd.grad(loss * 1.75, [lg])
    return loss.detach(), grad, maps


@pytest.mark.parametrize("H,W", ID.SIZES)
def test_the_cases_of_a_map_size_hold_every_property_together(H, W):
    ID.assert_family(H, W)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
@pytest.mark.parametrize("H,W,M", _CASE_IDS)
def test_plain_formulation_equals_the_float64_reference(H, W, M, weighted):
    from monosowa_amd.monodetr.losses import rasterize_ignore
    case = ID.case(H, W, M)
    for dtype in (torch.float64, torch.float32):                              # the rule: exact masks, whatever the logits' dtype
        got = rasterize_ignore(case["ign_boxes"], case["ign_valid"], case["fg"], H, W)
        assert got.dtype == torch.bool and torch.equal(got, case["ignored"])
    vP, gP, count = _plain(case, torch.float64, weighted)
    vR, gR, (_, fg, _, ign) = _reference(case, torch.float64, weighted)
    assert torch.equal(ign, case["ignored"]) and int(count.sum()) == int(ign.sum()) > 0
    assert _rel(vP, vR) <= REL64, (float(vP), float(vR))
    rows = lambda x: x.permute(0, 2, 3, 1)
    err = (rows(gP) - rows(gR)).norm(dim=-1) / rows(gR).norm(dim=-1).clamp_min(1e-300)
    assert float(err.max()) <= REL64
    g = rows(gP)
    assert (g[ign] == 0).all() and not torch.signbit(g[ign]).any()
    keep = ~ign & ~(fg & (case["wmap"] == 0) if weighted else torch.zeros_like(ign))
    assert (g[keep].abs().sum(-1) > 0).all()
    # the loss with the regions differs from the loss without them by exactly the ignored pixels' terms
    from monosowa_amd.monodetr.losses import DDNLoss
    full = DDNLoss().forward_padded(case["logits"].double(), case["boxes"].double(), case["depth"].double(), case["valid"],
                                    box_weight=case["weight"].double() if weighted else None)
    assert float(full) > float(vP)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
def test_non_finite_logits_under_ignored_pixels_reach_nothing_and_elsewhere_everything(weighted):
    case = ID.case(5, 7, 3)
    ign = case["ignored"]
    where = torch.nonzero(ign)
    assert len(where) >= 3
    clean_v, clean_g, _ = _plain(case, torch.float64, weighted)
    poisoned = case["logits"].clone()
    for (b, y, x), bad in zip(where[:3].tolist(), (float("nan"), float("inf"), -float("inf"))):
        poisoned[b, 5, y, x] = bad
    v, g, _ = _plain(case, torch.float64, weighted, logits=poisoned)
    assert torch.equal(v, clean_v) and torch.equal(g, clean_g)                # not one bit of the result moves
    rows = g.permute(0, 2, 3, 1)
    assert (rows[ign] == 0).all() and not torch.signbit(rows[ign]).any() and torch.isfinite(g).all()
    vR, gR, _ = _reference(case, torch.float64, weighted, logits=poisoned)
    assert torch.isfinite(vR) and torch.isfinite(gR).all()
    # the same values in a pixel that is not ignored: the loss is not finite, as it is today
    b, y, x = [p for p in torch.nonzero(~ign).tolist() if not case["fg"][p[0], p[1], p[2]]][0]         # (a background pixel: factor 1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        spoiled = case["logits"].clone()
        spoiled[b, 5, y, x] = bad
        v, _, _ = _plain(case, torch.float64, weighted, logits=spoiled)
        assert not torch.isfinite(v), bad


# ================================================================================================ 2. the key
def test_key_is_off_by_default_absent_from_the_shipped_yaml_and_a_bool():
    assert _criterion(True).ignore_depth_map is False and _criterion(False).ignore_depth_map is False
    assert _criterion(True, ignore_depth_map=None).ignore_depth_map is False
    assert _criterion(True, ignore_depth_map=False).ignore_depth_map is False
    assert _criterion(True, ignore_depth_map=True).ignore_depth_map is True
    assert "ignore_depth_map" not in yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["model"]
    assert "dontcare_below" not in yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["tester"]
    for bad in (1, 0, "true", "false", 0.5, [True], np.bool_(True)):
        with pytest.raises(ValueError, match="ignore_depth_map"):
            _criterion(True, ignore_depth_map=bad)
    assert _criterion(True).ignore_depth_report() is None


# ================================================================================================ 3. the criterion on CPU tensors
def _depth_map_reference(outputs, targets, ignore, dtype=torch.float64):
    """loss_depth_map of the final layer's map by the restatement: the padded inputs of label_weights_reference, the ignore boxes
    times (w, h, w, h) in float32"""
    tg = targets if "label_weight" in targets[0] else [dict(t, label_weight=torch.ones(len(t["labels"]))) for t in targets]
    pb, pd, pv, pw = LW.padded_depth_map_inputs(tg, MAP_WH, dtype)
    w, h = MAP_WH
    px = torch.from_numpy(np.asarray(ignore[0], np.float32) * np.array([w, h, w, h], np.float32))
    lg = outputs["pred_depth_map_logits"].to(dtype).requires_grad_(True)
    loss, (_, fg, wmap, ign) = ID.depth_map_loss(lg, pb, pd, pv, pw, px, torch.from_numpy(ignore[1]))
    (grad,) = torch.autograd.grad(loss, [lg])
    return float(loss.detach()), grad, ign


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "layerwise"])
def test_criterion_on_cpu_tensors_with_the_key_on_and_off(fast, weighted):
    outputs, targets, train, ignore = _case("mixed_train", weighted)
    rec = _criterion(True, train)
    _evaluate(rec, outputs, targets, ignore)                                  # records the matching
    idx = rec.matcher.idx

    def build(**cfg):
        c = _criterion(fast, train, **cfg)
        c.matcher.idx = idx
        return c
    off = build()
    v0, t0, g0 = _evaluate(off, outputs, targets, ignore)
    assert off.ignore_depth_report() is None and off.ignore_report() is not None and len(off.ignore_report()) == 2
    for value in (None, False):                                               # the key off: today's criterion, bit for bit
        c = build(ignore_depth_map=value)
        v, t, g = _evaluate(c, outputs, targets, ignore)
        assert c.ignore_depth_report() is None
        assert list(v) == list(v0) and all(torch.equal(v[k], v0[k]) for k in v0) and torch.equal(t, t0)
        assert all(torch.equal(g[n], g0[n]) for n in g0)
    on = build(ignore_depth_map=True)
    want, grad_want, ign = _depth_map_reference(outputs, targets, ignore)
    n_ign = int(ign.sum())
    assert n_ign > 100 and not ign[1].any()                                   # image 1 has no ignore box
    for dtype, v_tol, r_tol in ((torch.float64, REL64, REL64), (torch.float32, VALUE, ROW)):
        v1, t1, g1 = _evaluate(on, outputs, targets, ignore, dtype=dtype)
        assert on.ignore_depth_report() == (n_ign, 4 * 24 * 80)
        assert len(on.ignore_report()) == 2
        e = _rel(v1["loss_depth_map"], want)
        print("MEASURED %s loss_depth_map e %.3e" % (dtype, e))
        assert e <= v_tol, (dtype, e)
        rows = lambda x: x.permute(0, 2, 3, 1)
        scale = float(on.weight_dict["loss_depth_map"])
        e = CR.row_error(rows(g1["depth_map_logits"]), rows(grad_want * scale))
        print("MEASURED %s depth_map_logits row error %.3e" % (dtype, e))
        assert e <= r_tol, (dtype, e)
        gi = rows(g1["depth_map_logits"])[ign]
        assert (gi == 0).all() and not torch.signbit(gi).any()
        if dtype == torch.float32:                                            # every other key: the key-off criterion's, bit for bit
            assert list(v1) == list(v0)
            for k in v0:
                assert torch.equal(v1[k], v0[k]) != (k == "loss_depth_map"), k
            assert all(torch.equal(g1[n], g0[n]) != (n == "depth_map_logits") for n in g0)
            assert float(v1["loss_depth_map"]) < float(v0["loss_depth_map"])
    # a batch without regions: nothing is ignored, the report is None, and the result is the key-off criterion's
    v2, t2, g2 = _evaluate(on, outputs, targets)
    assert on.ignore_depth_report() is None
    v3, t3, g3 = _evaluate(off, outputs, targets)
    assert all(torch.equal(v2[k], v3[k]) for k in v3) and all(torch.equal(g2[n], g3[n]) for n in g3)


def test_eval_mode_criterion_ignores_the_pixels_too():
    outputs, targets, train, ignore = _case("eval_q50", False)
    assert train is False
    on = _criterion(True, False, ignore_depth_map=True)
    v, _, _ = _evaluate(on, outputs, targets, ignore, dtype=torch.float64)
    want, _, ign = _depth_map_reference(outputs, targets, ignore)
    assert _rel(v["loss_depth_map"], want) <= REL64 and on.ignore_depth_report() == (int(ign.sum()), 3 * 24 * 80)


# ================================================================================================ 4. tester.dontcare_below
_ROWS = {7: [[0, -1.25, 100.126, 150.0, 200.5, 250.25, 1.5, 1.6, 3.9, -2.0, 1.7, 20.0, 0.3, 0.91],
             [1, 0.5, 300.0, 160.0, 330.0, 240.0, 1.7, 0.6, 0.8, 4.0, 1.6, 15.0, -0.2, 0.35],          # below X
             [2, 0.1, 500.0, 170.0, 540.0, 230.0, 1.7, 0.6, 1.8, 6.0, 1.6, 25.0, 1.2, 0.5],            # at X: stays
             [0, 0.2, 600.0, 170.0, 700.0, 230.0, 1.5, 1.6, 3.9, 8.0, 1.6, 30.0, 1.0, float("nan")],   # NaN: as it is today
             [0, 0.3, 10.0, 20.0, 30.0, 40.0, 1.5, 1.6, 3.9, 9.0, 1.6, 35.0, 1.1, 0.2]],               # below X, at the threshold
         12: []}
_NAMES = ["Pedestrian", "Car", "Cyclist"]


def _written(tmp_path, name, **kw):
    from monosowa_amd.helpers.tester_helper import write_kitti_results
    out = tmp_path / name
    write_kitti_results(_ROWS, _NAMES, str(out), **kw)
    return {p.name: p.read_bytes() for p in sorted(out.iterdir())}


def test_doubtful_rows_are_written_as_dontcare_lines_in_place(tmp_path):
    today = _written(tmp_path, "plain")
    assert _written(tmp_path, "off", dontcare_below=None) == today and set(today) == {"000007.txt", "000012.txt"}
    assert today["000012.txt"] == b""
    lines = today["000007.txt"].decode().splitlines()
    assert lines[1] == "Car 0.0 0 0.50 300.00 160.00 330.00 240.00 1.70 0.60 0.80 4.00 1.60 15.00 -0.20 0.35"
    got = _written(tmp_path, "band", dontcare_below=0.5)["000007.txt"].decode().splitlines()
    assert len(got) == 5 and [got[i] for i in (0, 2, 3)] == [lines[i] for i in (0, 2, 3)]
    assert got[1] == "DontCare -1 -1 -10.00 300.00 160.00 330.00 240.00 -1.00 -1.00 -1.00 -1000.00 -1000.00 -1000.00 -10.00 0.35"
    assert got[4] == "DontCare -1 -1 -10.00 10.00 20.00 30.00 40.00 -1.00 -1.00 -1.00 -1000.00 -1000.00 -1000.00 -10.00 0.20"
    assert all(len(l.split(" ")) == 16 for l in got) and "nan" in got[3]
    assert _written(tmp_path, "one", dontcare_below=1.0)["000007.txt"].decode().splitlines()[3] == lines[3]


def test_dontcare_below_is_checked_when_detector_and_tester_are_built():
    from monosowa_amd.helpers.tester_helper import check_dontcare_below
    assert check_dontcare_below(None, 0.2) is None and check_dontcare_below(0.5, 0.2) == 0.5 and check_dontcare_below(1, 0.2) == 1.0
    for bad in (True, False, "0.5", 0.2, 0.1, 1.5, float("nan"), [0.5]):
        with pytest.raises(ValueError, match="dontcare_below"):
            check_dontcare_below(bad, 0.2)
    import inspect
    from monosowa_amd import detector
    from monosowa_amd.helpers import tester_helper
    assert "check_dontcare_below" in inspect.getsource(detector.Detector.__init__)
    assert "check_dontcare_below" in inspect.getsource(tester_helper.Tester.__init__)

    class _Loader:
        class dataset:
            max_objs, class_name = 50, _NAMES
    make = lambda **cfg: tester_helper.Tester(dict({"threshold": 0.2}, **cfg), torch.nn.Linear(1, 1), _Loader, None, train_cfg={"save_path": "x"})
    assert make().dontcare_below is None and make(dontcare_below=0.4).dontcare_below == 0.4
    with pytest.raises(ValueError, match="dontcare_below"):
        make(dontcare_below=0.2)


def dontcare_files(kitti_root, tmp_path):
    """Detections of image 000003 written twice: with the doubtful band as DontCare lines, and the same file without those lines.
    -> (directory with, directory without, lines of the first, label directory)"""
    from monosowa_amd.helpers.tester_helper import write_kitti_results
    cfg, root, files = kitti_root
    # its two plain Cars as they stand, one more Car in the doubtful band
    rows = {3: [[1, -1.83, 583.34, 182.67, 668.75, 217.29, 1.47, 1.71, 4.22, 1.30, 1.89, 30.72, -1.79, 0.9],
                [1, -1.5, 200.0, 180.0, 260.0, 230.0, 1.5, 1.6, 3.9, -9.0, 1.7, 25.0, -1.6, 0.3],
                [1, -0.52, 900.0, 174.0, 1100.0, 260.0, 1.66, 1.51, 3.84, 6.00, 1.78, 12.00, -0.32, 0.6]]}
    with_dc, without = tmp_path / "with_dc", tmp_path / "without"
    write_kitti_results(rows, _NAMES, str(with_dc), dontcare_below=0.5)
    text = (with_dc / "000003.txt").read_text().splitlines()
    assert [l.split(" ")[0] for l in text] == ["Car", "DontCare", "Car"]
    os.makedirs(without)
    (without / "000003.txt").write_text("\n".join(l for l in text if not l.startswith("DontCare")) + "\n")
    return with_dc, without, text, root / "training" / "label_2"


def test_written_dontcare_lines_come_back_as_ignore_boxes(kitti_root, tmp_path):
    """(that the evaluation's report does not move under these lines needs the overlap kernels: tests/test_ignore_depth_map_gpu.py)"""
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    from test_ignore_regions_cpu import _expected_boxes
    cfg, root, files = kitti_root
    with_dc, _, text, label_dir = dontcare_files(kitti_root, tmp_path)
    base = KITTI_Dataset("train", dict(cfg, random_flip=0.0, random_crop=0.0))
    item = [i.strip() for i in base.idx_list].index("000003")
    (label_dir / "000003.txt").write_text((with_dc / "000003.txt").read_text())          # the written file as the next round's labels
    ds = KITTI_Dataset("train", dict(cfg, ignore_regions=True, random_flip=0.0, random_crop=0.0))
    np.random.seed(0)
    _, _, t, info = ds[item]
    take = [i for i, l in enumerate(text) if l.startswith("DontCare") or not t["mask_2d"][i]]          # (a Car that is no target, too)
    want, want_mask = _expected_boxes(text, take, info)
    assert 1 in take and np.array_equal(t["ignore_mask"], want_mask) and np.array_equal(t["ignore_boxes"], want)
    band = _expected_boxes(text, [1], info)[0][0]
    assert (t["ignore_boxes"][t["ignore_mask"]] == band).all(1).any() and int(t["mask_2d"].sum()) >= 1
    # dataset.label_weights: score reads the same 16 columns
    ds = KITTI_Dataset("train", dict(cfg, ignore_regions=True, label_weights="score", random_flip=0.0, random_crop=0.0))
    np.random.seed(0)
    _, _, t, _ = ds[item]
    assert sorted(t["label_weight"][t["mask_2d"].astype(bool)].tolist()) == [float(np.float32(0.6)), float(np.float32(0.9))]
