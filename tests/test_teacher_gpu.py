"""``trainer.teacher`` on the GPU: ``mono_encode_targets_f64`` against the scalar restatement (tests/teacher_reference.py) bit for bit,
``Teacher.submit`` / ``collect`` against the Detector and ``encode_targets``, and Trainer steps with the key on and off."""
import contextlib
import copy
import ctypes
import logging
import os

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import teacher_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5


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


@pytest.fixture(scope="module")
def generated(golden_dir, tmp_path_factory):
    return R.cases(golden_dir, tmp_path_factory.mktemp("teacher_kitti"))


def _encode_settings(cfg, min_score=R.MIN_SCORE, weights="score"):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    from monosowa_amd.teacher import encode_settings
    return encode_settings(KITTI_Dataset.settings(cfg), min_score, weights)


# ================================================================================================ 1. the kernel
def _carve(B, n, shift):
    """Every output as a view into one poisoned byte buffer: 40 poisoned bytes in front of each, each start a multiple of 16 plus
    ``shift`` elements of its own dtype.  -> (buffer, dict of views, bool mask of the bytes that belong to an output)."""
    from monosowa_amd.teacher import OUTPUTS
    spec = [(k, dtype, (B, n) + shape) for k, (dtype, shape) in OUTPUTS.items()] + [("n_ignore", torch.int32, (B,))]
    cursor, places = 0, []
    for k, dtype, shape in spec:
        item = torch.empty((), dtype=dtype).element_size()
        start = (cursor + 40 + 15) // 16 * 16 + shift * item
        nbytes = int(np.prod(shape)) * item
        places.append((k, dtype, shape, start, nbytes))
        cursor = start + nbytes
    buf = torch.full((cursor + 64,), POISON, dtype=torch.uint8, device=_dev())
    inside = np.zeros(cursor + 64, dtype=bool)
    views = {}
    for k, dtype, shape, start, nbytes in places:
        views[k] = buf[start:start + nbytes].view(dtype).view(shape)
        inside[start:start + nbytes] = True
    return buf, views, inside


def _kernel(rows, count, records, es):
    """The launch at two placements of the outputs -> host copies of the first; asserts that no byte outside the outputs changed and
    that both placements hold the same bytes."""
    from monosowa_amd.teacher import encode_targets
    dev = _dev()
    r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(dev)
    rec = torch.from_numpy(np.ascontiguousarray(records, dtype=np.float64)).to(dev)
    got = []
    for shift in (0, 1):
        buf, views, inside = _carve(r.shape[0], es.max_objs, shift)
        assert len({v.data_ptr() % 16 for v in views.values()}) == (1 if shift == 0 else 3)
        out = encode_targets(r, c, rec, es, out=views)
        torch.cuda.synchronize()
        assert all(out[k].data_ptr() == views[k].data_ptr() for k in views)
        host = buf.cpu().numpy()
        assert (host[~inside] == POISON).all()
        got.append({k: v.cpu().numpy() for k, v in views.items()})
    for k in got[0]:
        assert got[0][k].tobytes() == got[1][k].tobytes(), k
    return got[0]


def _compare(got, want, where):
    """Bit for bit; ``heading_res`` within one float32 ulp of the angle's range where the device's atan2 differs -> such cells."""
    cells = 0
    for k in list(R.SHAPES) + ["n_ignore"]:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, g.shape)
        if k == "heading_res" and g.tobytes() != w.tobytes():
            cells += int((g.view(np.int32) != w.view(np.int32)).sum())
            assert np.abs(g.astype(np.float64) - w.astype(np.float64)).max() <= R.HEADING_RES_ULP, (where, k)
            continue
        assert g.tobytes() == w.tobytes(), (where, k)
    return cells


def test_kernel_equals_the_restatement_bit_for_bit(generated):
    cfg, st, case_list, _ = generated
    es = _encode_settings(cfg)
    cells = 0
    # B = 3, R = 8: the first eight rows of three cases; then every case at R = 12
    for chosen, R_ in ((case_list[:3], 8), (case_list, R.ROWS_PER_FRAME)):
        rows, records = np.stack([c["rows"][:R_] for c in chosen]), np.stack([c["record"] for c in chosen])
        count = np.full(len(chosen), R_, dtype=np.int32)
        want = R.restate(rows, count, records, st)
        cells += _compare(_kernel(rows, count, records, es), want, "generator R = %d" % R_)
        assert want["mask_2d"].any() and want["ignore_mask"].any()
    for fam in R.families(case_list, cfg):                      # B = 2, R = 100
        want = R.restate(fam["rows"], fam["count"], fam["records"], R.settings(fam["cfg"], fam["min_score"], fam["weights"]))
        got = _kernel(fam["rows"], fam["count"], fam["records"], _encode_settings(fam["cfg"], fam["min_score"], fam["weights"]))
        cells += _compare(got, want, fam["name"])
    print("heading_res cells where the device's atan2 moved the last place: %d" % cells)


def test_more_slots_than_lanes_is_refused(generated):
    from monosowa_amd.kitti_eval import load
    from monosowa_amd.teacher import OUTPUTS, empty_outputs, encode_targets
    cfg, _, case_list, _ = generated
    dev = _dev()
    es = _encode_settings(cfg)
    rows = torch.from_numpy(case_list[0]["rows"][None].copy()).to(dev)
    count = torch.tensor([12], dtype=torch.int32, device=dev)
    rec = torch.from_numpy(case_list[0]["record"][None].copy()).to(dev)
    cms = torch.from_numpy(es.cls_mean_size).to(dev)
    for n, want in ((64, 0), (65, -2)):
        out = empty_outputs(1, n, dev)
        names = list(OUTPUTS) + ["n_ignore"]
        pointers = (ctypes.c_void_p * len(names))(*[out[k].data_ptr() for k in names])
        code = load().mono_encode_targets_f64(rows.data_ptr(), count.data_ptr(), rec.data_ptr(), cms.data_ptr(), es.writelist_mask,
                                              es.depth_mode, int(es.clip_2d), es.min_score, es.weight_mode, es.weight, 1280, 384, 1, 12,
                                              3, n, pointers, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert code == want
    with pytest.raises(ValueError, match="encode_targets_host"):
        encode_targets(rows, count, rec, es._replace(max_objs=65))


# ================================================================================================ the shipped model
def _yaml():
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        return yaml.safe_load(f)


def _whole_config(dataset_cfg, tester=None, **trainer):
    cfg = _yaml()
    return {"dataset": dict(dataset_cfg, type="KITTI", device_aug=True, batch_size=2, unlabelled_split="train", train_split="train",
                            test_split="val"),
            "tester": dict({"type": "KITTI", "topk": 50, "threshold": 0.0}, **(tester or {})), "model": cfg["model"],
            "optimizer": cfg["optimizer"], "trainer": dict({"save_path": "outputs", "max_epoch": 2}, **trainer)}


def _model(seed=444, **over):
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    torch.manual_seed(seed)
    model, crit = build_model(dict(_yaml()["model"], device="cuda", **over))
    return to_mi355x_layout(model.to(_dev())), crit.to(_dev())


def _unlabelled_batch(whole, seed):
    from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
    loader = build_unlabelled_loader(whole["dataset"], workers=0)
    torch.manual_seed(seed)
    np.random.seed(seed)
    return loader, next(iter(loader))


@pytest.mark.parametrize("tester", [{}, {"nms_iou": 0.5, "flip_tta": True}], ids=["plain", "nms_iou+flip_tta"])
def test_submit_and_collect_equal_the_detector_and_the_encode(generated, tester):
    from monosowa_amd import Detector, Teacher
    from monosowa_amd.image_prep import prepare
    from monosowa_amd.teacher import encode_targets, student_records
    dataset_cfg = generated[0]
    dev = _dev()
    model, _ = _model()
    whole = _whole_config(dataset_cfg, tester, teacher={"min_score": 0.0, "source": "model"})
    loader, raw = _unlabelled_batch(whole, 5)
    canvas, calibs, targets, info = raw
    ds = loader.dataset
    frames = [np.array(Image.open(os.path.join(ds.image_dir, "%06d.png" % int(i)))) for i in info["img_id"]]
    with deterministic():
        det = Detector(whole, model=model.eval())
        scores = np.concatenate([r[:50, 13] for r in det.detect(frames, calibs.numpy())])      # the rows that find a slot
        det.close()
        assert len(scores) > 20
        whole["trainer"]["teacher"]["min_score"] = float(np.median(scores))
        teacher = Teacher(whole, model, dev)
        teacher.bind_source(None)
        teacher.refresh()
        teacher.submit(raw)
        images, calibs_dev, got, info_out = teacher.collect()
        assert teacher.collect() is None and info_out is info
        det = Detector(whole, model=teacher.module)
        rows = det.detect(frames, calibs.numpy())
        det.close()
    torch.cuda.synchronize()
    assert torch.equal(images, prepare(canvas, info["prep"], dev)) and torch.equal(calibs_dev.cpu(), calibs)
    width = max(max(len(r) for r in rows), 1)
    padded = np.zeros((2, width, 14))
    for b, r in enumerate(rows):
        padded[b, :len(r)] = r
    count = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
    records = torch.from_numpy(student_records(calibs, targets["img_size"], info["flip"], info["affine"], info["scale_depth"],
                                               info["canonical_scale"])).to(dev)
    want = encode_targets(torch.from_numpy(padded).to(dev), count, records, teacher.settings)
    torch.cuda.synchronize()
    assert set(got) == set(want) - {"n_ignore"} | {"img_size"}
    for k in got:
        assert torch.equal(got[k], want[k] if k != "img_size" else targets["img_size"].to(dev)), k
    n_targets, n_ignore = int(want["mask_2d"].sum()), int(want["n_ignore"].sum())
    print("targets %d, ignore boxes %d of %d rows" % (n_targets, n_ignore, int(count.sum())))
    assert n_targets > 0 and n_ignore > 0 and teacher.last_counts == (n_targets, n_ignore)
    assert np.array_equal(got["mask_2d"]._host_mask, got["mask_2d"].cpu().numpy())
    assert got["label_weight"]._host_weight.tobytes() == got["label_weight"].cpu().numpy().tobytes()
    assert got["ignore_mask"]._host_any is True
    teacher.close()


class _Loader:
    def __init__(self, seeds, batch_size=2):
        from monosowa_amd.synthetic import make_batch
        self.batch_size = batch_size
        self.batches = [make_batch(batch_size, "cpu", seed=s) for s in seeds]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


class _Rig:
    """A Trainer over a copy of the seeded model (dropout 0), with the forward seeded per call; ``teacher``: the keys of
    ``trainer.teacher`` or None."""

    def __init__(self, dataset_cfg, shared, seeds, teacher=None, **trainer_cfg):
        from monosowa_amd import Teacher, flash_attn, pointwise
        from monosowa_amd.helpers.optimizer_helper import build_optimizer
        from monosowa_amd.helpers.trainer_helper import Trainer
        model0, crit0 = shared
        self.model, self.crit = copy.deepcopy(model0), copy.deepcopy(crit0)
        self.k = 0

        def hook(module, args):
            torch.manual_seed(100 + self.k)
            pointwise._seed_counter[0] = flash_attn._seed_counter[0] = 0
            self.k += 1
        extra = {} if teacher is None else {"teacher": teacher}
        whole = _whole_config(dataset_cfg, **dict(trainer_cfg, **extra))
        self.opt = build_optimizer(whole["optimizer"], self.model)
        self.loader = _Loader(seeds)
        self.teacher = None
        if teacher is not None:
            from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
            self.teacher = Teacher(whole, self.model, _dev(), loader=build_unlabelled_loader(whole["dataset"], workers=0))
        self.model.register_forward_pre_hook(hook)             # behind the teacher's copy: its captured forward must not reseed
        self.trainer = Trainer(whole["trainer"], self.model, self.opt, self.loader, None, None, None, logging.getLogger("teacher"),
                               self.crit, "shipped", **({} if teacher is None else {"teacher": self.teacher}))
        self.trainer.log_interval = 10 ** 9
        self.model.train(), self.crit.train()

    def params(self):
        return [p.detach().clone() for p in self.model.parameters()]


@pytest.fixture(scope="module")
def shared():
    return _model(dropout=0.0)


def test_three_steps_with_the_key_on(generated, shared, monkeypatch):
    """Four cycles at batch 2 -- the first has no pseudo batch yet (the teacher runs one cycle ahead), the next three have one labelled
    and one pseudo micro-batch each.  ``torch.cuda.synchronize`` is called by nothing in a step except ``torch.cuda.graph`` itself when
    the engine captures its forward after a refresh: calls == captures in every step, and none of either in a step without a refresh."""
    import monosowa_amd.inference as inference
    rig = _Rig(generated[0], shared, [7, 8, 9, 10], teacher={"min_score": 0.0, "refresh": 2}, ema_decay=0.5)
    t, teacher = rig.trainer, rig.teacher
    assert teacher.config.source == "ema" and teacher.source is t.ema
    before = rig.params()
    syncs, captures = [0], [0]
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.__setitem__(0, syncs[0] + 1), real(*a, **k))[1])
    init = inference._Graph.__init__
    monkeypatch.setattr(inference._Graph, "__init__", lambda self, *a, **k: (captures.__setitem__(0, captures[0] + 1), init(self, *a, **k))[1])
    np.random.seed(3)
    torch.manual_seed(3)
    per_step, same, losses, pseudo = [], [], [], []
    for step, raw in enumerate(rig.loader):
        s0, c0 = syncs[0], captures[0]
        staged = t._teacher_turn()
        same.append(all(torch.equal(a, b) for a, b in zip(teacher.module.parameters(), t.ema.module.parameters())))
        total, _ = t.train_cycle([raw], staged)
        per_step.append((syncs[0] - s0, captures[0] - c0))
        losses.append(total)
        pseudo.append(len(staged))
    monkeypatch.undo()
    torch.cuda.synchronize()
    print("(synchronize calls, graph captures) per step: %s; pseudo micro-batches: %s; refreshes: %d" % (per_step, pseudo, teacher.refreshes))
    assert pseudo == [0, 1, 1, 1] and teacher.refreshes == 2
    assert all(s == c for s, c in per_step) and per_step[1] == (0, 0) and per_step[3] == (0, 0)
    assert same == [True, False, True, False]
    assert all(torch.isfinite(x).item() for x in losses)
    assert any(not torch.equal(a, b) for a, b in zip(before, rig.params()))
    assert all(torch.isfinite(p).all().item() for p in rig.model.parameters())
    teacher.close()


def test_an_epoch_with_the_key_on_logs_the_pseudo_counts(generated, shared, capsys):
    """``train_one_epoch`` itself with the teacher on: three loader batches are three cycles (the first without a pseudo batch), every
    one logs ``pseudo: targets n, ignored m`` with the counts of the cycle it ran, and the next cycle's batch is left in flight until
    ``close()`` drops it and ends the loader's iterator."""
    import re
    rig = _Rig(generated[0], shared, [7, 8, 9], teacher={"min_score": 0.0, "source": "model"})
    t, teacher = rig.trainer, rig.teacher
    t.log_interval = 1
    before = rig.params()
    seen, collect = [], teacher.collect

    def collecting():
        staged = collect()
        seen.append(teacher.last_counts)
        return staged
    teacher.collect = collecting
    np.random.seed(3)
    torch.manual_seed(3)
    t.train_one_epoch(0)
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    logged = [(int(n), int(m)) for n, m in re.findall(r"^pseudo: targets (\d+), ignored (\d+)$", out, flags=re.M)]
    print("logged (targets, ignored) per cycle: %s" % logged)
    assert logged == [(0, 0)] + seen and len(seen) == 2
    assert all(0 <= n <= 100 and 0 <= m <= 100 for n, m in seen)              # 2 images x 50 slots
    assert teacher.refreshes == 1 and teacher.in_flight() == 1 and teacher._iterator is not None
    assert any(not torch.equal(a, b) for a, b in zip(before, rig.params()))
    assert all(torch.isfinite(p).all().item() for p in rig.model.parameters())
    teacher.close()
    assert teacher.in_flight() == 0 and teacher._iterator is None and not teacher.engine.graphs and not teacher.engine.queue


def test_before_start_epoch_the_loop_is_the_plain_one(generated, shared):
    """``start_epoch: 1``: the parameters after epoch 0 are bit for bit those of a Trainer without the key."""
    got = []
    with deterministic():
        for teacher in (None, {"min_score": 0.0, "start_epoch": 1, "source": "model"}):
            rig = _Rig(generated[0], shared, [7, 8], teacher=teacher)
            rig.trainer.train_one_epoch(0)
            torch.cuda.synchronize()
            got.append(rig.params())
            if rig.teacher is not None:
                assert rig.teacher.refreshes == 0 and rig.teacher.in_flight() == 0 and not rig.teacher.engine.graphs
                rig.teacher.close()
    assert len(got[0]) == len(got[1]) and all(torch.equal(a, b) for a, b in zip(*got))
    assert any(not torch.equal(a, b) for a, b in zip(got[0], [p.detach() for p in shared[0].parameters()]))
