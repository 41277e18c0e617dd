"""``trainer.teacher`` on the CPU: the scalar restatement of the target encode (tests/teacher_reference.py) against the dataset class,
``encode_targets_host`` against the restatement bit for bit, ``UnlabelledKITTI``'s draws, the configuration errors and the engine's
``after=`` hook."""
import copy
import logging

import numpy as np
import pytest
import torch

import teacher_reference as R
from test_detector_cpu import StubModel, _stub_batch


@pytest.fixture(scope="module")
def generated(golden_dir, tmp_path_factory):
    cfg, st, case_list, stats = R.cases(golden_dir, tmp_path_factory.mktemp("teacher_kitti"))
    return cfg, st, case_list, stats


def _encode_settings(cfg, min_score=R.MIN_SCORE, weights="score"):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    from monosowa_amd.teacher import encode_settings
    return encode_settings(KITTI_Dataset.settings(cfg), min_score, weights)


def test_generator_delivers_targets_ignore_boxes_flips_and_crops(generated):
    _, _, case_list, stats = generated
    print(stats)
    assert stats["rows"] == 288 and len(case_list) == 24
    assert stats["discarded"] <= 0.10 * stats["draws"]
    assert stats["targets"] >= 0.30 * stats["rows"] and stats["ignore"] >= 0.30 * stats["rows"]
    assert 0 < stats["flips"] < 24 and 0 < stats["crops"] < 24


def test_restatement_equals_the_dataset_class_on_exactly_written_labels(generated):
    """``KITTI_Dataset.__getitem__`` on the exact-precision label files under the same seeds: which slot holds what and every
    integer key equal, every float key within 4 x the class's own spread between BLAS and exactly summed matrix products -- and that
    spread, measured again here, is the recorded one."""
    cfg, st, case_list, _ = generated
    plain = R.class_targets(cfg, case_list)
    exact = R.class_targets(cfg, case_list, exact_products=True)
    spread = {k: max(float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for a, b in zip(plain, exact))
              for k in R.FLOAT_KEYS}
    print("spread of the class:", spread)
    worst = dict.fromkeys(R.FLOAT_KEYS, 0.0)
    for c, want in zip(case_list, plain):
        got = R.restate(c["rows"][None], [R.ROWS_PER_FRAME], c["record"][None], st)
        assert set(R.SHAPES) == set(want) - {"img_size"}
        for k in R.EXACT_KEYS:
            assert got[k][0].dtype == np.asarray(want[k]).dtype and np.array_equal(got[k][0], want[k]), (c["seed"], c["item"], k)
        assert int(got["n_ignore"][0]) == int(np.count_nonzero(want["ignore_mask"]))
        for k in R.FLOAT_KEYS:
            assert got[k][0].dtype == want[k].dtype and got[k][0].shape == want[k].shape
            worst[k] = max(worst[k], float(np.abs(got[k][0].astype(np.float64) - want[k].astype(np.float64)).max()))
    print("restatement against the class:", worst)
    for k in R.FLOAT_KEYS:
        # the recorded spread is the class's on these inputs under the BLAS it was recorded with; a BLAS build that sums in another
        # order can move it without any change to the project: then re-record SPREAD (python tests/teacher_reference.py)
        assert spread[k] <= R.SPREAD[k], "%s: the class's spread is %r here, %r recorded: another BLAS? re-record SPREAD" % (k, spread[k], R.SPREAD[k])
        assert worst[k] <= R.ALLOWED[k], (k, worst[k], R.ALLOWED[k])


def _assert_bitwise(got, want, where):
    cells = 0
    for k in list(R.SHAPES) + ["n_ignore"]:
        g, w = np.asarray(got[k]), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, g.shape)
        if k == "heading_res" and g.tobytes() != w.tobytes():
            differ = g.view(np.int32) != w.view(np.int32)
            cells += int(differ.sum())
            assert np.abs(g.astype(np.float64) - w.astype(np.float64)).max() <= R.HEADING_RES_ULP, (where, k)
            continue
        assert g.tobytes() == w.tobytes(), (where, k)
    return cells


def test_host_encode_equals_the_restatement_bit_for_bit(generated):
    from monosowa_amd.teacher import encode_targets_host
    cfg, st, case_list, _ = generated
    cells = 0
    es = _encode_settings(cfg)
    rows, records = np.stack([c["rows"] for c in case_list]), np.stack([c["record"] for c in case_list])
    count = np.full(len(case_list), R.ROWS_PER_FRAME, dtype=np.int32)
    cells += _assert_bitwise(encode_targets_host(rows, count, records, es), R.restate(rows, count, records, st), "generator")
    seen = {"targets": 0, "ignore": 0}
    for fam in R.families(case_list, cfg):
        want = R.restate(fam["rows"], fam["count"], fam["records"], R.settings(fam["cfg"], fam["min_score"], fam["weights"]))
        got = encode_targets_host(fam["rows"], fam["count"], fam["records"], _encode_settings(fam["cfg"], fam["min_score"], fam["weights"]))
        cells += _assert_bitwise(got, want, fam["name"])
        n = np.minimum(fam["count"], 50)
        if fam["name"] == "count 0":
            assert not want["mask_2d"].any() and not want["ignore_mask"].any() and (want["label_weight"] == 1).all()
        if fam["name"] == "50 rows, all ignore boxes":
            assert not want["mask_2d"].any() and want["n_ignore"].sum() > 80
        if fam["name"] == "50 rows, all targets":
            assert want["mask_2d"].all() and not want["ignore_mask"].any()
        if fam["name"] == "count 70 > max_objs":
            assert want["mask_2d"].shape == (2, 50) and (want["mask_2d"].sum(1) + want["n_ignore"] <= n).all()
        seen["targets"] += int(want["mask_2d"].sum())
        seen["ignore"] += int(want["n_ignore"].sum())
    print("heading_res cells that differ in their last place: %d; families: %s" % (cells, seen))
    assert cells == 0                                   # both sides call numpy's float32 arctan2
    assert seen["targets"] > 100 and seen["ignore"] > 100


def test_unlabelled_dataset_consumes_the_training_samples_draws(generated):
    from monosowa_amd.kitti_dataset import KITTI_Dataset, UnlabelledKITTI
    cfg, _, _, _ = generated
    cfg = dict(cfg, device_aug=True, aug_pd=True)
    train, unlabelled = KITTI_Dataset("train", cfg), UnlabelledKITTI("train", cfg)
    unlabelled.get_label = None                         # a label file opened would fail here
    assert len(unlabelled) == len(train)
    flips = 0
    for seed in (1, 2, 3):
        for item in range(len(train)):
            np.random.seed(100 * seed + item)
            raw_t, P2_t, targets_t, info_t = train[item]
            after_t = np.random.get_state()
            np.random.seed(100 * seed + item)
            raw_u, P2_u, targets_u, info_u = unlabelled[item]
            after_u = np.random.get_state()
            assert after_t[0] == after_u[0] and np.array_equal(after_t[1], after_u[1]) and after_t[2:] == after_u[2:]
            assert raw_u.dtype == np.uint8 and np.array_equal(raw_t, raw_u) and np.array_equal(P2_t, P2_u)
            assert set(targets_u) == {"img_size"} and np.array_equal(targets_u["img_size"], targets_t["img_size"])
            assert set(info_u) == set(info_t)
            for k in ("flip", "affine", "affine_inv", "scale_depth", "prep", "canonical_scale", "img_id", "img_size", "height_crop"):
                assert np.array_equal(np.asarray(info_t[k]), np.asarray(info_u[k])), (seed, item, k)
            flips += int(info_u["flip"])
    assert 0 < flips < 18
    for bad in (dict(cfg, device_aug=False), {k: v for k, v in cfg.items() if k != "device_aug"}, dict(cfg, device_aug=1)):
        with pytest.raises(ValueError, match="device_aug"):
            UnlabelledKITTI("train", bad)
    with pytest.raises(ValueError, match="unlabelled_split"):
        UnlabelledKITTI("no_such_split", cfg)
    from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
    loader = build_unlabelled_loader(dict(cfg, type="KITTI", unlabelled_split="train", batch_size=2), workers=0)
    canvas, calibs, targets, info = next(iter(loader))
    assert canvas.dtype == torch.uint8 and canvas.shape[0] == 2 and calibs.shape == (2, 3, 4) and targets["img_size"].shape == (2, 2)
    assert info["prep"].shape[0] == 2 and info["affine"].shape == (2, 2, 3) and info["flip"].shape == (2,)
    with pytest.raises(ValueError, match="device_aug"):
        build_unlabelled_loader(dict(cfg, type="KITTI", unlabelled_split="train", batch_size=2, device_aug=False), workers=0)


GOOD = {"min_score": 0.5}


@pytest.mark.parametrize("bad", [
    [], "on", True, {"min_score": 0.5, "speed": 1}, {}, {"min_score": "0.5"}, {"min_score": True}, {"min_score": 1.5}, {"min_score": 0.1},
    {"min_score": float("nan")}, dict(GOOD, refresh=0), dict(GOOD, refresh=2.0), dict(GOOD, refresh=True), dict(GOOD, per_step=0),
    dict(GOOD, per_step="1"), dict(GOOD, start_epoch=-1), dict(GOOD, start_epoch=0.5), dict(GOOD, source="teacher"), dict(GOOD, source=None),
    dict(GOOD, weights="scores"), dict(GOOD, weights=-1.0), dict(GOOD, weights=float("inf")), dict(GOOD, weights=True)])
def test_malformed_teacher_keys_are_refused(bad):
    from monosowa_amd.teacher import teacher_config
    with pytest.raises(ValueError, match="trainer.teacher"):
        teacher_config(bad, True, 0.2)


def test_teacher_keys_defaults_and_source():
    from monosowa_amd.teacher import teacher_config
    assert teacher_config(None, True, 0.2) is None
    c = teacher_config({"min_score": 0.2}, True, 0.2)
    assert tuple(c) == (200, "ema", 1, 0.2, "score", 0)
    assert teacher_config({"min_score": 1}, False, 0.2).source == "model"
    c = teacher_config({"min_score": 0.6, "refresh": 3, "per_step": 2, "weights": 0, "start_epoch": 4, "source": "model"}, True, 0.2)
    assert tuple(c) == (3, "model", 2, 0.6, 0, 4)
    with pytest.raises(ValueError, match="ema_decay"):
        teacher_config({"min_score": 0.5, "source": "ema"}, False, 0.2)


def _whole_config(dataset_cfg, **trainer):
    return {"dataset": dict(dataset_cfg, type="KITTI", device_aug=True, batch_size=2, unlabelled_split="train"),
            "tester": {"type": "KITTI", "topk": 50, "threshold": 0.2}, "model": {},
            "trainer": dict({"save_path": "outputs", "max_epoch": 1}, **trainer)}


def test_teacher_and_trainer_refuse_what_the_issue_names(generated, monkeypatch):
    from monosowa_amd import Teacher
    from monosowa_amd.helpers.trainer_helper import Trainer
    dataset_cfg = generated[0]
    log = logging.getLogger("teacher")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good = _whole_config(dataset_cfg, teacher={"min_score": 0.5})
    teacher = Teacher(good, StubModel(), "cpu")
    assert teacher.loader is None and teacher.config.source == "model" and teacher.module is not teacher.live
    assert not teacher.module.training

    def build(cfg, **kw):
        return Trainer(cfg["trainer"], StubModel(), None, [], None, None, None, log, None, "tiny", **kw)
    assert build(good, teacher=teacher).teacher is teacher
    with pytest.raises(ValueError, match="teacher="):
        build(good)                                                                    # the key without a Teacher
    with pytest.raises(ValueError, match="trainer.teacher"):
        build(_whole_config(dataset_cfg), teacher=teacher)                            # a Teacher without the key
    with pytest.raises(ValueError, match="trainer.teacher"):
        build(_whole_config(dataset_cfg, teacher={"min_score": 0.5, "refresh": 0}), teacher=teacher)
    with pytest.raises(ValueError, match="label_audit"):
        build(_whole_config(dataset_cfg, teacher={"min_score": 0.5}, label_audit=True), teacher=teacher)
    with pytest.raises(ValueError, match="label_audit"):
        Teacher(_whole_config(dataset_cfg, teacher={"min_score": 0.5}, label_audit=True), StubModel(), "cpu")
    with pytest.raises(ValueError, match="ema_decay"):
        build(_whole_config(dataset_cfg, teacher={"min_score": 0.5, "source": "ema"}), teacher=teacher)
    with pytest.raises(ValueError, match="ema_decay"):
        Teacher(_whole_config(dataset_cfg, teacher={"min_score": 0.5, "source": "ema"}), StubModel(), "cpu")
    with pytest.raises(ValueError, match="min_score"):
        Teacher(_whole_config(dataset_cfg, teacher={"min_score": 0.1}), StubModel(), "cpu")      # below tester.threshold
    with pytest.raises(ValueError, match="absent"):
        Teacher(_whole_config(dataset_cfg), StubModel(), "cpu")
    aug = copy.deepcopy(good)
    aug["dataset"]["aug_calib"] = True
    with pytest.raises(ValueError, match="aug_calib"):
        Teacher(aug, StubModel(), "cpu")
    # a class the detector names, ignored by the class and outside the writelist: the device encode would drop what the class keeps
    ignored = copy.deepcopy(good)
    ignored["dataset"].update(writelist=["Car"], ignore_classes=["DontCare", "Pedestrian"])
    with pytest.raises(ValueError, match="ignore_classes"):
        Teacher(ignored, StubModel(), "cpu")
    ignored["dataset"].update(writelist=["Car", "Pedestrian"])                        # in the writelist it is no ignore class
    assert Teacher(ignored, StubModel(), "cpu").settings.writelist_mask == 0b011
    ignored["dataset"].update(writelist=["Car"], ignore_classes=["DontCare", "Van", "Tram"])
    assert Teacher(ignored, StubModel(), "cpu").settings.writelist_mask == 0b010
    many = copy.deepcopy(good)
    many["tester"].update(topk=200, nms_iou=0.5, flip_tta=True)
    with pytest.raises(ValueError, match="candidates"):
        Teacher(many, StubModel(), "cpu")


def test_without_the_key_the_trainer_builds_nothing(monkeypatch):
    """No Teacher, no unlabelled loader, no engine: the constructors are made to fail, and the Trainer still builds."""
    import monosowa_amd.helpers.dataloader_helper as dataloader_helper
    import monosowa_amd.inference as inference
    import monosowa_amd.teacher as teacher
    from monosowa_amd.helpers.trainer_helper import Trainer

    def refuse(*a, **k):
        raise AssertionError("built with trainer.teacher absent")
    monkeypatch.setattr(teacher.Teacher, "__init__", refuse)
    monkeypatch.setattr(teacher, "teacher_config", refuse)
    monkeypatch.setattr(dataloader_helper, "build_unlabelled_loader", refuse)
    monkeypatch.setattr(inference.InferenceEngine, "__init__", refuse)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for cfg in ({}, {"teacher": None}):
        t = Trainer(dict({"save_path": "outputs", "max_epoch": 1}, **cfg), StubModel(), None, [], None, None, None,
                    logging.getLogger("teacher"), None, "tiny")
        assert t.teacher is None and t.teacher_cfg is None


def test_engine_after_hook_on_the_cpu_device():
    """Called once per batch with the fused rows; its dict comes back as ``Completed.extra``; without it ``Completed`` is what it was."""
    from monosowa_amd.inference import InferenceEngine
    cms = np.zeros((3, 3))
    geom = torch.tensor([[1242.0, 375.0, 1.0, 1.0, 600.0, 180.0, 720.0, 720.0, 0.06, 0.0]], dtype=torch.float64)
    for fuse in (None, (0.05, False, "mean")):
        plain = InferenceEngine(StubModel(), "cpu", topk=50, decode=(cms, 0.3), fuse=fuse)
        hooked = InferenceEngine(StubModel(), "cpu", topk=50, decode=(cms, 0.3), fuse=fuse)
        calls = []

        def after(rows, count, slot):
            calls.append((rows.clone(), count.clone(), slot))
            return {"total": count.sum().reshape(1), "note": "kept as it is"}
        for n, B in enumerate((3, 2)):
            g = geom.repeat(B, 1)
            want = (plain.submit(*_stub_batch(n, B), geom=g, tag=n) + plain.drain())[0]
            got = (hooked.submit(*_stub_batch(n, B), geom=g, tag=n, after=after) + hooked.drain())[0]
            assert len(calls) == n + 1 and calls[-1][2] is None
            assert want.extra is None and want.dets is None
            assert got.rows.tobytes() == want.rows.tobytes() and got.count.tobytes() == want.count.tobytes()
            assert (got.support is None) == (fuse is None) and (fuse is None or got.support.tobytes() == want.support.tobytes())
            assert calls[-1][0].numpy().tobytes() == want.rows.tobytes() and calls[-1][1].numpy().tobytes() == want.count.tobytes()
            assert isinstance(got.extra["total"], np.ndarray) and int(got.extra["total"][0]) == int(want.count.sum())
            assert got.extra["note"] == "kept as it is"
        with pytest.raises(ValueError, match="geom"):
            hooked.submit(*_stub_batch(4, 2), tag=4, after=after)
            hooked.drain()
    done = (InferenceEngine(StubModel(), "cpu", topk=50).submit(*_stub_batch(0, 2), tag=0))[0]
    assert done.extra is None and done.rows is None and done.dets.shape == (2, 50, 37)


def test_teacher_submit_and_collect_on_the_cpu_device(generated, monkeypatch):
    """The same sequence on a CPU device (the engine runs inside ``submit``, the host function encodes): the staged batch is what
    ``stage_batch`` would return, its targets are ``encode_targets_host`` of the engine's rows, ``prepare_targets`` accepts them."""
    from monosowa_amd import Teacher
    from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
    from monosowa_amd.image_prep import prepare
    from monosowa_amd.synthetic import prepare_targets
    from monosowa_amd.teacher import encode_targets_host, student_records
    whole = _whole_config(generated[0], teacher={"min_score": 0.3})
    whole["tester"].update(threshold=0.0, nms_iou=0.5)
    teacher = Teacher(whole, StubModel(), "cpu", loader=build_unlabelled_loader(whole["dataset"], workers=0))
    teacher.bind_source(None)
    assert teacher.collect() is None
    teacher.refresh()
    np.random.seed(11)
    torch.manual_seed(11)
    for _ in range(4):                                   # 3 batches per pass: the loader is cycled
        raw = teacher.next_raw()
        teacher.submit(raw)
        assert teacher.in_flight() == 1
        images, calibs, targets, info = teacher.collect()
        assert teacher.in_flight() == 0 and info is raw[3]
        assert torch.equal(images, prepare(raw[0], info["prep"], "cpu")) and torch.equal(calibs, raw[1])
        rows, count = teacher.last_rows
        records = student_records(raw[1], raw[2]["img_size"], info["flip"], info["affine"], info["scale_depth"], info["canonical_scale"])
        want = encode_targets_host(rows, count, records, teacher.settings)
        assert set(targets) == set(want) - {"n_ignore"} | {"img_size"}
        for k in want:
            if k != "n_ignore":
                assert targets[k].numpy().tobytes() == want[k].tobytes(), k
        assert teacher.last_counts == (int(want["mask_2d"].sum()), int(want["n_ignore"].sum())) and teacher.last_counts[0] > 0
        assert np.array_equal(targets["mask_2d"]._host_mask, want["mask_2d"])
        assert targets["label_weight"]._host_weight.tobytes() == want["label_weight"].tobytes()
        tl = prepare_targets(targets, 2)
        assert sum(len(t["labels"]) for t in tl) == teacher.last_counts[0] and tl.weight_sum > 0
        assert (tl.ignore is not None) == (teacher.last_counts[1] > 0)
    assert teacher.refreshes == 1
    teacher.close()
