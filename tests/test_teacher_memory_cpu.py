"""``trainer.teacher_memory`` on the CPU: the configuration, ``merge_host`` against the scalar restatement (tests/memory_reference.py)
byte for byte over three passes with state carried, the two properties the rule promises, the state dict, the checkpoint keys, the
export tool and the refusal under more than one rank."""
import importlib.util
import logging
import os

import numpy as np
import pytest
import torch

import memory_reference as R
from test_detector_cpu import StubModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(value, min_score=0.5, threshold=0.2, nms_iou=None, max_objs=50):
    from monosowa_amd.teacher_memory import memory_config
    return memory_config(value, min_score, threshold, nms_iou, max_objs)


# ================================================================================================ configuration
def test_memory_keys_defaults():
    from monosowa_amd.teacher import TEACHER_KEYS, TeacherConfig, teacher_config
    assert _config(None) is None
    assert tuple(_config({})) == (0.5, 0.5, 0.2, 50)
    assert tuple(_config({}, nms_iou=0.3, threshold=0.1, max_objs=80)) == (0.5, 0.3, 0.1, 64)
    assert tuple(_config({}, nms_iou=0, max_objs=7)) == (0.5, 0.5, 0.2, 7)
    assert tuple(_config({"momentum": 0.9, "iou": 1, "drop_below": 0, "slots": 1})) == (0.9, 1.0, 0.0, 1)
    assert tuple(_config({"drop_below": 0.5, "slots": 64})) == (0.5, 0.5, 0.5, 64)      # drop_below = min_score is allowed
    # the sibling key is what it was: six fields, and no key of the memory is known inside it
    assert TEACHER_KEYS == ("refresh", "source", "per_step", "min_score", "weights", "start_epoch") and TeacherConfig._fields == TEACHER_KEYS
    assert tuple(teacher_config({"min_score": 0.2}, True, 0.2)) == (200, "ema", 1, 0.2, "score", 0)
    with pytest.raises(ValueError, match="trainer.teacher"):
        teacher_config({"min_score": 0.5, "momentum": 0.5}, True, 0.2)


@pytest.mark.parametrize("bad", [
    [], "on", True, 3, {"speed": 1}, {"momentum": 0}, {"momentum": 1}, {"momentum": 1.5}, {"momentum": -0.1}, {"momentum": True},
    {"momentum": "0.5"}, {"momentum": float("nan")}, {"momentum": None}, {"iou": 0}, {"iou": 1.01}, {"iou": True}, {"iou": "0.5"},
    {"iou": float("nan")}, {"drop_below": -0.01}, {"drop_below": 0.51}, {"drop_below": True}, {"drop_below": "0.2"},
    {"drop_below": float("nan")}, {"slots": 0}, {"slots": 65}, {"slots": 4.0}, {"slots": True}, {"slots": "4"}, {"slots": float("nan")}])
def test_malformed_memory_keys_are_refused(bad):
    with pytest.raises(ValueError, match="trainer.teacher_memory"):
        _config(bad)


def test_the_key_needs_the_teacher_and_one_rank(monkeypatch):
    from monosowa_amd.helpers.trainer_helper import Trainer
    with pytest.raises(ValueError, match="trainer.teacher_memory needs trainer.teacher"):
        _config({}, min_score=None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="trainer.teacher_memory"):
        Trainer({"save_path": "outputs", "max_epoch": 1, "teacher_memory": {}}, StubModel(), None, [], None, None, None,
                logging.getLogger("memory"), None, "tiny")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(ValueError, match="trainer.teacher_memory.*rank"):
        _config({})
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 1)
    assert _config({}) is not None


# ================================================================================================ the rule
def _memory(N, M, bank=None, count=None, **kw):
    from monosowa_amd import LabelMemory
    m = LabelMemory(list(range(N)), M, kw.get("momentum", R.MOMENTUM), kw.get("iou", R.IOU), kw.get("drop_below", R.DROP), "cpu")
    if bank is not None:
        m.bank.copy_(torch.from_numpy(bank))
        m.count.copy_(torch.from_numpy(count))
    return m


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def restated():
    return {gen.__name__: R.run(gen) for gen in (R.small_passes, R.wide_passes)}


@pytest.mark.parametrize("gen", [R.small_passes, R.wide_passes], ids=["B4 N6 M4 R8", "B1 M64 R130"])
def test_merge_host_equals_the_restatement_over_three_passes(gen, restated):
    bank, bank_count, passes = gen()
    memory = _memory(bank.shape[0], bank.shape[1], bank, bank_count)
    totals = np.zeros(6, dtype=np.int64)
    for p, ((rows, count, frame), want) in enumerate(zip(passes, restated[gen.__name__])):
        want_bank, want_bank_count, want_rows, want_count, want_stats, pairs = want
        assert R.margin_holds(pairs), "pass %d: a same-class pair lies within %g of the threshold" % (p, R.MARGIN)
        out_rows, out_count, stats = memory.merge_host(_t(rows), _t(count), _t(frame))
        assert out_rows.dtype == torch.float64 and out_count.dtype == torch.int32 and stats.dtype == torch.int32
        assert np.array_equal(R.bits(memory.bank.numpy()), R.bits(want_bank)), p
        assert np.array_equal(memory.count.numpy(), want_bank_count), p
        assert np.array_equal(R.bits(out_rows.numpy()), R.bits(want_rows)), p
        assert np.array_equal(out_count.numpy(), want_count) and np.array_equal(stats.numpy(), want_stats), p
        # matched + missed = entries before, entries before + created - dropped - evicted = entries after
        totals += want_stats.sum(0)
    print("%s: matched, created, missed, dropped, evicted, skipped = %s" % (gen.__name__, totals.tolist()))
    assert (totals[:5] > 0).all()
    if gen is R.small_passes:
        assert totals[5] == 3                                 # the NaN, +Inf and -Inf rows
        first = restated[gen.__name__][0]
        assert first[1][5] == 4 and first[1][3] == 4          # the hostile counts are rewritten
        assert (first[0][4] == 0).all() and (first[0][1] == 0).all()      # frames no call named yet


def test_generated_families_are_what_they_claim(restated):
    p1, p2, p3 = restated["small_passes"]
    s1, s2, s3 = p1[4], p2[4], p3[4]
    assert s1[0].tolist() == [0, 3, 0, 0, 0, 0]               # empty bank
    assert s1[1][4] == 2                                      # six survivors, M = 4: eviction
    assert s2[0][0] == 3 and s2[0][2] == 0                    # all matched
    assert s3[0][2] == p2[3][0] and s3[0][0] == 0             # all missed
    assert s3[0][3] >= 1                                      # decay below drop_below
    assert s2[1][5] == 3                                      # NaN, +Inf, -Inf
    assert s3[1].tolist()[:2] == [0, 0] and s3[1][5] == 0     # a negative count brings nothing
    # image 2: the zero-side box never matches (its copy becomes a second entry), the twins claim one entry each, the other class its own
    assert s2[2][0] == 3 and s2[2][1] == 1


def test_p1_first_pass_on_an_empty_bank_returns_the_rows(restated):
    rng = np.random.default_rng(5)
    M, R_ = 6, 9
    rows = np.zeros((2, R_, 14))
    for b, n in enumerate((6, 4)):
        scores = np.sort(rng.uniform(R.DROP, 1.0, n))[::-1]
        scores[-1] = R.DROP                                   # at drop_below: kept
        if b == 0:
            scores[2] = scores[1]                             # an exact tie keeps the row order
        for i in range(n):
            rows[b, i] = R._seen(rng, R._object(rng, i), scores[i])
    count, frame = np.array([6, 4], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    memory = _memory(3, M)
    out_rows, out_count, stats = memory.merge_host(_t(rows), _t(count), _t(frame))
    assert np.array_equal(R.bits(out_rows.numpy()), R.bits(rows[:, :M])) and out_count.tolist() == [6, 4]
    assert stats.tolist() == [[0, 6, 0, 0, 0, 0], [0, 4, 0, 0, 0, 0]]
    assert np.array_equal(R.bits(memory.bank.numpy()[[1, 0], :, :14]), R.bits(rows[:, :M]))
    assert (memory.bank.numpy()[2] == 0).all() and memory.count.tolist() == [4, 6, 0]
    # P3: the same rows again -- only `hits` grows
    before = memory.bank.numpy().copy()
    again, again_count, stats = memory.merge_host(_t(rows), _t(count), _t(frame))
    assert np.array_equal(R.bits(again.numpy()), R.bits(out_rows.numpy())) and again_count.tolist() == [6, 4]
    after = memory.bank.numpy()
    assert np.array_equal(R.bits(after[:, :, :14]), R.bits(before[:, :, :14])) and np.array_equal(after[:, :, 15], before[:, :, 15])
    assert stats.tolist() == [[6, 0, 0, 0, 0, 0], [4, 0, 0, 0, 0, 0]]
    assert after[1, :6, 14].tolist() == [2.0] * 6 and after[0, :4, 14].tolist() == [2.0] * 4 and after[0, 4:, 14].tolist() == [0.0, 0.0]
    # the restatement says the same of both
    bank, bank_count = np.zeros((3, M, 16)), np.zeros(3, dtype=np.int32)
    for _ in range(2):
        want = R.merge(rows, count, frame, bank, bank_count)
        assert np.array_equal(R.bits(want[0]), R.bits(rows[:, :M]))


def test_an_alternately_seen_row_stays_below_a_steadily_seen_one():
    rng = np.random.default_rng(6)
    steady, blinking = R._object(rng, 0), R._object(rng, 1)
    memory = _memory(1, 4, drop_below=0.0)
    for p in range(8):
        items = [R._seen(rng, steady, 0.8)] + ([R._seen(rng, blinking, 0.8)] if p % 2 == 0 else [])
        rows = R._pack([items], 2)
        out_rows, out_count, _ = memory.merge_host(_t(rows), torch.tensor([len(items)], dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
        assert out_count.item() == 2
        by_class = {float(r[0]): float(r[13]) for r in out_rows[0, :2].numpy()}       # object 0 is of class 0, object 1 of class 1
        s_steady, s_blinking = by_class[steady[0]], by_class[blinking[0]]
        assert s_steady == 0.8                                # s + w (s - s) = s
        assert s_blinking <= s_steady and (p == 0 or s_blinking < s_steady)
    assert memory.bank[0, :2, 14].tolist() == [8.0, 4.0] and memory.bank[0, :2, 15].tolist() == [0.0, 1.0]


def test_wrapper_refuses_what_it_cannot_merge():
    from monosowa_amd import LabelMemory
    memory = _memory(4, 3)
    rows, count, frames = torch.zeros((2, 5, 14), dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    memory.merge_host(rows, count, frames)
    with pytest.raises(ValueError, match="twice"):
        memory.merge_host(rows, count, torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="float64"):
        memory.merge_host(rows.float(), count, frames)
    with pytest.raises(ValueError, match="contiguous"):
        memory.merge_host(torch.zeros((2, 14, 5), dtype=torch.float64).transpose(1, 2), count, frames)
    with pytest.raises(ValueError, match="frames"):
        memory.merge_host(rows, count, frames.long())
    with pytest.raises(ValueError, match="count"):
        memory.merge_host(rows, count[:1], frames)
    with pytest.raises(ValueError, match="rows per image"):
        memory.merge_host(torch.zeros((2, 257, 14), dtype=torch.float64), count, frames)
    named = LabelMemory(["000007", "000003", "000011"], 2, 0.5, 0.5, 0.2, "cpu")
    assert named.positions(torch.tensor([11, 7])).tolist() == [2, 0] and named.positions([3]).dtype == torch.int32
    with pytest.raises(KeyError):
        named.positions([5])
    with pytest.raises(ValueError, match="twice"):
        named.positions([3, 3])
    with pytest.raises(ValueError, match="twice"):
        LabelMemory([1, 1], 2, 0.5, 0.5, 0.2, "cpu")
    for bad in (dict(slots=0), dict(slots=65), dict(momentum=0.0), dict(momentum=1.0), dict(iou=0.0), dict(iou=1.5)):
        with pytest.raises(ValueError):
            LabelMemory([1], **dict(dict(slots=2, momentum=0.5, iou=0.5, drop_below=0.2, device="cpu"), **bad))


# ================================================================================================ state, checkpoint, export
def _filled():
    bank, bank_count, passes = R.small_passes()
    memory = _memory(6, 4, bank, bank_count)
    for rows, count, frame in passes[:2]:
        memory.merge_host(_t(rows), _t(count), _t(frame))
    return memory


def test_state_dict_round_trip_and_mismatch(caplog):
    from monosowa_amd import LabelMemory
    memory = _filled()
    state = memory.state_dict()
    assert sorted(state) == ["bank", "count", "drop_below", "ids", "iou", "momentum", "slots"]
    assert state["bank"].shape == (6, 4, 16) and state["bank"].dtype == torch.float64 and state["count"].dtype == torch.int32
    assert state["bank"].data_ptr() != memory.bank.data_ptr()
    other = _memory(6, 4)
    with caplog.at_level(logging.WARNING):
        assert other.load_state_dict(state) is True
    assert not caplog.records
    assert np.array_equal(R.bits(other.bank.numpy()), R.bits(memory.bank.numpy())) and torch.equal(other.count, memory.count)
    for wrong in (LabelMemory([0, 1, 2, 3, 4, 6], 4, 0.5, 0.5, 0.2, "cpu"), _memory(6, 5)):
        wrong.bank.fill_(1.0)
        wrong.count.fill_(2)
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert wrong.load_state_dict(state) is False
        assert len(caplog.records) == 1 and "starts empty" in caplog.records[0].getMessage()
        assert not wrong.bank.any() and not wrong.count.any()
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert other.load_state_dict(None) is False           # a checkpoint without the key
    assert len(caplog.records) == 1 and not other.bank.any()


class _Teacher:
    threshold = 0.2

    def __init__(self, memory):
        self.memory = memory

    def bind_source(self, ema):
        pass


def test_checkpoint_keys_with_the_key_off_and_on(tmp_path, monkeypatch, caplog):
    from monosowa_amd.helpers.save_helper import load_checkpoint, save_checkpoint
    from monosowa_amd.helpers.trainer_helper import Trainer
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    log = logging.getLogger("memory")
    base = {"save_path": "outputs", "max_epoch": 1}
    plain = Trainer(base, StubModel(), None, [], None, None, None, log, None, "tiny")
    assert sorted(plain._checkpoint_state(0, 0)) == ["best_epoch", "best_result", "epoch", "model_state", "optimizer_state"]
    memory = _filled()
    on = Trainer(dict(base, teacher={"min_score": 0.5}, teacher_memory={}), StubModel(), None, [], None, None, None, log, None, "tiny",
                 teacher=_Teacher(memory))
    state = on._checkpoint_state(0, 0)
    assert sorted(state) == ["best_epoch", "best_result", "epoch", "model_state", "optimizer_state", "teacher_memory"]
    off = Trainer(dict(base, teacher={"min_score": 0.5}), StubModel(), None, [], None, None, None, log, None, "tiny", teacher=_Teacher(None))
    assert "teacher_memory" not in off._checkpoint_state(0, 0)
    save_checkpoint(state, str(tmp_path / "with"))
    save_checkpoint(plain._checkpoint_state(0, 0), str(tmp_path / "without"))
    fresh = _memory(6, 4)
    load_checkpoint(StubModel(), None, str(tmp_path / "with.pth"), "cpu", memory=fresh)
    assert np.array_equal(R.bits(fresh.bank.numpy()), R.bits(memory.bank.numpy())) and torch.equal(fresh.count, memory.count)
    with caplog.at_level(logging.WARNING):
        load_checkpoint(StubModel(), None, str(tmp_path / "without.pth"), "cpu", memory=fresh)
    assert sum("starts empty" in r.getMessage() for r in caplog.records) == 1 and not fresh.bank.any() and not fresh.count.any()


def _tool():
    spec = importlib.util.spec_from_file_location("teacher_memory_tool", os.path.join(ROOT, "tools", "teacher_memory.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_export_writes_the_detectors_bytes_and_min_hits_filters(tmp_path, capsys):
    import json
    from monosowa_amd.helpers.tester_helper import write_kitti_results
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    tool = _tool()
    memory = _filled()
    torch.save({"epoch": 1, "teacher_memory": memory.state_dict()}, str(tmp_path / "checkpoint.pth"))
    torch.save({"epoch": 1}, str(tmp_path / "plain.pth"))
    bank, count = memory.bank.numpy(), memory.count.numpy()
    assert (bank[:, :, 14] >= 2).any() and (bank[:, :, 14][bank[:, :, 14] > 0] < 2).any()
    names = KITTI_Dataset.settings({}).class_name
    for min_hits, below in ((0, None), (2, None), (0, 0.5)):
        out, want = tmp_path / ("out_%d_%s" % (min_hits, below)), tmp_path / ("want_%d_%s" % (min_hits, below))
        argv = ["export", "--checkpoint", str(tmp_path / "checkpoint.pth"), "--out", str(out), "--min-hits", str(min_hits)]
        tool.main(argv + ([] if below is None else ["--dontcare-below", str(below)]))
        rows = {f: bank[f, :count[f]][bank[f, :count[f], 14] >= min_hits][:, :14] for f in range(6)}
        write_kitti_results(rows, names, str(want), dontcare_below=below)
        assert sorted(os.listdir(out)) == sorted(os.listdir(want)) == ["%06d.txt" % f for f in range(6)]
        for name in os.listdir(want):
            assert (out / name).read_bytes() == (want / name).read_bytes(), name
        lines = sum(len((out / name).read_text().splitlines()) for name in os.listdir(out))
        assert lines == sum(len(r) for r in rows.values()) and (lines < count.sum()) == (min_hits == 2)
        if below is not None:
            assert any("DontCare" in (out / name).read_text() for name in os.listdir(out))
    capsys.readouterr()
    tool.main(["summary", "--checkpoint", str(tmp_path / "checkpoint.pth")])
    got = json.loads(capsys.readouterr().out)
    assert got["frames"] == 6 and got["entries"] == int(count.sum()) and len(got["score"]) == 5 and got["hits"][-1] >= 2
    with pytest.raises(KeyError, match="teacher_memory"):
        tool.main(["summary", "--checkpoint", str(tmp_path / "plain.pth")])


# ================================================================================================ the Teacher on the CPU device
def test_teacher_on_the_cpu_device_merges_between_fuse_and_encode(golden_dir, tmp_path_factory):
    """Key off / on, two passes over the generated frames: pass 1 trains on the targets of the key-off run (P1); in both passes the
    targets are the host encode of the restatement's merge of the engine's own rows (the stub model answers every call differently, so
    pass 2 is a look that differs: entries are matched, missed and created)."""
    import teacher_reference as T
    from monosowa_amd import Teacher
    from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
    from monosowa_amd.teacher import encode_targets_host, student_records
    dataset_cfg = T.cases(golden_dir, tmp_path_factory.mktemp("memory_kitti"))[0]
    got = {}
    for key in (None, {"drop_below": 0.0}):
        whole = {"dataset": dict(dataset_cfg, type="KITTI", device_aug=True, batch_size=2, unlabelled_split="train"),
                 "tester": {"type": "KITTI", "topk": 50, "threshold": 0.0, "nms_iou": 0.5}, "model": {},
                 "trainer": dict({"save_path": "outputs", "max_epoch": 1, "teacher": {"min_score": 0.3}},
                                 **({} if key is None else {"teacher_memory": key}))}
        teacher = Teacher(whole, StubModel(), "cpu", loader=build_unlabelled_loader(whole["dataset"], workers=0))
        teacher.bind_source(None)
        teacher.refresh()
        assert (teacher.memory is None) == (key is None) and teacher.last_memory is None
        np.random.seed(11)
        torch.manual_seed(11)
        n_batches = len(teacher.loader)
        bank = None if key is None else np.zeros(tuple(teacher.memory.bank.shape))
        bank_count = None if key is None else np.zeros(teacher.memory.count.shape[0], dtype=np.int32)
        seen = []
        for step in range(2 * n_batches):
            raw = teacher.next_raw()
            teacher.submit(raw)
            _, _, targets, info = teacher.collect()
            seen.append((info["img_id"].tolist(), {k: v.numpy().copy() for k, v in targets.items()}))
            if key is None:
                continue
            rows, count = teacher.last_rows
            frames = teacher.memory.positions(info["img_id"]).numpy()
            merged = R.merge(rows, count, frames, bank, bank_count, teacher.memory.momentum, teacher.memory.iou, 0.0)
            assert R.margin_holds(merged[3])
            records = student_records(raw[1], raw[2]["img_size"], info["flip"], info["affine"], info["scale_depth"], info["canonical_scale"])
            want = encode_targets_host(merged[0], merged[1], records, teacher.settings)
            for k in want:
                if k != "n_ignore":
                    assert targets[k].numpy().tobytes() == want[k].tobytes(), (step, k)
            assert teacher.last_memory == tuple(int(v) for v in merged[2].sum(0))
            assert step >= n_batches or teacher.last_memory == (0, int(count.sum()), 0, 0, 0, 0)
            total = merged[2].sum(0) if step == 0 else total + merged[2].sum(0)
        assert key is None or (total[1] > 0 and total[2] > 0)
        got[key is None] = seen[:n_batches]
        teacher.close()
    for (ids_off, off), (ids_on, on) in zip(got[True], got[False]):
        assert ids_off == ids_on
        for k in off:
            assert off[k].tobytes() == on[k].tobytes(), k
