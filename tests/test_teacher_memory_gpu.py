"""``trainer.teacher_memory`` on the GPU: ``mono_memory_merge_f64`` against the scalar restatement (tests/memory_reference.py) byte for
byte over three passes, nothing written outside its outputs, its return codes, and the Teacher / Trainer with the key on."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import memory_reference as R
import test_teacher_gpu as G

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _memory(bank, bank_count):
    from monosowa_amd import LabelMemory
    m = LabelMemory(list(range(bank.shape[0])), bank.shape[1], R.MOMENTUM, R.IOU, R.DROP, _dev())
    m.bank.copy_(torch.from_numpy(bank))
    m.count.copy_(torch.from_numpy(bank_count))
    return m


# ================================================================================================ 1. the kernel
@pytest.mark.parametrize("gen", [R.small_passes, R.wide_passes], ids=["B4 N6 M4 R8", "B1 M64 R130"])
def test_kernel_equals_the_restatement_over_three_passes(gen):
    want_all = R.run(gen)
    bank, bank_count, passes = gen()
    memory = _memory(bank, bank_count)
    for p, ((rows, count, frame), want) in enumerate(zip(passes, want_all)):
        want_bank, want_bank_count, want_rows, want_count, want_stats, pairs = want
        assert R.margin_holds(pairs), "pass %d: a same-class pair lies within %g of the threshold" % (p, R.MARGIN)
        out_rows, out_count, stats = memory.merge(_t(rows), _t(count), _t(frame))
        torch.cuda.synchronize()
        assert np.array_equal(stats.cpu().numpy(), want_stats), (p, stats.cpu().numpy().tolist(), want_stats.tolist())
        assert np.array_equal(out_count.cpu().numpy(), want_count) and np.array_equal(memory.count.cpu().numpy(), want_bank_count), p
        assert np.array_equal(R.bits(out_rows.cpu().numpy()), R.bits(want_rows)), p
        assert np.array_equal(R.bits(memory.bank.cpu().numpy()), R.bits(want_bank)), p


def _carve(spec, shift_bytes):
    """Every array of ``spec`` (name, dtype, shape) as a view into one buffer of sentinel bytes, 40 of them in front of each, each
    start a multiple of 16 plus ``shift_bytes`` -> (buffer, views, bool mask of the bytes that belong to an array)."""
    cursor, places = 0, []
    for name, dtype, shape in spec:
        item = torch.empty((), dtype=dtype).element_size()
        start = (cursor + 40 + 15) // 16 * 16 + shift_bytes
        nbytes = int(np.prod(shape)) * item
        places.append((name, dtype, shape, start, nbytes))
        cursor = start + nbytes
    buf = torch.full((cursor + 64,), SENTINEL, dtype=torch.uint8, device=_dev())
    inside, views = np.zeros(cursor + 64, dtype=bool), {}
    for name, dtype, shape, start, nbytes in places:
        views[name] = buf[start:start + nbytes].view(dtype).view(shape)
        inside[start:start + nbytes] = True
    return buf, views, inside


def test_nothing_outside_the_outputs_is_written():
    """The outputs inside sentinel bytes at two placements; frames -1 and N give zeros and touch no bank; the blocks of frames the
    call does not name keep every byte."""
    from monosowa_amd.kitti_eval import load
    bank0, bank_count0, passes = R.small_passes()
    rows, count, _ = passes[0]
    N, M, B, R_ = 6, 4, 4, 8
    frame = np.array([2, -1, N, 3], dtype=np.int32)
    bank0[[0, 1, 4]] = 3.5                                     # frames the call does not name: rubbish that must stay
    bank_count0[[0, 1, 4]] = (2, -7, 99)
    want_bank, want_bank_count = bank0.copy(), bank_count0.copy()
    want_rows, want_count, want_stats, _ = R.merge(rows, count, frame, want_bank, want_bank_count)
    assert not want_rows[1].any() and not want_rows[2].any() and want_count.tolist()[1:3] == [0, 0] and not want_stats[1:3].any()
    assert want_count[0] > 0 and want_count[3] > 0
    assert np.array_equal(want_bank[[0, 1, 4, 5]], bank0[[0, 1, 4, 5]]) and want_bank_count[[0, 1, 4, 5]].tolist() == [2, -7, 99, -1]
    d_rows, d_count, d_frame = _t(rows), _t(count), _t(frame)
    spec = [("bank", torch.float64, (N, M, 16)), ("bank_count", torch.int32, (N,)), ("out_rows", torch.float64, (B, M, 14)),
            ("out_count", torch.int32, (B,)), ("stats", torch.int32, (B, 6))]
    for shift in (0, 8):
        buf, v, inside = _carve(spec, shift)
        assert all(t.data_ptr() % 16 == shift for t in v.values())
        v["bank"].copy_(torch.from_numpy(bank0))
        v["bank_count"].copy_(torch.from_numpy(bank_count0))
        code = load().mono_memory_merge_f64(d_rows.data_ptr(), d_count.data_ptr(), d_frame.data_ptr(), v["bank"].data_ptr(),
                                            v["bank_count"].data_ptr(), R.MOMENTUM, R.IOU, R.DROP, v["out_rows"].data_ptr(),
                                            v["out_count"].data_ptr(), v["stats"].data_ptr(), B, R_, N, M,
                                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert code == 0
        assert (buf.cpu().numpy()[~inside] == SENTINEL).all()
        assert np.array_equal(R.bits(v["bank"].cpu().numpy()), R.bits(want_bank)), shift
        assert np.array_equal(v["bank_count"].cpu().numpy(), want_bank_count), shift
        assert np.array_equal(R.bits(v["out_rows"].cpu().numpy()), R.bits(want_rows)), shift
        assert np.array_equal(v["out_count"].cpu().numpy(), want_count) and np.array_equal(v["stats"].cpu().numpy(), want_stats), shift


def test_return_codes_and_the_wrapper():
    from monosowa_amd import LabelMemory
    from monosowa_amd.kitti_eval import load
    dev = _dev()
    B, R_, N, M = 2, 5, 3, 4
    rows = torch.zeros((B, R_, 14), dtype=torch.float64, device=dev)
    count, frame = torch.zeros(B, dtype=torch.int32, device=dev), torch.tensor([0, 2], dtype=torch.int32, device=dev)
    bank, bank_count = torch.zeros((N, 64, 16), dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    out_rows = torch.zeros((B, 64, 14), dtype=torch.float64, device=dev)
    out_count, stats = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros((B, 6), dtype=torch.int32, device=dev)
    big_rows = torch.zeros((B, 256, 14), dtype=torch.float64, device=dev)
    pointers = [t.data_ptr() for t in (rows, count, frame, bank, bank_count)], [t.data_ptr() for t in (out_rows, out_count, stats)]

    def call(first=None, last=None, momentum=0.5, iou=0.5, B=B, R_=R_, N=N, M=M):
        first, last = first or pointers[0], last or pointers[1]
        code = load().mono_memory_merge_f64(*first, momentum, iou, 0.2, *last, B, R_, N, M, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return code
    assert call() == 0
    assert call(M=64) == 0 and call(M=1) == 0 and call(B=0) == 0 and call(N=0) == 0 and call(iou=1.0) == 0
    assert call(first=[big_rows.data_ptr()] + pointers[0][1:], R_=256) == 0
    for k in range(5):
        assert call(first=[None if j == k else p for j, p in enumerate(pointers[0])]) == -1
    for k in range(3):
        assert call(last=[None if j == k else p for j, p in enumerate(pointers[1])]) == -1
    for bad in (dict(M=0), dict(M=65), dict(R_=0), dict(R_=257), dict(B=-1), dict(N=-1), dict(iou=0.0), dict(iou=1.5),
                dict(iou=float("nan")), dict(momentum=0.0), dict(momentum=1.0), dict(momentum=float("nan"))):
        assert call(**bad) == -2, bad
    memory = LabelMemory(list(range(N)), M, 0.5, 0.5, 0.2, dev)
    memory.merge(rows, count, frame)
    with pytest.raises(ValueError, match="twice"):
        memory.merge(rows, count, torch.tensor([1, 1], dtype=torch.int32))         # host frames are checked; positions() checks its own
    with pytest.raises(ValueError, match="float64"):
        memory.merge(rows.float(), count, frame)
    with pytest.raises(ValueError, match="contiguous"):
        memory.merge(torch.zeros((B, 14, R_), dtype=torch.float64, device=dev).transpose(1, 2), count, frame)
    with pytest.raises(ValueError, match="frames"):
        memory.merge(rows, count, frame.long())
    with pytest.raises(ValueError, match="CUDA"):
        memory.merge(rows.cpu(), count.cpu(), frame.cpu())
    with pytest.raises(ValueError, match="out_rows"):
        memory.merge(rows, count, frame, out=(out_rows, out_count, stats))          # 64 slots, the memory has 4
    torch.cuda.synchronize()


# ================================================================================================ 2. the Teacher
@pytest.fixture(scope="module")
def generated(golden_dir, tmp_path_factory):
    import teacher_reference as T
    return T.cases(golden_dir, tmp_path_factory.mktemp("memory_kitti"))


def _positive_sizes(model):
    """The size head's last layer set to a Car's (h, w, l) plus a hundredth of its random weights: the generated configuration decodes
    sizes without mean shapes, so an untrained head gives sizes around zero, half of them negative -- and a rectangle with a side that
    is not > 0 matches nothing, its own copy included.  Every row of this model has sides > 0, the condition under which the rule
    promises P3."""
    seen = set()
    with torch.no_grad():
        for mlp in model.dim_embed_3d:
            last = mlp.layers[-1]
            if id(last) not in seen:
                seen.add(id(last))
                last.weight.mul_(0.01)
                last.bias.copy_(torch.tensor([1.5, 1.6, 3.9], device=last.bias.device))
    return model


def _collect_all(teacher, raws):
    out = []
    for raw in raws:
        teacher.submit(raw)
        _, _, targets, info = teacher.collect()
        out.append((targets, teacher.last_rows, teacher.last_memory))
    torch.cuda.synchronize()
    return out


def _same_targets(a, b, where):
    assert set(a) == set(b)
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), (where, k)


def test_teacher_end_to_end_over_three_passes(generated):
    """``nms_iou`` on, ``fuse: 'seed'``, two unlabelled batches.  Pass 1 equals the key-off Teacher (P1), pass 2 with unchanged weights
    equals pass 1 (P3), pass 3 after a refresh from another model equals ``encode_targets`` of the restatement's merge of the engine's
    own rows."""
    from monosowa_amd import Teacher
    from monosowa_amd.helpers.dataloader_helper import build_unlabelled_loader
    from monosowa_amd.teacher import encode_settings, encode_targets, student_records
    dev = _dev()
    model = _positive_sizes(G._model()[0])
    other = _positive_sizes(G._model(seed=445)[0])
    tester = {"nms_iou": 0.5, "fuse": "seed"}
    whole = G._whole_config(generated[0], tester, teacher={"min_score": 0.0, "source": "model"})
    loader = build_unlabelled_loader(whole["dataset"], workers=0)
    torch.manual_seed(5)
    np.random.seed(5)
    it = iter(loader)
    raws = [next(it), next(it)]
    assert len({int(i) for raw in raws for i in raw[3]["img_id"]}) == 4
    with G.deterministic():
        off = Teacher(whole, model, dev)
        off.bind_source(None)
        off.refresh()
        scores = np.concatenate([rows[b, :count[b], 13] for _, (rows, count), _ in _collect_all(off, raws) for b in range(2)])
        min_score = float(np.median(scores))                   # half of the rows targets, half ignore boxes
        off.settings = encode_settings(off.dataset, min_score, "score")
        want1 = _collect_all(off, raws)
        off.close()
        whole["trainer"]["teacher"]["min_score"] = min_score
        whole["trainer"]["teacher_memory"] = {"drop_below": 0.0}
        on = Teacher(whole, model, dev, loader=loader)
        on.bind_source(None)
        on.refresh()
        assert on.memory.slots == 50 and on.memory.iou == 0.5 and on.memory.bank.shape == (len(loader.dataset.idx_list), 50, 16)
        got1 = _collect_all(on, raws)
        got2 = _collect_all(on, raws)
        state = on.memory.state_dict()
        on.live = other                                         # the next refresh copies a differently seeded model
        on.refresh()
        got3 = _collect_all(on, raws)
    n_rows = 0
    for b in range(2):
        assert want1[b][2] is None
        rows, count = got1[b][1]
        kept = np.arange(rows.shape[1])[None, :] < count[:, None]
        assert (rows[kept][:, 7] > 0).all() and (rows[kept][:, 8] > 0).all(), "P3 is promised for rows with sides > 0"
        _same_targets(got1[b][0], want1[b][0], "pass 1, batch %d" % b)
        _same_targets(got2[b][0], got1[b][0], "pass 2, batch %d" % b)
        assert got2[b][1][0].tobytes() == got1[b][1][0].tobytes()
        n = int(got1[b][1][1].sum())
        n_rows += n
        assert got1[b][2] == (0, n, 0, 0, 0, 0) and got2[b][2] == (n, 0, 0, 0, 0, 0)
    assert int(got1[0][0]["mask_2d"].sum()) > 0 and n_rows > 20
    bank, bank_count = state["bank"].numpy().copy(), state["count"].numpy().copy()
    totals = np.zeros(6, dtype=np.int64)
    for b, raw in enumerate(raws):
        rows, count = got3[b][1]
        assert rows.tobytes() != got1[b][1][0].tobytes()
        frames = on.memory.positions(raw[3]["img_id"]).numpy()
        merged = R.merge(rows, count, frames, bank, bank_count, on.memory.momentum, on.memory.iou, on.memory.drop_below)
        assert R.margin_holds(merged[3]), "a pair of the models' own rows lies within %g of the threshold" % R.MARGIN
        info = raw[3]
        records = torch.from_numpy(student_records(raw[1], raw[2]["img_size"], info["flip"], info["affine"], info["scale_depth"],
                                                   info["canonical_scale"])).to(dev)
        want = encode_targets(_t(merged[0]), _t(merged[1]), records, on.settings._replace(cls_mean_size=on._cms))
        torch.cuda.synchronize()
        got = got3[b][0]
        for k in got:
            if k != "img_size":
                assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (b, k)
        assert got3[b][2] == tuple(int(v) for v in merged[2].sum(0))
        totals += merged[2].sum(0)
    print("pass 3: matched, created, missed, dropped, evicted, skipped = %s of %d remembered rows" % (totals.tolist(), n_rows))
    assert np.array_equal(R.bits(on.memory.bank.cpu().numpy()), R.bits(bank)) and np.array_equal(on.memory.count.cpu().numpy(), bank_count)
    assert totals[1] + totals[2] > 0                           # another model sees the frames differently
    on.close()


# ================================================================================================ 3. the Trainer
def _four_cycles(generated, shared, memory):
    """Four cycles as ``test_three_steps_with_the_key_on`` runs and counts them -> the rig, (synchronize calls, captures) per step."""
    import monosowa_amd.inference as inference
    extra = {} if memory is None else {"teacher_memory": memory}
    rig = G._Rig(generated[0], shared, [7, 8, 9, 10], teacher={"min_score": 0.0, "refresh": 2}, ema_decay=0.5, **extra)
    t = rig.trainer
    syncs, captures = [0], [0]
    real, init = torch.cuda.synchronize, inference._Graph.__init__
    torch.cuda.synchronize = lambda *a, **k: (syncs.__setitem__(0, syncs[0] + 1), real(*a, **k))[1]
    inference._Graph.__init__ = lambda self, *a, **k: (captures.__setitem__(0, captures[0] + 1), init(self, *a, **k))[1]
    try:
        np.random.seed(3)
        torch.manual_seed(3)
        per_step, remembered = [], []
        for raw in rig.loader:
            s0, c0 = syncs[0], captures[0]
            staged = t._teacher_turn()
            total, _ = t.train_cycle([raw], staged)
            per_step.append((syncs[0] - s0, captures[0] - c0))
            remembered.append(t._memory_counts)
            assert torch.isfinite(total).item()
    finally:
        torch.cuda.synchronize, inference._Graph.__init__ = real, init
    torch.cuda.synchronize()
    return rig, per_step, remembered


@pytest.fixture(scope="module")
def shared():
    return G._model(dropout=0.0)


def test_steps_synchronise_as_often_as_without_the_key_and_the_checkpoint_restores(generated, shared, tmp_path):
    from monosowa_amd import LabelMemory
    from monosowa_amd.helpers.save_helper import load_checkpoint, save_checkpoint
    plain, steps_off, remembered_off = _four_cycles(generated, shared, None)
    assert plain.teacher.memory is None and remembered_off == [None] * 4
    assert "teacher_memory" not in plain.trainer._checkpoint_state(0, 0)
    plain.teacher.close()
    rig, steps_on, remembered = _four_cycles(generated, shared, {"drop_below": 0.0})
    print("(synchronize calls, graph captures) per step, key off: %s, on: %s; memory per cycle: %s" % (steps_off, steps_on, remembered))
    assert steps_on == steps_off and steps_on[1] == (0, 0) and steps_on[3] == (0, 0)
    assert remembered[0] == (0, 0, 0, 0, 0) and all(sum(r) > 0 for r in remembered[1:])
    # save mid-run (a batch is in flight: its merge is in the bank once the stream is waited for, which state_dict() does)
    memory = rig.teacher.memory
    state = rig.trainer._checkpoint_state(0, 0)
    assert set(state) == {"epoch", "model_state", "optimizer_state", "best_result", "best_epoch", "ema_state", "teacher_memory"}
    save_checkpoint(state, str(tmp_path / "checkpoint"))
    torch.cuda.synchronize()
    want_bank, want_count = memory.bank.cpu().numpy(), memory.count.cpu().numpy()
    assert want_count.sum() > 0 and want_bank[:, :, 14].max() >= 1
    fresh = LabelMemory(memory.ids, memory.slots, memory.momentum, memory.iou, memory.drop_below, _dev())
    load_checkpoint(None, None, str(tmp_path / "checkpoint.pth"), _dev(), logger=logging.getLogger("memory"), memory=fresh)
    torch.cuda.synchronize()
    assert np.array_equal(R.bits(fresh.bank.cpu().numpy()), R.bits(want_bank)) and np.array_equal(fresh.count.cpu().numpy(), want_count)
    rig.teacher.close()
