"""``trainer.label_audit`` without a GPU: the key's validation, the float64 torch fallback of ``LabelAudit.observe`` against the
label-by-label reference (tests/label_audit_reference.py), the ring's bookkeeping, the refusals, ``tools/label_audit.py report`` on
hand-made files, the two criterion formulations handing ``observe`` the same pairs, and one epoch of the tiny CPU model with the key on.

BOUND is the one of tests/test_label_audit_gpu.py: 4 x the worst relative error of the float32 evaluation of the nine columns against
float64 on the shared cases.  The fallback evaluates in float64 itself, so it sits orders of magnitude inside."""
import csv
import logging
import os
import sys

import numpy as np
import pytest
import torch

import label_audit_reference as R
from test_accumulation_cpu import _Loader, _process_state, _seed_hook, _trainer      # noqa: F401  (_process_state: autouse fixture)
from test_distributed_gloo import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 5.2e-7           # see tests/test_label_audit_gpu.py


def _observe(audit, case, layer=0):
    audit.observe(*[case[k] for k in R.PRED], case["idx"], R.flat_of(case), layer=layer)


def _mask(sizes, slots=50):
    """Host object mask [B, slots] with sizes[b] objects in image b, not in the leading slots alone."""
    mask = np.zeros((len(sizes), slots), dtype=bool)
    for b, n in enumerate(sizes):
        mask[b, np.arange(n) * 2 + b] = True
    return mask


# --------------------------------------------------------------------------------------------------- 1. the key
def test_key_absent_none_or_false_is_off_and_anything_but_a_bool_raises():
    model, crit, opt = _build()
    loader = _Loader([])
    for cfg in ({}, {"label_audit": None}, {"label_audit": False}):
        trainer = _trainer(model, crit, opt, loader, **cfg)
        assert trainer.label_audit is None and crit.audit is None
    for bad in ("yes", 1, 0, "true", 1.0, [], {}):
        with pytest.raises(ValueError, match="label_audit"):
            _trainer(model, crit, opt, loader, label_audit=bad)
    assert crit.audit is None
    try:
        on = _trainer(model, crit, opt, _Loader([7, 8, 9]), label_audit=True)
        assert on.label_audit is not None and crit.audit is on.label_audit
        assert on.label_audit.capacity == 3 * 2 * 50 and on.label_audit.ring.shape == (300, 9) and on.label_audit.ring.dtype == torch.float64

        class _Set:
            max_objs = 7

            def __len__(self):
                return 11
        sized = _Loader([])
        sized.dataset = _Set()
        assert _trainer(model, crit, opt, sized, label_audit=True).label_audit.capacity == 77
    finally:
        crit.__dict__.pop("audit", None)
    import monosowa_amd
    from monosowa_amd.label_audit import LabelAudit
    assert monosowa_amd.LabelAudit is LabelAudit


# --------------------------------------------------------------------------------------------------- 2. the fallback
@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("layer", [0, 2])
def test_fallback_on_cpu_tensors_equals_the_float64_reference(name, layer):
    from monosowa_amd.label_audit import COLUMNS, LabelAudit
    case = R.shared_case(name)
    NL, B, C, Q, G, sizes = R.CASES[name]
    T = sum(sizes)
    audit = LabelAudit(T + 5, "cpu")
    audit.begin_batch(np.arange(B) + 100, _mask(sizes))
    _observe(audit, case, layer)
    assert audit.kernel_observes == 0
    got = audit.drain()
    want = R.rows(case, layer)
    err = R.rel_error(torch.from_numpy(got["values"]), want)
    print("\n%s layer %d: fallback against the reference %.3e (bound %.1e)" % (name, layer, err, BOUND))
    assert got["values"].shape == (T, 9) and got["values"].dtype == np.float64 and err <= BOUND
    assert (got["values"][:, 8] == G).all() and list(got["columns"]) == list(COLUMNS) and COLUMNS[4] == "depth_abs"
    assert np.array_equal(got["cls"], case["labels"].numpy())
    other = R.rows(case, 2 - layer)
    assert R.rel_error(torch.from_numpy(got["values"])[:, :8], other[:, :8]) > 1e-2          # the layers do differ


def test_a_label_without_a_pair_gets_zeros_and_a_nan_stays_in_its_row():
    from monosowa_amd.label_audit import LabelAudit
    case = {k: v.clone() for k, v in R.shared_case("G1").items()}
    case["idx"] = case["idx"][:, :, 1:].contiguous()                # the first label loses its only pair
    b, q, t = case["idx"][:, 0, 0].tolist()
    case["depth"][0, b, q, 0] = float("nan")
    audit = LabelAudit(3, "cpu")
    audit.begin_batch([5, 6, 7], _mask((1, 0, 2)))
    _observe(audit, case, 0)
    values = audit.drain()["values"]
    assert t in (1, 2) and not values[0].any()
    assert np.isnan(values[t, [3, 4]]).all() and np.isfinite(np.delete(values[t], [3, 4])).all() and np.isfinite(values[3 - t]).all()
    assert values[t, 8] == 1 and values[3 - t, 8] == 1


# --------------------------------------------------------------------------------------------------- 3. the ring
def test_offsets_keys_backlog_on_a_full_ring_and_drain_empties_it():
    from monosowa_amd.label_audit import LabelAudit
    case = R.shared_case("G1")
    sizes = (1, 0, 2)
    mask = _mask(sizes)
    audit = LabelAudit(7, "cpu")
    want = R.rows(case, 0)
    for step in range(5):
        off, T = audit.begin_batch([10 * step, 10 * step + 1, 10 * step + 2], mask, epoch=step // 2)
        assert (off, T) == ((0, 3, 0, 3, 0)[step], 3)                # 3 + 3 fit 7 rows, the third batch drains first
        _observe(audit, case, 0)
        assert audit.early_drains == step // 2 and len(audit._backlog) == step // 2
    got = audit.drain()
    assert got["img_id"].tolist() == [i for s in range(5) for i in (10 * s, 10 * s + 2, 10 * s + 2)]
    assert got["line"].tolist() == [0, 2, 4] * 5 and got["epoch"].tolist() == [0] * 6 + [1] * 6 + [2] * 3
    assert got["values"].shape == (15, 9) and all(np.array_equal(got["values"][3 * s:3 * s + 3], want.numpy()) for s in range(5))
    again = audit.drain()
    assert again["values"].shape == (0, 9) and len(again["img_id"]) == 0 and not audit.ring.any() and audit._fill == 0
    # a batch that was begun and never observed leaves no rows
    audit.begin_batch([1, 2, 3], mask)
    audit.begin_batch([4, 5, 6], mask)
    _observe(audit, case, 0)
    assert audit.drain()["img_id"].tolist() == [4, 6, 6]
    with pytest.raises(ValueError, match="does not fit"):
        LabelAudit(2, "cpu").begin_batch([1, 2, 3], mask)
    with pytest.raises(ValueError, match="at least 1"):
        LabelAudit(0, "cpu")


def test_begin_batch_takes_the_mask_from_the_host_and_refuses_a_device_mask_without_one():
    from monosowa_amd.label_audit import LabelAudit, host_mask_of
    from monosowa_amd.synthetic import attach_host_mask
    mask = _mask((2, 1))
    audit = LabelAudit(8, "cpu")
    assert audit.begin_batch([3, 4], torch.from_numpy(mask)) == (0, 3)
    carried = attach_host_mask(torch.zeros(2, 50, dtype=torch.bool), mask)        # the attached copy wins over the tensor's own values
    assert audit.begin_batch([3, 4], carried) == (0, 3)

    class _OnDevice:
        is_cuda = True
    with pytest.raises(ValueError, match="attach_host_mask"):
        host_mask_of(_OnDevice())
    with pytest.raises(ValueError, match="attach_host_mask"):
        audit.begin_batch([3, 4], _OnDevice())


def test_observe_refuses_another_number_of_targets_and_a_call_without_begin_batch():
    from monosowa_amd.label_audit import LabelAudit
    case = R.shared_case("G1")
    audit = LabelAudit(8, "cpu")
    with pytest.raises(RuntimeError, match="begin_batch"):
        _observe(audit, case)
    audit.begin_batch([1, 2, 3], _mask((1, 0, 3)))
    with pytest.raises(ValueError, match="3 targets, begin_batch reserved 4"):
        _observe(audit, case)
    audit.begin_batch([1, 2, 3], _mask((1, 0, 2)))
    with pytest.raises(ValueError, match="layer"):
        _observe(audit, case, layer=3)


# --------------------------------------------------------------------------------------------------- 4. report
def _npz(path, img_id, line, cls, depth_abs, count):
    from monosowa_amd.label_audit import COLUMNS, save
    values = np.zeros((len(line), 9))
    values[:, 4], values[:, 8] = depth_abs, count
    values[:, 0] = np.asarray(depth_abs) * 10.0
    save(path, {"epoch": np.zeros(len(line), np.int64), "img_id": np.asarray(img_id), "line": np.asarray(line), "cls": np.asarray(cls),
                "values": values, "columns": np.asarray(COLUMNS)})


def test_report_averages_over_the_last_epochs_and_ranks(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import label_audit as tool
    finally:
        sys.path.pop(0)
    d = str(tmp_path / "label_audit")
    # two epochs; epoch 1 comes from two ranks.  Label (7, 0) is seen in both epochs, (7, 1) twice in epoch 1 (once per rank)
    _npz(os.path.join(d, "epoch_000.npz"), [7, 7, 9], [0, 1, 3], [1, 2, 0], [1.0, 8.0, 0.5], [3, 3, 3])
    _npz(os.path.join(d, "epoch_001.rank0.npz"), [7, 7], [0, 1], [1, 2], [2.5, 2.0], [3, 3])
    _npz(os.path.join(d, "epoch_001.rank1.npz"), [7, 4], [1, 2], [2, 1], [4.0, float("nan")], [3, 3])
    open(os.path.join(d, "notes.txt"), "w").write("not a record\n")
    assert sorted(tool.epoch_files(d)) == [0, 1] and len(tool.epoch_files(d)[1]) == 2
    columns, rows = tool.report(d)
    key = lambda r: (r["img_id"], r["line"])
    assert [key(r) for r in rows] == [(4, 2), (7, 1), (7, 0), (9, 3)]                   # NaN in front, then by the mean of depth_abs
    by = {key(r): r for r in rows}
    assert by[(7, 1)]["depth_abs"] == pytest.approx((8.0 + 2.0 + 4.0) / 3) and by[(7, 1)]["seen"] == 3 and by[(7, 1)]["cls"] == 2
    assert by[(7, 0)]["depth_abs"] == pytest.approx(1.75) and by[(7, 0)]["center"] == pytest.approx(17.5) and by[(7, 0)]["count"] == 3.0
    _, last = tool.report(d, last=1)
    assert [key(r) for r in last] == [(4, 2), (7, 1), (7, 0)] and {key(r): r for r in last}[(7, 1)]["depth_abs"] == pytest.approx(3.0)
    _, by_center = tool.report(d, by="center")
    assert [key(r) for r in by_center][1:] == [(7, 1), (7, 0), (9, 3)]
    with pytest.raises(ValueError, match="--by"):
        tool.report(d, by="nothing")
    out = str(tmp_path / "ranked.csv")
    tool.main(["report", d, "--last", "2", "--top", "2", "--csv", out])
    table = list(csv.reader(open(out)))
    assert table[0] == ["img_id", "line", "cls", "seen", "center", "bbox", "giou", "depth", "depth_abs", "size", "angle", "score", "count"]
    assert len(table) == 5 and table[2][:4] == ["7", "1", "2", "3"] and float(table[2][8]) == pytest.approx(14.0 / 3)
    printed = capsys.readouterr().out.splitlines()
    assert printed[0].startswith("4 labels, ranked by depth_abs") and len(printed) == 4


# --------------------------------------------------------------------------------------------------- 5. the criterion
class _Spy:
    def __init__(self):
        self.calls = []

    def observe(self, *args, **kwargs):
        self.calls.append((args, kwargs))


def test_both_formulations_hand_observe_the_same_pairs_and_the_losses_do_not_change():
    from monosowa_amd.synthetic import make_batch, prepare_targets
    from test_accumulation_cpu import RES
    model, crit, _ = _build()
    inputs, calibs, targets, _ = make_batch(2, "cpu", seed=7, resolution=RES)
    tl = prepare_targets(targets, 2)
    torch.manual_seed(100)
    with torch.no_grad():
        outputs = model(inputs, calibs, tl, targets["img_size"])
        plain = crit.forward_fast(outputs, tl)
        spy = _Spy()
        crit.audit = spy
        try:
            fast = crit.forward_fast(outputs, tl)
            crit.forward_layerwise(outputs, tl)
        finally:
            del crit.audit
    assert crit.audit is None and len(spy.calls) == 2
    assert all(torch.equal(plain[k], fast[k]) for k in plain) and len(plain.keys()) > 20
    (a, ka), (b, kb) = spy.calls
    assert ka == kb == {"layer": 0}
    T = int(targets["mask_2d"].sum())
    assert a[5].shape == (3, len(outputs["aux_outputs"]) + 1, T * crit.group_num) and b[5].shape == (3, 1, T * crit.group_num)
    assert torch.equal(a[5][:, 0], b[5][:, 0])
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x[0], y[0]) and not x.requires_grad
    assert all(torch.equal(a[6][k].reshape(-1), b[6][k].reshape(-1)) for k in ("labels", "boxes_3d", "depth", "size_3d", "heading_bin", "heading_res"))
    assert torch.equal(R.rows(R.case_of_observe(a), 0), R.rows(R.case_of_observe(b), 0))


# --------------------------------------------------------------------------------------------------- 6. the Trainer on the CPU
def test_one_epoch_on_the_cpu_writes_the_epochs_file_with_the_loaders_keys(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    model, crit, opt = _build()
    _seed_hook(model)
    loader = _Loader([7, 8])
    for i, batch in enumerate(loader.batches):
        batch[3]["img_id"] = np.array([100 * i + 4, 100 * i + 2])
    try:
        trainer = _trainer(model, crit, opt, loader, label_audit=True)
        trainer.log_interval = 10 ** 9
        lines = []
        handler = logging.Handler()
        handler.emit = lambda record: lines.append(record.getMessage())
        trainer.logger.addHandler(handler)
        level = trainer.logger.level
        trainer.logger.setLevel(logging.INFO)
        try:
            trainer.train_one_epoch(0)
        finally:
            trainer.logger.removeHandler(handler)
            trainer.logger.setLevel(level)
    finally:
        crit.__dict__.pop("audit", None)
    folder = os.path.join("outputs", "tiny", "label_audit")
    assert os.listdir(folder) == ["epoch_000.npz"]
    got = np.load(os.path.join(folder, "epoch_000.npz"))
    want_ids, want_lines = [], []
    for batch in loader.batches:
        hb, hs = np.nonzero(batch[2]["mask_2d"].numpy())
        want_ids += batch[3]["img_id"][hb].tolist()
        want_lines += hs.tolist()
    assert got["img_id"].tolist() == want_ids and got["line"].tolist() == want_lines and len(want_ids) > 4
    assert (got["values"][:, 8] == crit.group_num).all() and (got["cls"] == 1).all() and np.isfinite(got["values"]).all()
    assert (got["values"][:, [0, 1, 2, 4, 5, 6]] > 0).all() and ((got["values"][:, 7] > 0) & (got["values"][:, 7] < 1)).all()
    assert any(l.startswith("Epoch 0: label audit: %d labels seen, |d - d*| median: " % len(want_ids)) and "max: " in l for l in lines)
