"""Label audit (``trainer.label_audit``): what the criterion's matched-pair terms say about every single label, kept on the device.

    audit = LabelAudit(capacity_rows, device)                   # capacity: labels seen between two drains
    criterion.audit = audit
    audit.begin_batch(info["img_id"], targets["mask_2d"])       # before the forward: T rows reserved, their keys noted on the host
    loss_dict = criterion(model(...), target_list)              # the criterion calls audit.observe(...) behind its matching
    record = audit.drain()                                      # the only call that waits for the device

MonoSOWA trains on labels a machine wrote; the record answers which of them the model keeps disagreeing with.  The matcher pairs every
label with ``group_num`` queries (one in eval mode) and ``csrc/matched_losses.hip`` evaluates the loss terms per pair; ``observe`` makes
``mono_label_audit_f32`` (include/monosowa_pointwise.h) write, per label, the mean of every term over its pairs of the final decoder
layer, straight into the reserved rows of a ``[capacity, 9]`` float64 ring -- one launch, no atomics, no synchronisation.  The columns
(``COLUMNS``): centre L1, l/r/t/b L1, 1 - GIoU, the Laplacian depth term, |d - d*|, plain size L1, heading cross entropy + residual L1,
the matched queries' score for the label's class, and the number of pairs.

The identity of a label never travels to the device: ``prepare_targets`` flattens a batch in the row-major order of the host object
mask, and slot ``i`` of a sample's padded arrays is object ``i`` of its label file, so flat target ``t`` is (image ``hb[t]``, label line
``hs[t]``) of ``np.nonzero(host_mask)``.  ``begin_batch`` notes ``(epoch, img_id, line)`` per reserved row; ``drain`` joins them.  The
class of a label is copied beside its row on the device (one small device-to-device copy per ``observe``).

Two limits.  The terms are measured in the frame of that step's augmentation (flip, crop, canonical depth), and only the labels that
pass the dataset's filter and ``mask_2d`` ever appear.

On CPU tensors, another dtype than float32, more than 255 classes or without the built library the same columns come from torch
operations in float64 (``columns_torch``); that path may synchronise.  A ``begin_batch`` on a full ring first drains it into a host
backlog -- a synchronisation; size ``capacity`` to the labels between two drains and it never happens."""
import os

import numpy as np
import torch

COLUMNS = ("center", "bbox", "giou", "depth", "depth_abs", "size", "angle", "score", "count")
WIDTH = len(COLUMNS)


def host_mask_of(mask):
    """The object mask of a batch as a host bool array without a device synchronisation: a numpy array, a CPU tensor, or a device
    tensor that carries ``synthetic.attach_host_mask``'s copy."""
    if isinstance(mask, np.ndarray):
        return mask.astype(bool)
    host = getattr(mask, "_host_mask", None)
    if host is None:
        if mask.is_cuda:
            raise ValueError("the label audit names the labels of a batch on the host: a device-resident batch needs "
                             "synthetic.attach_host_mask on its mask_2d")
        host = mask.numpy()
    return np.asarray(host).astype(bool)


def columns_torch(logits, boxes, depth, dims, angle, idx, flat, layer, T):
    """The ``[T, 9]`` float64 rows of ``mono_label_audit_f32`` through torch operations, every term evaluated in float64."""
    f64 = torch.float64
    dev = logits.device
    b, q, t = idx[0, layer], idx[1, layer], idx[2, layer]
    K = t.shape[0]
    take = lambda x: x[layer][b, q].to(f64)
    pb, tb = take(boxes), flat["boxes_3d"].to(f64)[t]
    center = (pb[:, 0:2] - tb[:, 0:2]).abs().sum(1)
    bbox = (pb[:, 2:6] - tb[:, 2:6]).abs().sum(1)
    xyxy = lambda c: torch.stack([c[:, 0] - c[:, 2], c[:, 1] - c[:, 4], c[:, 0] + c[:, 3], c[:, 1] + c[:, 5]], 1)
    xa, xb = xyxy(pb), xyxy(tb)
    area_a, area_b = (xa[:, 2] - xa[:, 0]) * (xa[:, 3] - xa[:, 1]), (xb[:, 2] - xb[:, 0]) * (xb[:, 3] - xb[:, 1])
    wh = (torch.min(xa[:, 2:], xb[:, 2:]) - torch.max(xa[:, :2], xb[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = area_a + area_b - inter
    wh_c = (torch.max(xa[:, 2:], xb[:, 2:]) - torch.min(xa[:, :2], xb[:, :2])).clamp(min=0)
    hull = wh_c[:, 0] * wh_c[:, 1]
    giou = 1 - (inter / union - (hull - union) / hull)
    pd, td = take(depth), flat["depth"].reshape(-1).to(f64)[t]
    dabs = (pd[:, 0] - td).abs()
    dep = 1.4142 * torch.exp(-pd[:, 1]) * dabs + pd[:, 1]
    size = (take(dims) - flat["size_3d"].to(f64)[t]).abs().sum(1)
    pa = take(angle)
    bins = flat["heading_bin"].reshape(-1).long()[t]
    ce = -torch.gather(torch.log_softmax(pa[:, 0:12], dim=1), 1, bins.view(-1, 1)).squeeze(1)
    res = torch.gather(pa[:, 12:24], 1, bins.view(-1, 1)).squeeze(1)
    ang = ce + (res - flat["heading_res"].reshape(-1).to(f64)[t]).abs()
    cls = flat["labels"].reshape(-1).long()[t]
    score = torch.sigmoid(torch.gather(take(logits), 1, cls.view(-1, 1)).squeeze(1))
    terms = torch.stack([center, bbox, giou, dep, dabs, size, ang, score], 1) if K else torch.zeros((0, WIDTH - 1), dtype=f64, device=dev)
    sums = torch.zeros((T, WIDTH - 1), dtype=f64, device=dev).index_add_(0, t, terms)
    count = torch.zeros(T, dtype=f64, device=dev).index_add_(0, t, torch.ones(K, dtype=f64, device=dev))
    means = torch.where(count.view(T, 1) > 0, sums / count.view(T, 1), torch.zeros((), dtype=f64, device=dev))
    return torch.cat([means, count.view(T, 1)], 1)


def _empty():
    return {"epoch": np.zeros(0, np.int64), "img_id": np.zeros(0, np.int64), "line": np.zeros(0, np.int64), "cls": np.zeros(0, np.int64),
            "values": np.zeros((0, WIDTH), np.float64)}


class LabelAudit:
    def __init__(self, capacity_rows, device):
        capacity = int(capacity_rows)
        if capacity < 1:
            raise ValueError("LabelAudit: capacity_rows must be at least 1, got %r" % (capacity_rows,))
        self.capacity = capacity
        self.device = torch.device(device)
        self.ring = torch.zeros(capacity, WIDTH, dtype=torch.float64, device=self.device)
        self.cls = torch.zeros(capacity, dtype=torch.int64, device=self.device)
        self._keys = []                  # host side of the rows in the ring, one (epoch [T], img_id [T], line [T]) per batch
        self._fill = 0                   # rows of the ring that are reserved
        self._open = None                # (offset, T) of the batch begin_batch reserved and observe has not yet served
        self._backlog = []               # parts drained early by a begin_batch on a full ring
        self.kernel_observes = 0         # observes served by mono_label_audit_f32
        self.early_drains = 0

    # ------------------------------------------------------------------------------------------------------------------ reserve
    def _drop_open(self):
        """A batch that was begun and never observed (its forward raised, or the criterion was not called) leaves no rows."""
        if self._open is not None:
            self._fill = self._open[0]
            self._keys.pop()
            self._open = None

    def begin_batch(self, img_ids, host_mask, epoch=0):
        """Reserves one row per object of ``host_mask`` ([B, max_objs], see ``host_mask_of``) in ``prepare_targets``' order and
        notes ``(epoch, img_ids[image], slot)`` for each.  Returns ``(offset, T)``.  Nothing is sent to the device."""
        self._drop_open()
        ids = np.asarray(img_ids).reshape(-1)
        host = host_mask_of(host_mask)
        if host.ndim != 2 or host.shape[0] < len(ids):
            raise ValueError("LabelAudit.begin_batch: a [B, max_objs] mask for %d images is needed, got shape %r" % (len(ids), host.shape))
        hb, hs = np.nonzero(host[:len(ids)])                 # row-major = per image, slot order: prepare_targets' order
        T = len(hb)
        if T > self.capacity:
            raise ValueError("LabelAudit.begin_batch: a batch of %d labels does not fit a ring of %d rows" % (T, self.capacity))
        if self._fill + T > self.capacity:
            self._backlog.append(self._collect())             # a synchronisation: the ring was sized too small
            self.early_drains += 1
        self._open = (self._fill, T)
        self._keys.append((np.full(T, int(epoch), np.int64), ids[hb], hs.astype(np.int64)))
        self._fill += T
        return self._open

    # ------------------------------------------------------------------------------------------------------------------ observe
    @staticmethod
    def _kernel_serves(logits):
        from . import pointwise
        return pointwise.label_audit_supported(logits) and os.path.exists(os.environ.get("MONOSOWA_POINTWISE_LIB", pointwise._PATH))

    def observe(self, logits, boxes, depth, dims, angle, idx, flat, layer=0):
        """The rows of the open batch from the stacked predictions ``[NL, B, Q, C | 6 | 2 | 3 | 24]``, the matched pairs ``idx``
        ``[3, NL, K]`` (image, query, flat target; on the predictions' device) and the batch-flat targets ``flat``.  Call it under
        ``torch.no_grad()`` with detached tensors.  On the kernel path: one launch into the ring and one copy of the classes beside
        it; nothing waits for the device."""
        if self._open is None:
            raise RuntimeError("LabelAudit.observe without an open begin_batch")
        off, T = self._open
        if flat["labels"].shape[0] != T:
            raise ValueError("LabelAudit.observe: the criterion has %d targets, begin_batch reserved %d rows"
                             % (flat["labels"].shape[0], T))
        if not 0 <= layer < logits.shape[0]:
            raise ValueError("LabelAudit.observe: layer %r of %d" % (layer, logits.shape[0]))
        self._open = None
        if T == 0:
            return
        if logits.device != self.device:
            raise ValueError("LabelAudit.observe: predictions on %s, the ring on %s" % (logits.device, self.device))
        f32, i64 = torch.float32, torch.int64
        labels = flat["labels"].reshape(-1).to(i64).contiguous()
        self.cls[off:off + T].copy_(labels)
        if self._kernel_serves(logits):
            from .pointwise import label_audit
            preds = [t.contiguous() for t in (logits, boxes, depth, dims, angle)]
            if any(t.dtype != f32 for t in preds):
                raise ValueError("LabelAudit.observe: the predictions are not all float32")
            tgt = (flat["boxes_3d"].to(f32).contiguous(), flat["depth"].reshape(-1).to(f32).contiguous(),
                   flat["size_3d"].to(f32).contiguous(), flat["heading_bin"].reshape(-1).to(i64).contiguous(),
                   flat["heading_res"].reshape(-1).to(f32).contiguous())
            label_audit(*preds, idx.to(i64).contiguous(), labels, *tgt, self.ring.data_ptr() + 8 * WIDTH * off, T, int(layer))
            self.kernel_observes += 1
        else:
            self.ring[off:off + T].copy_(columns_torch(logits, boxes, depth, dims, angle, idx, flat, int(layer), T))

    # ------------------------------------------------------------------------------------------------------------------ drain
    def _collect(self):
        """The reserved rows of the ring and their keys as host arrays; the ring starts over (zeroed).  Waits for the device."""
        self._drop_open()
        n = self._fill
        if n == 0:
            return _empty()
        values = self.ring[:n].to("cpu", copy=True).numpy()
        cls = self.cls[:n].to("cpu", copy=True).numpy()
        self.ring.zero_()
        part = {"epoch": np.concatenate([k[0] for k in self._keys]), "img_id": np.concatenate([k[1] for k in self._keys]),
                "line": np.concatenate([k[2] for k in self._keys]), "cls": cls, "values": values}
        self._keys, self._fill = [], 0
        return part

    def drain(self):
        """Every row since the last drain, oldest first: ``{"epoch", "img_id", "line", "cls", "values" [N, 9], "columns"}``; the ring
        starts over.  The only call that is meant to wait for the device."""
        parts = [p for p in self._backlog + [self._collect()] if len(p["line"])]
        self._backlog = []
        out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]} if parts else _empty()
        out["columns"] = np.asarray(COLUMNS)
        return out

    # ------------------------------------------------------------------------------------------------------------------ scan
    def scan(self, model, criterion, loader, device):
        """One pass over ``loader`` in eval mode under ``no_grad`` -- ``group_num`` is 1 there, so every label has one pair -- and the
        drained record: an existing label set audited with a trained checkpoint.  The modes and ``criterion.audit`` are put back."""
        from .helpers.trainer_helper import stage_batch
        from .synthetic import prepare_targets
        modes, own, before = (model.training, criterion.training), "audit" in criterion.__dict__, getattr(criterion, "audit", None)
        model.eval(), criterion.eval()
        criterion.audit = self
        try:
            with torch.no_grad():
                for raw in loader:
                    inputs, calibs, targets, info = stage_batch(raw, device)
                    self.begin_batch(info["img_id"], targets["mask_2d"])
                    target_list = prepare_targets(targets, inputs.shape[0])
                    criterion(model(inputs, calibs, target_list, targets["img_size"]), target_list)
        finally:
            if own:
                criterion.audit = before
            else:                                              # the class attribute (None) shows again
                criterion.__dict__.pop("audit", None)
            model.train(modes[0]), criterion.train(modes[1])
        return self.drain()


def save(path, record):
    """One drained record as an ``.npz`` (the format ``tools/label_audit.py report`` merges)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **record)
