"""Self-training in the train loop (``trainer.teacher``): a teacher's KITTI rows become the student's targets on the device.

    settings = encode_settings(dataset, min_score, weights)      what the encode reads of a dataset's settings
    records  = student_records(P2, img_size, flip, affine, scale_depth, canonical_scale)      float64 [B, RECORD_DOUBLES]
    targets  = encode_targets(rows, count, records, settings)    one launch of mono_encode_targets_f64 (include/monosowa_kitti.h)
    targets  = encode_targets_host(rows, count, records, settings)      the same contract in numpy scalars (CPU, max_objs > 64)
    teacher  = Teacher(cfg, model, device)                       refresh() / submit(raw) / collect(): see the class

The contract (include/monosowa_kitti.h has it in full).  ``rows`` float64 ``[B, R, 14]`` and ``count`` are what
``mono_decode_dets_f64`` / ``mono_fuse_dets_f64`` leave.  Slot ``i < min(count, max_objs)`` of every output is line ``i`` of the label
file ``write_kitti_results(..., dontcare_below=min_score)`` would write from the rows if it wrote every number exactly, read by
``KITTI_Dataset.__getitem__`` on a training split with ``label_weights: score`` and ``ignore_regions: true`` under the record's flip
and crop: rows scoring ``min_score`` or more are targets weighted by their score (or by a constant), the others -- and the rows the
dataset's filters drop -- are ignore boxes, packed at the front.  The outputs are the dataset's target dict as ``[B, max_objs, ...]``
with the dataset's dtypes, plus ``label_weight``, ``ignore_boxes``, ``ignore_mask`` and ``n_ignore`` int32 ``[B]``.

Two stated differences from the class: ``rect_to_img``'s and ``affine_transform``'s small matrix products are evaluated left to right
in double, each operation rounded (numpy hands them to BLAS, whose order differs), and the kernel's float32 ``atan2`` is the double
one rounded where the host function calls numpy's.
"""
import collections
import ctypes

import numpy as np
import torch

RECORD_DOUBLES = 23            # P2 (12), img_w, img_h, flip, trans (6), crop_scale, canonical_scale  (csrc/encode_targets.h)
MAX_DEVICE_OBJS = 64           # one lane per slot
DEPTH_MODES = {"normal": 0, "inverse": 1, "none": 2}
# name -> (dtype, trailing shape); the order of the kernel's output pointers
OUTPUTS = collections.OrderedDict([
    ("labels", (torch.int8, ())), ("boxes", (torch.float32, (4,))), ("boxes_3d", (torch.float32, (6,))), ("depth", (torch.float32, (1,))),
    ("size_2d", (torch.float32, (2,))), ("size_3d", (torch.float32, (3,))), ("src_size_3d", (torch.float32, (3,))),
    ("heading_bin", (torch.int64, (1,))), ("heading_res", (torch.float32, (1,))), ("mask_2d", (torch.bool, ())),
    ("calibs", (torch.float32, (3, 4))), ("indices", (torch.int64, ())), ("objects", (torch.float32, (7,))),
    ("label_weight", (torch.float32, ())), ("ignore_boxes", (torch.float32, (4,))), ("ignore_mask", (torch.bool, ()))])

EncodeSettings = collections.namedtuple("EncodeSettings", "writelist_mask cls_mean_size depth_mode clip_2d min_score weight_mode weight "
                                                          "resolution max_objs")


def check_weights(value):
    """``trainer.teacher.weights``: 'score' -> (0, 0.0); a finite number that is not negative -> (1, number)."""
    if value == "score" and isinstance(value, str):
        return 0, 0.0
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not np.isfinite(value) or value < 0:
        raise ValueError("trainer.teacher.weights = %r is neither 'score' nor a finite number that is not negative" % (value,))
    return 1, float(value)


def encode_settings(dataset, min_score, weights="score"):
    """What the encode reads of a dataset's settings (a ``KITTI_Dataset`` or ``KITTI_Dataset.settings(cfg)``)."""
    if dataset.aug_calib:
        raise ValueError("dataset.aug_calib refits P2 of a flipped frame by an SVD on the host: the teacher's targets are encoded on "
                         "the device and do not support it")
    if dataset.depth_scale not in DEPTH_MODES:
        raise ValueError("dataset.depth_scale = %r is not one of %s" % (dataset.depth_scale, sorted(DEPTH_MODES)))
    # the class makes an ignore box of a line whose class is in dataset.ignore_classes and not in the writelist; the encode knows
    # DontCare and writelist lines only, which is the same thing unless a class the detector can name is ignored that way
    clash = sorted(set(getattr(dataset, "ignore_classes", None) or ()) & (set(dataset.class_name) - set(dataset.writelist)))
    if clash:
        raise ValueError("dataset.ignore_classes names %s, which the teacher can detect and the writelist leaves out: the class would "
                         "make ignore boxes of such rows and the device encode drops them; take them out of ignore_classes or into "
                         "the writelist" % ", ".join(clash))
    mask = 0
    for c, name in enumerate(dataset.class_name):
        if name in dataset.writelist:
            mask |= 1 << c
    mode, weight = check_weights(weights)
    return EncodeSettings(mask, np.ascontiguousarray(dataset.cls_mean_size, dtype=np.float64), DEPTH_MODES[dataset.depth_scale],
                          bool(dataset.clip_2d), float(min_score), mode, weight,
                          (int(dataset.resolution[0]), int(dataset.resolution[1])), int(dataset.max_objs))


def student_records(P2, img_size, flip, affine, scale_depth, canonical_scale):
    """float64 ``[B, RECORD_DOUBLES]`` from a collated batch's calibs ``[B, 3, 4]`` and ``info`` entries (arrays or tensors)."""
    arr = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    P2 = arr(P2).astype(np.float32).reshape(-1, 12)
    B = P2.shape[0]
    rec = np.zeros((B, RECORD_DOUBLES), dtype=np.float64)
    rec[:, 0:12] = P2
    rec[:, 12:14] = arr(img_size).reshape(B, 2)
    rec[:, 14] = arr(flip).reshape(B).astype(bool)
    rec[:, 15:21] = arr(affine).reshape(B, 6)
    rec[:, 21] = arr(scale_depth).reshape(B)
    rec[:, 22] = arr(canonical_scale).reshape(B)
    return rec


def empty_outputs(B, max_objs, device):
    out = {k: torch.empty((B, max_objs) + shape, dtype=dtype, device=device) for k, (dtype, shape) in OUTPUTS.items()}
    out["n_ignore"] = torch.empty((B,), dtype=torch.int32, device=device)
    return out


def encode_targets(rows, count, records, settings, out=None):
    """One launch of ``mono_encode_targets_f64`` on the current stream: rows float64 ``[B, R, 14]``, count int32 ``[B]``, records
    float64 ``[B, RECORD_DOUBLES]`` (contiguous CUDA tensors) -> dict of the outputs (``out``: a dict of such tensors to write into).
    ``max_objs > 64`` is a ValueError: the caller takes ``encode_targets_host``."""
    from .kitti_eval import load
    if rows.dim() != 3 or rows.shape[2] != 14 or rows.dtype != torch.float64 or not rows.is_cuda or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float64 CUDA tensor [B, R, 14], got %s %s" % (rows.dtype, tuple(rows.shape)))
    B, R, _ = rows.shape
    cms = settings.cls_mean_size
    if not isinstance(cms, torch.Tensor):
        cms = torch.from_numpy(cms).to(rows.device)
    for name, t, dtype, shape in (("count", count, torch.int32, (B,)), ("records", records, torch.float64, (B, RECORD_DOUBLES)),
                                  ("cls_mean_size", cms, torch.float64, (cms.shape[0], 3))):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != rows.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor %s on %s, got %s %s on %s"
                             % (name, dtype, shape, rows.device, t.dtype, tuple(t.shape), t.device))
    n = settings.max_objs
    if n > MAX_DEVICE_OBJS:
        raise ValueError("the encode kernel has one lane per slot: max_objs = %d > %d takes encode_targets_host" % (n, MAX_DEVICE_OBJS))
    if out is None:
        out = empty_outputs(B, n, rows.device)
    names = list(OUTPUTS) + ["n_ignore"]
    for k in names:
        dtype, shape = OUTPUTS[k] if k in OUTPUTS else (torch.int32, None)
        want = (B, n) + shape if shape is not None else (B,)
        t = out[k]
        if t.dtype != dtype or tuple(t.shape) != want or t.device != rows.device or not t.is_contiguous():
            raise ValueError("out[%r] must be a contiguous %s tensor %s on %s" % (k, dtype, want, rows.device))
    pointers = (ctypes.c_void_p * len(names))(*[out[k].data_ptr() for k in names])
    with torch.cuda.device(rows.device):
        code = load().mono_encode_targets_f64(rows.data_ptr(), count.data_ptr(), records.data_ptr(), cms.data_ptr(),
                                              settings.writelist_mask, settings.depth_mode, int(settings.clip_2d), settings.min_score,
                                              settings.weight_mode, settings.weight, settings.resolution[0], settings.resolution[1],
                                              B, R, int(cms.shape[0]), n, pointers, torch.cuda.current_stream().cuda_stream)
    if code:
        raise RuntimeError("mono_encode_targets_f64 failed with code %d" % code)
    return out


_F, _D = np.float32, np.float64
_PI = 3.141592653589793


def _affine(t, x, y):
    """``affine_transform`` left to right in double: t float64 [6], x and y float32."""
    return t[0] * _D(x) + t[1] * _D(y) + t[2], t[3] * _D(x) + t[4] * _D(y) + t[5]


def _mod(a, b):
    """numpy's float32 ``%`` for b > 0."""
    m = _F(np.fmod(a, b))
    if m != 0:
        if m < 0:
            m = _F(m + b)
    else:
        m = _F(0.0)
    return m


def _wrap32(a):
    pi, two_pi = _F(_PI), _F(2 * _PI)
    return _F(a - two_pi) if a > pi else (_F(a + two_pi) if a < -pi else a)


def _clip(v, zero, one):
    return zero if v < 0 else (one if v > 1 else v)


def encode_targets_host(rows, count, records, settings):
    """``mono_encode_targets_f64``'s contract in numpy scalars -> dict of numpy arrays (``mask_2d`` / ``ignore_mask`` bool)."""
    rows, count = np.asarray(rows, dtype=np.float64), np.asarray(count)
    records = np.asarray(records, dtype=np.float64)
    B, R, _ = rows.shape
    n_max, C = settings.max_objs, settings.cls_mean_size.shape[0]
    np_dtype = {torch.int8: np.int8, torch.float32: np.float32, torch.int64: np.int64, torch.bool: bool}
    out = {k: np.zeros((B, n_max) + shape, dtype=np_dtype[dtype]) for k, (dtype, shape) in OUTPUTS.items()}
    out["label_weight"][:] = 1.0
    out["n_ignore"] = np.zeros(B, dtype=np.int32)
    res_w, res_h = _D(settings.resolution[0]), _D(settings.resolution[1])
    bin_size = 2 * _PI / 12.0
    with np.errstate(all="ignore"):
        for b in range(B):
            rec = records[b]
            P = rec[0:12].astype(np.float32)
            img_w, flip, t, crop_scale, canonical_scale = rec[12], rec[14] != 0, rec[15:21], rec[21], rec[22]
            packed = 0
            for i in range(int(min(max(count[b], 0), R, n_max))):
                r = rows[b, i]
                score = r[13]
                dontcare = not (score >= settings.min_score)
                named = bool(r[0] > -1.0 and r[0] < C)
                cls = int(r[0]) if named else 0
                listed = (not dontcare) and named and bool((settings.writelist_mask >> cls) & 1)
                if settings.weight_mode == 0:
                    out["label_weight"][b, i] = _F(score) if (score >= 0 and np.isfinite(score)) else _F(0.0)
                else:
                    out["label_weight"][b, i] = _F(settings.weight)
                x1, y1, x2, y2 = _F(r[2]), _F(r[3]), _F(r[4]), _F(r[5])
                h, w, l = r[6], r[7], r[8]
                px, py, pz = _F(r[9]), _F(r[10]), _F(r[11])
                ry = r[12]
                unknown = not (_D(y2) - _D(y1) + 1.0 >= 25.0)
                if flip:
                    x1, x2 = _F(img_w - _D(x2)), _F(img_w - _D(x1))
                    ry = _PI - ry
                    ry = ry - 2 * _PI if ry > _PI else (ry + 2 * _PI if ry < -_PI else ry)
                ignore, target = dontcare or listed, False
                if listed and not unknown and not (pz < 2 or pz > 65):
                    a, c = _affine(t, x1, y1)
                    bx0, by0 = _F(a), _F(c)
                    a, c = _affine(t, x2, y2)
                    bx1, by1 = _F(a), _F(c)
                    c2x, c2y = _F(_F(bx0 + bx1) / _F(2)), _F(_F(by0 + by1) / _F(2))
                    X, Y, Z = _D(px), _D(py) + (-(h / 2)), _D(pz)
                    p0 = X * _D(P[0]) + Y * _D(P[1]) + Z * _D(P[2]) + _D(P[3])
                    p1 = X * _D(P[4]) + Y * _D(P[5]) + Z * _D(P[6]) + _D(P[7])
                    u, v = p0 / Z, p1 / Z
                    if flip:
                        u = img_w - u
                    cx, cy = _affine(t, _F(u), _F(v))
                    if not (cx < 0 or cx >= res_w or cy < 0 or cy >= res_h):
                        out["labels"][b, i] = cls
                        s2w, s2h = _F(bx1 - bx0), _F(by1 - by0)
                        out["size_2d"][b, i] = s2w, s2h
                        k0, k1, k2, k3 = _F(_D(bx0) / res_w), _F(_D(by0) / res_h), _F(_D(bx1) / res_w), _F(_D(by1) / res_h)
                        c3x, c3y = cx / res_w, cy / res_h
                        sides = [c3x - _D(k0), _D(k2) - c3x, c3y - _D(k1), _D(k3) - c3y]
                        keep = True
                        if any(e < 0 for e in sides):
                            keep = settings.clip_2d
                            sides = [_clip(e, _D(0.0), _D(1.0)) for e in sides]
                        if keep:
                            target, ignore = True, False
                            out["boxes"][b, i] = _D(c2x) / res_w, _D(c2y) / res_h, _D(s2w) / res_w, _D(s2h) / res_h
                            out["boxes_3d"][b, i] = [c3x, c3y] + sides
                            z = _F(_D(pz) * canonical_scale)
                            out["depth"][b, i, 0] = (_D(z) * crop_scale, _D(z) / crop_scale, z)[settings.depth_mode]
                            centre = _F(_F(x1 + x2) / _F(2))
                            hd = _wrap32(_wrap32(_F(_F(ry) - np.arctan2(_F(centre - P[2]), P[0]))))
                            two_pi = _F(2 * _PI)
                            hd = _mod(hd, two_pi)
                            shifted = _mod(_F(hd + _F(bin_size / 2)), two_pi)
                            q = _F(shifted / _F(bin_size))
                            k = int(q) if q == q else 0
                            out["heading_bin"][b, i, 0] = k
                            out["heading_res"][b, i, 0] = _F(shifted - _F(k * bin_size + bin_size / 2))
                            src = np.array([h, w, l], dtype=np.float32)
                            out["src_size_3d"][b, i] = src
                            out["size_3d"][b, i] = src.astype(np.float64) - settings.cls_mean_size[cls]
                            out["mask_2d"][b, i] = True
                            out["calibs"][b, i] = P.reshape(3, 4)
                            out["objects"][b, i] = [src[0], src[1], src[2], px, py, z, _F(ry)]
                if ignore:
                    fw, fh = _F(settings.resolution[0]), _F(settings.resolution[1])
                    a, c = _affine(t, x1, y1)
                    g0, g1 = _clip(_F(_F(a) / fw), _F(0), _F(1)), _clip(_F(_F(c) / fh), _F(0), _F(1))
                    a, c = _affine(t, x2, y2)
                    g2, g3 = _clip(_F(_F(a) / fw), _F(0), _F(1)), _clip(_F(_F(c) / fh), _F(0), _F(1))
                    if not (g2 <= g0 or g3 <= g1):
                        out["ignore_boxes"][b, packed] = g0, g1, g2, g3
                        out["ignore_mask"][b, packed] = True
                        packed += 1
            out["n_ignore"][b] = packed
    return out


# ================================================================================================ trainer.teacher
TEACHER_KEYS = ("refresh", "source", "per_step", "min_score", "weights", "start_epoch")
TeacherConfig = collections.namedtuple("TeacherConfig", TEACHER_KEYS)


def teacher_config(value, ema_on, threshold=None):
    """``trainer.teacher`` -> None (absent or None: off) or a ``TeacherConfig``; anything malformed is a ValueError.  ``ema_on``: whether
    ``trainer.ema_decay`` is set; ``threshold``: ``tester.threshold`` when the caller knows it (``min_score`` may not lie below it)."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError("trainer.teacher = %r is not a mapping (absent or None: off)" % (value,))
    unknown = sorted(set(value) - set(TEACHER_KEYS))
    if unknown:
        raise ValueError("trainer.teacher: unknown key(s) %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(TEACHER_KEYS)))

    def integer(key, default, least):
        v = value.get(key, default)
        if isinstance(v, bool) or not isinstance(v, int) or v < least:
            raise ValueError("trainer.teacher.%s = %r is not an integer >= %d" % (key, v, least))
        return v
    refresh, per_step, start_epoch = integer("refresh", 200, 1), integer("per_step", 1, 1), integer("start_epoch", 0, 0)
    source = value.get("source", "ema" if ema_on else "model")
    if source not in ("ema", "model") or not isinstance(source, str):
        raise ValueError("trainer.teacher.source = %r is neither 'ema' nor 'model'" % (source,))
    if source == "ema" and not ema_on:
        raise ValueError("trainer.teacher.source = 'ema' needs trainer.ema_decay: there is no averaged model to copy")
    if "min_score" not in value:
        raise ValueError("trainer.teacher.min_score is required: a number in [tester.threshold, 1]")
    low = 0.0 if threshold is None else float(threshold)
    m = value["min_score"]
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not (low <= float(m) <= 1.0):
        raise ValueError("trainer.teacher.min_score = %r is not a number in [tester.threshold = %r, 1]" % (m, low))
    weights = value.get("weights", "score")
    check_weights(weights)
    return TeacherConfig(refresh, source, per_step, float(m), weights, start_epoch)


class Teacher:
    """The mean teacher of ``trainer.teacher``: an eval-mode copy of the model that labels raw, un-augmented frames one cycle ahead of
    the student.

        teacher.refresh()            the copy := the source's weights (the EMA module, or the live model)
        teacher.submit(raw)          one collated unlabelled batch: teacher forward, decode, fuse and the target encode, enqueued
        staged = teacher.collect()   the oldest submitted batch as ``stage_batch`` would return it: (images, calibs, targets, info)

    ``raw`` is a batch of ``UnlabelledKITTI`` through ``collate_raw``: the uint8 canvas, P2, ``{"img_size"}`` and the student's ``info``
    (``prep``, ``affine``, ``scale_depth``, ``flip``, ``canonical_scale``).  The teacher looks at the frames without flip, crop or
    photometric step (``detector.frame_geometry``); behind decode and fuse, on the same stream, one ``mono_encode_targets_f64`` launch
    turns the rows into targets under the student's augmentation, and ``mask_2d``, ``label_weight`` and ``n_ignore`` go to the slot's
    pinned memory ahead of the slot's event.  ``collect`` waits on that event only and attaches the host copies, so that
    ``prepare_targets`` and the Trainer's box count need no synchronisation."""

    def __init__(self, cfg, model, device, source=None, loader=None):
        from .fuse import MAX_CANDIDATES, fuse_config
        from .helpers.save_helper import unwrap
        from .inference import InferenceEngine
        from .kitti_dataset import KITTI_Dataset
        import copy
        self.cfg = cfg
        self.device = torch.device(device)
        ema_on = bool(cfg["trainer"].get("ema_decay"))
        self.threshold = cfg["tester"].get("threshold", 0.2)
        self.config = teacher_config(cfg["trainer"].get("teacher"), ema_on, self.threshold)
        if self.config is None:
            raise ValueError("Teacher: trainer.teacher is absent from the configuration")
        if cfg["trainer"].get("label_audit"):
            raise ValueError("trainer.label_audit names every label by its label line: pseudo rows have none, so it cannot be "
                             "combined with trainer.teacher")
        self.dataset = KITTI_Dataset.settings(cfg["dataset"])
        if "ignore_classes" in cfg["dataset"]:       # the student's ignore_regions reading of it; encode_settings refuses a clash
            classes = cfg["dataset"]["ignore_classes"]
            if isinstance(classes, str) or not all(isinstance(c, str) for c in classes):
                raise ValueError("dataset.ignore_classes = %r is not a list of class names" % (classes,))
            self.dataset.ignore_classes = [c for c in classes if c not in self.dataset.writelist]
        self.settings = encode_settings(self.dataset, self.config.min_score, self.config.weights)      # aug_calib: ValueError
        if self.device.type == "cuda" and self.settings.max_objs > MAX_DEVICE_OBJS:
            raise ValueError("the encode kernel has one lane per slot and the host encode would need the rows on the host inside the "
                             "step: max_objs = %d > %d is not supported on a GPU" % (self.settings.max_objs, MAX_DEVICE_OBJS))
        self.topk = cfg["tester"]["topk"]
        self.fuse = fuse_config(cfg["tester"])
        views = 2 if self.fuse is not None and self.fuse[1] else 1
        if self.fuse is not None and views * self.topk > MAX_CANDIDATES:
            raise ValueError("trainer.teacher: %d view(s) x tester.topk = %d exceed the %d candidates the fuse kernel takes; the host "
                             "fuse leaves no rows on the device to encode" % (views, self.topk, MAX_CANDIDATES))
        self.live = unwrap(model)
        if self.device.type == "cuda":
            from .helpers.model_helper import to_mi355x_layout
            to_mi355x_layout(self.live)
        self.module = copy.deepcopy(self.live).eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
        self.source = source                         # a ModelEMA, or None: the live bare module
        self.loader, self._iterator = loader, None
        self.engine = InferenceEngine(self.module, self.device, topk=self.topk, max_objs=self.dataset.max_objs,
                                      in_flight=max(2, self.config.per_step),
                                      decode=(self.dataset.cls_mean_size, self.threshold), fuse=self.fuse)
        self._cms = torch.from_numpy(self.settings.cls_mean_size).to(self.device)
        self._pending = collections.deque()          # raw batches in submission order, beside the engine's queue
        self._done = collections.deque()             # batches the engine handed back before they were asked for
        self._epochs = 0                             # passes over the unlabelled loader begun
        self.refreshes = 0
        self.last_counts = (0, 0)                    # (targets, ignore boxes) of the batch collected last, from the pinned copies
        self.last_rows = None                        # (rows, count) that batch was encoded from: the engine's host copies
        # trainer.teacher_memory (monosowa_amd/teacher_memory.py): the rows are merged into the frame's remembered rows between fuse
        # and encode, and the encode reads the memory's rows.  Absent: nothing is built and every launch is what it is without it
        from .teacher_memory import MAX_ROWS, LabelMemory, memory_config
        self.memory_config = memory_config(cfg["trainer"].get("teacher_memory"), self.config.min_score, self.threshold,
                                           cfg["tester"].get("nms_iou"), self.dataset.max_objs)
        self.memory = None
        self.last_memory = None                      # (matched, created, missed, dropped, evicted, skipped) of the batch collected last
        if self.memory_config is not None:
            if views * self.topk > MAX_ROWS:
                raise ValueError("trainer.teacher_memory: %d view(s) x tester.topk = %d exceed the %d rows per image the merge takes"
                                 % (views, self.topk, MAX_ROWS))
            if self.loader is None:
                from .helpers.dataloader_helper import build_unlabelled_loader
                self.loader = build_unlabelled_loader(cfg["dataset"])
            m = self.memory_config
            self.memory = LabelMemory(self.loader.dataset.idx_list, m.slots, m.momentum, m.iou, m.drop_below, self.device)

    # ------------------------------------------------------------------------------------------------ weights
    def bind_source(self, ema):
        """The Trainer's ``ModelEMA`` (or None) once it exists: ``source: 'ema'`` copies from it, ``'model'`` from the live module."""
        if self.config.source == "ema":
            if ema is None:
                raise ValueError("trainer.teacher.source = 'ema' needs trainer.ema_decay: there is no averaged model to copy")
            self.source = ema
        else:
            self.source = None

    @torch.no_grad()
    def refresh(self):
        """The copy's parameters and buffers := the source's, by ``torch._foreach_copy_``; what the eval forward derives from them
        (folded weights, the engine's graphs) is dropped.  Call with nothing in flight."""
        from .ema import _invalidate_derived
        src = self.source.sync_untracked() if self.source is not None else self.live
        mine, theirs = list(self.module.parameters()), list(src.parameters())
        assert len(mine) == len(theirs)
        if mine:
            torch._foreach_copy_(mine, theirs)
        mine, theirs = list(self.module.buffers()), list(src.buffers())
        assert len(mine) == len(theirs)
        if mine:
            torch._foreach_copy_(mine, theirs)
        _invalidate_derived()
        self.engine.sync_weights()
        self.refreshes += 1

    # ------------------------------------------------------------------------------------------------ unlabelled frames
    def next_raw(self):
        """The next collated unlabelled batch; the loader is cycled endlessly (built from ``dataset.unlabelled_split`` on first use
        when none was given)."""
        if self.loader is None:
            from .helpers.dataloader_helper import build_unlabelled_loader
            self.loader = build_unlabelled_loader(self.cfg["dataset"])
        for _ in range(2):
            if self._iterator is None:
                sampler = getattr(self.loader, "sampler", None)
                if hasattr(sampler, "set_epoch"):
                    sampler.set_epoch(self._epochs)
                self._iterator = iter(self.loader)
                self._epochs += 1
            try:
                return next(self._iterator)
            except StopIteration:
                self._iterator = None
        raise ValueError("dataset.unlabelled_split yields no batch")

    # ------------------------------------------------------------------------------------------------ one batch
    def _teacher_view(self, calibs, img_size):
        """The teacher's own records and geometry rows: every frame as ``Detector`` sees it -- no flip, no crop, no photometric step."""
        from .detector import frame_geometry, geometry_row
        P2, sizes = calibs.numpy(), np.asarray(img_size)
        geos = [frame_geometry(sizes[i], P2[i], self.dataset) for i in range(len(P2))]
        prep = torch.from_numpy(np.stack([g["prep"] for g in geos]))
        geom = torch.from_numpy(np.stack([geometry_row(g) for g in geos]))
        height_crop = torch.from_numpy(np.array([g["height_crop"] for g in geos], dtype=np.float64))
        return prep, geom, height_crop

    def submit(self, raw):
        canvas, calibs, targets, info = raw
        img_size = targets["img_size"]
        prep, geom, height_crop = self._teacher_view(calibs, img_size)
        records = torch.from_numpy(student_records(calibs, img_size, info["flip"], info["affine"], info["scale_depth"],
                                                   info["canonical_scale"]))
        if self.device.type == "cuda":
            prep, geom, records = prep.pin_memory(), geom.pin_memory(), records.pin_memory()
        memory = self.memory
        frames = None if memory is None else memory.positions(info["img_id"])      # host lookup; pinned beside the records

        def after(rows, count, slot):
            stats = None
            if memory is not None:                                    # between fuse and encode: the encode reads the memory's rows
                if slot is None:
                    rows, count, stats = memory.merge_host(rows.contiguous(), count.to(torch.int32), frames)
                else:
                    rows, count, stats = memory.merge(rows, count, frames.to(self.device, non_blocking=True))
            if slot is None:                                          # the CPU device: the host function
                out = encode_targets_host(rows.numpy(), count.numpy(), records.numpy(), self.settings)
                out = {k: torch.from_numpy(v) for k, v in out.items()}
                host = {"targets": out, "mask_2d": out["mask_2d"], "label_weight": out["label_weight"], "n_ignore": out["n_ignore"]}
                return host if stats is None else dict(host, memory=stats)
            out = encode_targets(rows, count, records.to(self.device, non_blocking=True), self.settings._replace(cls_mean_size=self._cms))
            host = {}
            for k in ("mask_2d", "label_weight", "n_ignore"):
                host[k] = slot.pinned("teacher_" + k, out[k])
                host[k].copy_(out[k], non_blocking=True)
            if stats is not None:
                host["memory"] = slot.pinned("teacher_memory", stats)
                host["memory"].copy_(stats, non_blocking=True)
            return dict(host, targets=out)
        if self.device.type == "cuda":               # one upload: the engine's prepare now and collect()'s later read this copy
            canvas = canvas.to(self.device, non_blocking=True)
        self._pending.append((canvas, calibs, targets, info))
        done = self.engine.submit(canvas, calibs, img_size, height_crop, prep=prep, geom=geom, tag=len(self._pending), after=after)
        self._done.extend(done)

    def in_flight(self):
        return len(self._pending)

    def collect(self):
        """The oldest submitted batch, staged: waits on its slot's event only.  None with nothing submitted."""
        from .image_prep import prepare
        from .synthetic import attach_host_any, attach_host_mask, attach_host_weight
        if not self._pending:
            return None
        done = self._done.popleft() if self._done else self.engine.complete_oldest()
        canvas, calibs, targets, info = self._pending.popleft()
        extra = done.extra
        out = dict(extra["targets"])
        out.pop("n_ignore")
        out["img_size"] = targets["img_size"].to(self.device, non_blocking=True)
        attach_host_mask(out["mask_2d"], extra["mask_2d"])
        attach_host_weight(out["label_weight"], extra["label_weight"])
        attach_host_any(out["ignore_mask"], bool(np.asarray(extra["n_ignore"]).sum() > 0))
        self.last_counts = (int(np.count_nonzero(extra["mask_2d"])), int(np.asarray(extra["n_ignore"]).sum()))
        self.last_rows = (done.rows, done.count)     # the (fused) rows of this pass, host copies (with the memory on: what was merged)
        if self.memory is not None:
            self.last_memory = tuple(int(v) for v in np.asarray(extra["memory"]).reshape(-1, 6).sum(0))
        images = prepare(canvas, info["prep"], self.device)
        return images, calibs.to(self.device, non_blocking=True), out, info

    def close(self):
        """The end of training: the batches in flight are waited for and dropped, the engine's graphs freed, and the unlabelled
        loader's iterator (its worker processes) ended."""
        self._pending.clear()
        self._done.clear()
        self.engine.close()
        self._iterator = None
