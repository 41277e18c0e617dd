"""``monosowa_amd.Detector``: camera frames in, KITTI detections out -- no KITTI directory, no DataLoader, no text files.

    det = Detector(cfg, checkpoint=path)            # or Detector(cfg, model=m); cfg = the YAML dict
    det = Detector(cfg, checkpoint=path, weights="ema")     # the checkpoint's averaged weights (trainer.ema_decay)
    rows = det.detect(frames, P2, batch_size=16)    # frames: list of uint8 [h, w, 3] arrays (sizes may differ); P2: [N, 3, 4]
    for ids, rows in det.stream(batches): ...       # batches: an iterable of (frames, P2)
    det.write_kitti(rows, ids, directory)           # the files Tester.save_results writes

With ``tester.nms_iou`` (and ``tester.flip_tta`` / ``tester.fuse``) in the configuration the rows are suppressed / fused on the device
first (monosowa_amd/fuse.py); ``det.detect(frames, P2, support=True)`` also returns how many candidates each row stands for.

``rows[i]`` is float64 ``[n_i, 14]`` in ``decode_detections``' column order: cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry,
score.  Frames run on monosowa_amd/inference.py's ``InferenceEngine`` like ``Tester.inference``'s batches (image preparation,
graph-replayed forward and detection extraction on the GPU); the rows are decoded on the device as well
(``mono_decode_dets_f64``), so the host thread only pads frames into a canvas and slices results.

Per-frame quantities come from ``frame_geometry``: what ``KITTI_Dataset.__getitem__`` computes for a non-augmented sample, by the
dataset's own functions.  ``threshold`` / ``topk`` are read from ``cfg["tester"]`` and class names / ``cls_mean_size`` / canonical
focal length from ``cfg["dataset"]`` as the Tester and the dataset read them.
"""
import os

import numpy as np
import torch

from .fuse import fuse_config
from .helpers.save_helper import load_checkpoint, unwrap
from .image_prep import collate_raw, make_record
from .inference import InferenceEngine
from .kitti_dataset import Calibration, KITTI_Dataset, get_affine_transform
from .kitti_eval import GEOM_DOUBLES


def frame_geometry(size, P2, dataset):
    """One frame's ``info`` entries and camera, from its ``size`` (w, h), its 3 x 4 projection matrix and a dataset's settings
    (``KITTI_Dataset.settings(cfg["dataset"])`` or a dataset): kitti_dataset.py's ``__getitem__`` without augmentation -- centre
    = size / 2 and crop = size.  ``P2`` is taken in float32, as the calibration file's reader gives it.
    -> dict: img_size, height_crop, canonical_scale, prep (image_prep's record), calib (``Calibration``: cu cv fu fv tx ty P2)."""
    calib = Calibration({"P2": np.array(P2, dtype=np.float32).reshape(3, 4), "R0": None, "Tr_velo2cam": None})
    img_size = np.array((int(size[0]), int(size[1])))
    center = np.array(img_size) / 2
    crop_size, crop_scale = img_size, 1
    _, trans_inv = get_affine_transform(center, crop_size, 0, dataset.resolution, inv=1)
    fu, _, _, _, height_cropped = dataset.adjust_intrinsics(calib.fu, calib.fv, calib.cu, calib.cv, img_size, center, crop_scale,
                                                            crop_size, False)
    canonical_scale = dataset.canonical_focal_length / fu if dataset.use_canonical_module else 1.0
    return {"img_size": img_size, "height_crop": height_cropped, "canonical_scale": canonical_scale,
            "prep": make_record(img_size, trans_inv, False, None), "calib": calib}


def geometry_row(geo):
    """The float64 ``[GEOM_DOUBLES]`` row ``mono_decode_dets_f64`` reads for one frame (include/monosowa_kitti.h)."""
    c = geo["calib"]
    assert GEOM_DOUBLES == 10
    return np.array([geo["img_size"][0], geo["img_size"][1], geo["height_crop"], geo["canonical_scale"], c.cu, c.cv, c.fu, c.fv,
                     c.tx, c.ty], dtype=np.float64)


def check_frame(frame, index):
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.size == 0:
        what = "%s %s" % (frame.dtype, frame.shape) if isinstance(frame, np.ndarray) else type(frame).__name__
        raise ValueError("frame %d is not an 8-bit RGB image (uint8 [h, w, 3]), got %s" % (index, what))


class Detector:
    def __init__(self, cfg, checkpoint=None, model=None, device=None, weights=None):
        if (checkpoint is None) == (model is None):
            raise ValueError("Detector needs exactly one of checkpoint= and model=")
        if weights is not None and model is not None:
            raise ValueError("Detector: weights= selects what is loaded from checkpoint=; it cannot be combined with model=")
        if weights not in (None, "model", "ema"):
            raise ValueError("Detector: weights must be 'model' or 'ema', got %r" % (weights,))
        self.cfg = cfg
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        if model is None:
            from .helpers.model_helper import build_model, to_mi355x_layout
            model, _ = build_model(dict(cfg["model"], device=self.device.type))
            load_checkpoint(model=model, optimizer=None, filename=checkpoint, map_location=self.device, weights=weights or "model")
            model = model.to(self.device)
            if self.device.type == "cuda":
                model = to_mi355x_layout(model)
        # the bare module, as Tester takes it: a DistributedDataParallel forward would start collectives no other rank joins
        self.model = unwrap(model)
        self.dataset = KITTI_Dataset.settings(cfg["dataset"])
        self.class_name = self.dataset.class_name
        self.threshold = cfg["tester"].get("threshold", 0.2)
        self.topk = cfg["tester"]["topk"]
        # tester.nms_iou / flip_tta / fuse: duplicate suppression and flip-view fusion of the rows (monosowa_amd/fuse.py); None: off
        self.fuse = fuse_config(cfg["tester"])
        # tester.dontcare_below: rows scoring below it are written by write_kitti as DontCare lines; None: off
        from .helpers.tester_helper import check_dontcare_below
        self.dontcare_below = check_dontcare_below(cfg["tester"].get("dontcare_below"), self.threshold)
        self.engine = InferenceEngine(self.model, self.device, topk=self.topk, max_objs=self.dataset.max_objs,
                                      decode=(self.dataset.cls_mean_size, self.threshold), fuse=self.fuse)

    def _batch(self, frames, P2, first_id):
        """(frames, P2) -> what ``engine.submit`` takes: the raw canvas and default-collated info, as a ``device_aug`` loader's
        ``collate_raw`` makes them, plus the geometry rows of the device decode."""
        P2 = np.asarray(P2)
        if P2.ndim == 2:
            P2 = np.broadcast_to(P2, (len(frames), 3, 4))
        if P2.shape != (len(frames), 3, 4):
            raise ValueError("P2 must be [%d, 3, 4] (one matrix per frame) or [3, 4], got %s" % (len(frames), P2.shape))
        samples, geom = [], []
        for i, frame in enumerate(frames):
            check_frame(frame, first_id + i)
            geo = frame_geometry((frame.shape[1], frame.shape[0]), P2[i], self.dataset)
            geom.append(geometry_row(geo))
            info = {k: geo[k] for k in ("img_size", "height_crop", "canonical_scale", "prep")}
            samples.append((frame, geo["calib"].P2, 0, info))
        canvas, calibs, _, info = collate_raw(samples)
        geom = torch.from_numpy(np.stack(geom))
        if self.device.type == "cuda":
            canvas, info["prep"], geom = canvas.pin_memory(), info["prep"].pin_memory(), geom.pin_memory()
        return canvas, calibs, info, geom

    @torch.no_grad()
    def stream(self, batches):
        """``batches``: an iterable of ``(frames, P2)``, one engine batch each.  Yields ``(ids, rows)`` per batch in order, as the
        batches complete: ``ids`` are the frames' running indices, ``rows[i]`` float64 ``[n_i, 14]``.  The weights the model holds
        when the call starts are the ones used."""
        for done in self._completed(batches):
            yield done.tag, [done.rows[i, :done.count[i]] for i in range(len(done.tag))]

    @torch.no_grad()
    def _completed(self, batches):
        """``stream``'s loop: the engine's ``Completed`` batches in order, ``tag`` = the frames' running indices."""
        self.engine.sync_weights()
        n = 0
        try:
            for frames, P2 in batches:
                frames = list(frames)
                if not frames:
                    continue
                canvas, calibs, info, geom = self._batch(frames, P2, n)
                ids = list(range(n, n + len(frames)))
                n += len(frames)
                yield from self.engine.submit(canvas, calibs, info["img_size"], info["height_crop"], prep=info["prep"], geom=geom, tag=ids)
            yield from self.engine.drain()
        finally:
            self.engine.abandon()                       # left early (an exception, or the consumer stopped): nothing stays in flight

    def detect(self, frames, P2, batch_size=16, support=False):
        """All frames, ``batch_size`` at a time -> ``rows``: one float64 ``[n_i, 14]`` array per frame.  With the fuse keys set the
        rows are the fused ones; ``support=True`` -> ``(rows, support)``, ``support[i]`` int32 ``[n_i]``: how many candidates each
        row stands for (1 everywhere with the keys off)."""
        frames = list(frames)
        P2 = np.asarray(P2)
        if P2.ndim == 2:
            P2 = np.broadcast_to(P2, (len(frames), 3, 4))
        if P2.shape != (len(frames), 3, 4):
            raise ValueError("P2 must be [%d, 3, 4] (one matrix per frame) or [3, 4], got %s" % (len(frames), P2.shape))
        chunks = ((frames[i:i + batch_size], P2[i:i + batch_size]) for i in range(0, len(frames), int(batch_size)))
        out, members = [], []
        for done in self._completed(chunks):
            for i in range(len(done.tag)):
                out.append(done.rows[i, :done.count[i]])
                members.append(np.ones(done.count[i], dtype=np.int32) if done.support is None else done.support[i, :done.count[i]])
        return (out, members) if support else out

    def write_kitti(self, rows, ids, directory):
        """One KITTI result file per frame, ``%06d.txt`` of its id: the files ``Tester.save_results`` writes for these rows."""
        from .helpers.tester_helper import write_kitti_results
        write_kitti_results(dict(zip(ids, rows)), self.class_name, os.fspath(directory), dontcare_below=self.dontcare_below)

    def close(self):
        self.engine.close()
