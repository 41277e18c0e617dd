"""The label memory of self-training (``trainer.teacher_memory``): the teacher's rows matched and smoothed across passes.

    config = memory_config(value, min_score, threshold, nms_iou, max_objs)      None (off) or a checked ``MemoryConfig``
    memory = LabelMemory(ids, slots, momentum, iou, drop_below, device)
    out_rows, out_count, stats = memory.merge(rows, count, frames)      one launch of mono_memory_merge_f64 on the current stream
    out_rows, out_count, stats = memory.merge_host(rows, count, frames) the same contract in numpy scalars (a CPU device)
    frames = memory.positions(img_ids)                                   host lookup -> pinned int32 [B]
    memory.state_dict() / memory.load_state_dict(state)

The rule (include/monosowa_kitti.h has it in full).  Per frame the bank holds up to ``slots`` entries of 16 doubles: a KITTI row whose
column 13 is the smoothed score, ``hits`` and ``misses``.  A pass's rows -- in the raw frame's coordinates, which no augmentation of
the student touches -- are matched in row order against the frame's entries by class and the evaluation's BEV overlap, each row
claiming the lowest unclaimed entry it overlaps by ``iou``.  A claimed entry takes the row's geometry and moves its score towards
the row's, ``s += (1 - momentum) * (s_row - s)``; an entry nothing claimed moves towards 0; an unmatched row becomes an entry.  What
falls below ``drop_below`` is dropped, the rest is ordered by score, the first ``slots`` stay.  The merged rows are what the target
encode reads, so a remembered object that is not seen this pass decays through the ignore band ``[drop_below, min_score)`` before
it disappears, instead of being trained as background at once.

Limits.  Not under DDP: the frames a rank sees change from pass to pass and the exchange between ranks is not built.  The memory
is only as good as the teacher's geometry; columns 0..12 follow the newest match, no geometry is averaged.  Rows with a score that
is not finite take no part.  With ``tester.fuse: 'mean'`` rows do not arrive in score order, so the slot order of the first pass
differs from a run without the key; the set of targets does not.
"""
import collections
import logging
import math

import numpy as np
import torch

ENTRY = 16                     # doubles per entry: a 14-column row, hits, misses
ROW = 14
MAX_SLOTS = 64                 # one lane per entry (csrc/memory_merge.h)
MAX_ROWS = 256
STATS = ("matched", "created", "missed", "dropped", "evicted", "skipped")
MEMORY_KEYS = ("momentum", "iou", "drop_below", "slots")
MemoryConfig = collections.namedtuple("MemoryConfig", MEMORY_KEYS)


def _number(key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
        raise ValueError("trainer.teacher_memory.%s = %r is not a number" % (key, v))
    return float(v)


def memory_config(value, min_score, threshold=None, nms_iou=None, max_objs=50):
    """``trainer.teacher_memory`` -> None (absent or None: off) or a ``MemoryConfig``; anything malformed is a ValueError.
    ``min_score``: ``trainer.teacher.min_score``, None when ``trainer.teacher`` is off; ``threshold`` / ``nms_iou``: the tester's keys
    (defaults of ``drop_below`` / ``iou``); ``max_objs``: the dataset's (default of ``slots``)."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError("trainer.teacher_memory = %r is not a mapping (absent or None: off)" % (value,))
    unknown = sorted(set(value) - set(MEMORY_KEYS), key=repr)
    if unknown:
        raise ValueError("trainer.teacher_memory: unknown key(s) %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(MEMORY_KEYS)))
    if min_score is None:
        raise ValueError("trainer.teacher_memory needs trainer.teacher: it remembers the teacher's rows")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise ValueError("trainer.teacher_memory is not supported with more than one rank: the frames a rank sees change from pass "
                         "to pass and the exchange of memories between ranks is not built")
    momentum = _number("momentum", value.get("momentum", 0.5))
    if not 0.0 < momentum < 1.0:
        raise ValueError("trainer.teacher_memory.momentum = %r is not a number inside (0, 1)" % (value.get("momentum"),))
    iou = _number("iou", value.get("iou", nms_iou if nms_iou else 0.5))
    if not 0.0 < iou <= 1.0:
        raise ValueError("trainer.teacher_memory.iou = %r is not a number in (0, 1]" % (value.get("iou"),))
    drop = _number("drop_below", value.get("drop_below", 0.2 if threshold is None else threshold))
    if not 0.0 <= drop <= float(min_score):
        raise ValueError("trainer.teacher_memory.drop_below = %r is not a number in [0, trainer.teacher.min_score = %r]"
                         % (drop, min_score))
    slots = value.get("slots", min(int(max_objs), MAX_SLOTS))
    if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= MAX_SLOTS:
        raise ValueError("trainer.teacher_memory.slots = %r is not an integer in [1, %d]" % (slots, MAX_SLOTS))
    return MemoryConfig(momentum, iou, drop, slots)


def _flag(row_box, entry_box, thr):
    """The overlap test of the rule on two float32 rectangles (as float64 values): ``fuse.fuse_rows_host``'s own function."""
    from .fuse import bev_iou
    return bool(np.float32(bev_iou(row_box, entry_box)) >= thr)       # NaN (not finite, no area): never


def merge_rows_host(rows, count, frames, bank, bank_count, momentum, iou, drop_below):
    """``mono_memory_merge_f64``'s contract in numpy scalars.  ``bank`` float64 ``[N, M, 16]`` and ``bank_count`` int32 ``[N]`` are
    updated in place -> (out_rows ``[B, M, 14]``, out_count int32 ``[B]``, stats int32 ``[B, 6]``)."""
    rows, count, frames = np.asarray(rows, dtype=np.float64), np.asarray(count), np.asarray(frames)
    B, R, _ = rows.shape
    N, M, _ = bank.shape
    if not (1 <= M <= MAX_SLOTS and 1 <= R <= MAX_ROWS and 0.0 < iou <= 1.0 and 0.0 < momentum < 1.0):
        raise ValueError("merge: slots %d, rows %d, iou %r or momentum %r outside the contract" % (M, R, iou, momentum))
    out_rows = np.zeros((B, M, ROW), dtype=np.float64)
    out_count, stats = np.zeros(B, dtype=np.int32), np.zeros((B, len(STATS)), dtype=np.int32)
    w, thr, bev = np.float64(1.0) - np.float64(momentum), np.float32(iou), [9, 11, 8, 7, 12]
    with np.errstate(all="ignore"):
        for b in range(B):
            f = int(frames[b])
            if f < 0 or f >= N:
                continue
            n, k = int(min(max(count[b], 0), R)), int(min(max(bank_count[f], 0), M))
            new, old = rows[b, :n], bank[f, :k].copy()
            new_box = new[:, bev].astype(np.float32).astype(np.float64)
            old_box = old[:, bev].astype(np.float32).astype(np.float64)
            claimer, unmatched, skipped = [-1] * k, [], 0
            for i in range(n):
                if not np.isfinite(new[i, 13]):
                    skipped += 1
                    continue
                for e in range(k):
                    if claimer[e] < 0 and new[i, 0] == old[e, 0] and _flag(new_box[i], old_box[e], thr):
                        claimer[e] = i
                        break
                else:
                    unmatched.append(i)
            cands = []                                        # entries of 16 doubles: the old ones in slot order, then the new rows
            for e in range(k):
                entry, i = old[e].copy(), claimer[e]
                s = entry[13]
                d = (new[i, 13] if i >= 0 else np.float64(0.0)) - s
                t = w * d
                entry[13] = s + t
                if i >= 0:
                    entry[:13] = new[i, :13]
                    entry[14], entry[15] = entry[14] + 1.0, 0.0
                else:
                    entry[15] = entry[15] + 1.0
                cands.append(entry)
            for i in unmatched:
                entry = np.zeros(ENTRY, dtype=np.float64)
                entry[:ROW] = new[i]
                entry[14] = 1.0
                cands.append(entry)
            alive = [c for c in cands if c[13] >= drop_below]
            alive.sort(key=lambda c: -c[13])                  # stable: ties keep old before new, each in their own order
            kept = alive[:M]
            bank[f] = 0.0
            for r, c in enumerate(kept):
                bank[f, r] = c
                out_rows[b, r] = c[:ROW]
            bank_count[f] = out_count[b] = len(kept)
            matched = sum(1 for i in claimer if i >= 0)
            stats[b] = (matched, len(unmatched), k - matched, len(cands) - len(alive), len(alive) - len(kept), skipped)
    return out_rows, out_count, stats


class LabelMemory:
    """The bank of ``trainer.teacher_memory``: per frame of ``ids`` (the names of ``ImageSets/NAME.txt`` in file order) up to
    ``slots`` remembered rows, on ``device``, allocated once."""

    def __init__(self, ids, slots, momentum, iou, drop_below, device):
        self.ids = [int(i) for i in ids]
        self.index = {}
        for position, i in enumerate(self.ids):
            if i in self.index:
                raise ValueError("LabelMemory: frame %r is listed twice" % (i,))
            self.index[i] = position
        if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= MAX_SLOTS:
            raise ValueError("LabelMemory: slots = %r is not an integer in [1, %d]" % (slots, MAX_SLOTS))
        if not 0.0 < float(momentum) < 1.0 or not 0.0 < float(iou) <= 1.0 or math.isnan(float(drop_below)):
            raise ValueError("LabelMemory: momentum %r must lie inside (0, 1), iou %r in (0, 1], drop_below %r be a number"
                             % (momentum, iou, drop_below))
        self.slots, self.momentum, self.iou, self.drop_below = slots, float(momentum), float(iou), float(drop_below)
        self.device = torch.device(device)
        self.bank = torch.zeros((len(self.ids), slots, ENTRY), dtype=torch.float64, device=self.device)
        self.count = torch.zeros((len(self.ids),), dtype=torch.int32, device=self.device)

    def positions(self, img_ids):
        """Frame names of one batch -> their positions, int32 ``[B]`` (pinned where a GPU is there to read it).  KeyError for a name
        the memory does not know, ValueError for one named twice: one workgroup owns one frame's block."""
        names = [int(i) for i in (img_ids.tolist() if hasattr(img_ids, "tolist") else img_ids)]
        if len(set(names)) != len(names):
            raise ValueError("LabelMemory: a frame is named twice in one batch: %r" % (names,))
        out = torch.empty((len(names),), dtype=torch.int32, pin_memory=self.device.type == "cuda")
        for b, i in enumerate(names):
            if i not in self.index:
                raise KeyError("LabelMemory: frame %r is not in the memory's split" % (i,))
            out[b] = self.index[i]
        return out

    def _check(self, rows, count, frames, cuda):
        if rows.dim() != 3 or rows.shape[2] != ROW or rows.dtype != torch.float64 or rows.is_cuda != cuda or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous float64 %s tensor [B, R, 14], got %s %s"
                             % ("CUDA" if cuda else "CPU", rows.dtype, tuple(rows.shape)))
        B, R, _ = rows.shape
        if not 1 <= R <= MAX_ROWS:
            raise ValueError("the merge takes 1 to %d rows per image, got %d" % (MAX_ROWS, R))
        for name, t in (("count", count), ("frames", frames)):
            if t.dtype != torch.int32 or tuple(t.shape) != (B,) or t.device != rows.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous torch.int32 tensor %s on %s, got %s %s on %s"
                                 % (name, (B,), rows.device, t.dtype, tuple(t.shape), t.device))
        if rows.device != self.bank.device:
            raise ValueError("rows live on %s, the memory on %s" % (rows.device, self.bank.device))
        return B, R

    def merge(self, rows, count, frames, out=None):
        """One launch of ``mono_memory_merge_f64`` on the current stream: rows float64 ``[B, R, 14]``, count and frames int32 ``[B]``
        (contiguous CUDA tensors; the frames distinct) -> (out_rows ``[B, slots, 14]``, out_count int32 ``[B]``, stats int32
        ``[B, 6]``); ``out``: such a triple to write into.  Whether the frames are distinct is checked where it costs no
        synchronisation: by ``positions``, or here for a host tensor."""
        from .kitti_eval import load
        if not frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 1:
            if len(set(frames.tolist())) != frames.shape[0]:
                raise ValueError("LabelMemory: a frame is named twice in one batch: %r" % (frames.tolist(),))
            frames = frames.to(self.device, non_blocking=True)
        B, R = self._check(rows, count, frames, True)
        M = self.slots
        if out is None:
            out = (torch.empty((B, M, ROW), dtype=torch.float64, device=rows.device),
                   torch.empty((B,), dtype=torch.int32, device=rows.device),
                   torch.empty((B, len(STATS)), dtype=torch.int32, device=rows.device))
        for name, t, dtype, shape in (("out_rows", out[0], torch.float64, (B, M, ROW)), ("out_count", out[1], torch.int32, (B,)),
                                      ("stats", out[2], torch.int32, (B, len(STATS)))):
            if t.dtype != dtype or tuple(t.shape) != shape or t.device != rows.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s tensor %s on %s" % (name, dtype, shape, rows.device))
        with torch.cuda.device(rows.device):
            code = load().mono_memory_merge_f64(rows.data_ptr(), count.data_ptr(), frames.data_ptr(), self.bank.data_ptr(),
                                                self.count.data_ptr(), self.momentum, self.iou, self.drop_below, out[0].data_ptr(),
                                                out[1].data_ptr(), out[2].data_ptr(), B, R, len(self.ids), M,
                                                torch.cuda.current_stream().cuda_stream)
        if code:
            raise RuntimeError("mono_memory_merge_f64 failed with code %d" % code)
        return out

    def merge_host(self, rows, count, frames):
        """``merge`` for a memory on a CPU device: CPU tensors in, CPU tensors out, the bank updated in place."""
        if self.device.type != "cpu":
            raise ValueError("merge_host runs on a CPU memory; this one lives on %s" % self.device)
        self._check(rows, count, frames, False)
        if len(set(frames.tolist())) != frames.shape[0]:
            raise ValueError("LabelMemory: a frame is named twice in one batch: %r" % (frames.tolist(),))
        got = merge_rows_host(rows.numpy(), count.numpy(), frames.numpy(), self.bank.numpy(), self.count.numpy(), self.momentum,
                              self.iou, self.drop_below)
        return tuple(torch.from_numpy(a) for a in got)

    def state_dict(self):
        """The memory as CPU tensors: a synchronisation; the caller saves where it waits anyway."""
        return {"ids": torch.tensor(self.ids, dtype=torch.int64), "slots": self.slots, "bank": self.bank.cpu().clone(),
                "count": self.count.cpu().clone(), "momentum": self.momentum, "iou": self.iou, "drop_below": self.drop_below}

    def load_state_dict(self, state, logger=None):
        """Restores bank and counts in place when ``ids`` and ``slots`` are this memory's; otherwise (or with ``state`` None) one
        warning, and the memory starts empty.  The settings stay the configuration's."""
        ids = None if state is None else [int(i) for i in torch.as_tensor(state["ids"]).tolist()]
        if state is None or ids != self.ids or int(state["slots"]) != self.slots:
            (logger or logging.getLogger(__name__)).warning(
                "teacher_memory: the checkpoint holds %s; the label memory starts empty",
                "no 'teacher_memory'" if state is None else "a memory of other frames or slots")
            self.bank.zero_()
            self.count.zero_()
            return False
        self.bank.copy_(state["bank"])
        self.count.copy_(state["count"])
        return True
