"""The per-batch inference work of one model on one device (``Tester.inference`` and ``Detector`` both run on it).

    engine = InferenceEngine(model, device, topk=50)
    for batch in batches:
        for done in engine.submit(inputs, calibs, img_size, height_crop, prep=records, tag=batch_info):
            ...                                   # done.tag, done.dets [B, K, 37] (numpy), in submission order
    for done in engine.drain(): ...
    engine.close()

On a CUDA device a batch is: ``image_prep.prepare`` straight into the static input of a captured graph (or a copy of prepared
images), one graph replay of the eval forward, ``mono_extract_dets_f32`` (and, when the caller gives per-image geometry,
``mono_decode_dets_f64``, and with ``fuse=`` the duplicate suppression / flip-view fusion ``mono_fuse_dets_f64``) on the same stream,
a non-blocking copy into a pinned host slot, an event.  ``submit`` returns after
enqueueing; nothing synchronises the device: the consumer waits on the oldest slot's event only, and only when ``in_flight``
batches are already queued.  One graph per batch size seen, at most ``MAX_GRAPHS``; further batch sizes run eagerly.  A capture
that fails raises.  On a CPU device the same sequence runs eagerly inside ``submit``.  The device decides; there is no switch.

Model-only time is an event pair around each replay, read when the batch completes (``model_seconds`` / ``images``).
"""
import collections
import time

import numpy as np
import torch

from .helpers.decode_helper import decode_detections, extract_dets_from_outputs
from .fuse import MAX_CANDIDATES, fuse_rows_device, fuse_rows_host
from .image_prep import FLIP, RESOLUTION, is_raw_batch, prepare

MAX_GRAPHS = 3


class Completed:
    """One finished batch: ``tag`` as given to ``submit``; ``dets`` float32 ``[B, K, 37]``, or, for a batch submitted with
    geometry, ``rows`` float64 ``[B, K, 14]`` (kept rows first) and ``count`` int32 ``[B]``; on an engine with ``fuse=`` the rows
    are the fused ones, ``[B, V * K, 14]``, and ``support`` int32 ``[B, V * K]`` holds the members of each row's cluster.  Host arrays
    owned by the caller.  ``extra``: None, or for a batch submitted with ``after=`` the dict that hook returned, its tensors as host
    arrays."""
    __slots__ = ("tag", "dets", "rows", "count", "support", "extra")

    def __init__(self, tag, dets=None, rows=None, count=None, support=None, extra=None):
        self.tag, self.dets, self.rows, self.count, self.support, self.extra = tag, dets, rows, count, support, extra


class _Graph:
    """The eval forward of one batch shape, captured as ``GraphedForward`` captures it: eager warm-up on a side stream first
    (hipBLASLt's first-use timing and MSDA's per-geometry table fill happen outside capture), then the capture."""

    def __init__(self, model, images, calibs, img_sizes, warmup=2):
        self.images, self.calibs, self.img_sizes = images, calibs, img_sizes
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                model(self.images, self.calibs, None, self.img_sizes, dn_args=0)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.outputs = model(self.images, self.calibs, None, self.img_sizes, dn_args=0)

    def free(self):
        self.graph.reset()
        self.outputs = self.images = self.calibs = self.img_sizes = None


class _Slot:
    """Pinned host memory one in-flight batch lands in, its completion event and the event pair around its forward."""

    def __init__(self):
        self.buffers = {}
        self.done = torch.cuda.Event()
        self.start, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def pinned(self, name, like):
        buf = self.buffers.get(name)
        if buf is None or buf.shape[0] < like.shape[0] or buf.shape[1:] != like.shape[1:] or buf.dtype != like.dtype:
            buf = self.buffers[name] = torch.empty(like.shape, dtype=like.dtype, pin_memory=True)
        return buf[:like.shape[0]]


def weights_stamp(model):
    """What a captured forward was captured FROM: every parameter's and buffer's address and version, and the optimizer-step
    count (the raw-pointer AdamW steps without touching version counters; backbone.py keys its folded weights the same way)."""
    from .monodetr.backbone import _PARAM_EPOCH
    tensors = list(model.parameters()) + list(model.buffers())
    return (None if _PARAM_EPOCH is None else _PARAM_EPOCH[0], tuple((t.data_ptr(), t._version) for t in tensors))


class InferenceEngine:
    def __init__(self, model, device, topk=50, max_objs=50, in_flight=2, decode=None, fuse=None):
        """``decode``: ``(cls_mean_size [C, 3], threshold)`` for batches submitted with ``geom`` (rows instead of detections).
        ``fuse``: ``(iou, flip_tta, mode)`` as ``fuse.fuse_config`` returns it -- every batch then comes with ``geom`` and its rows
        are fused (monosowa_amd/fuse.py); with ``flip_tta`` the mirrored frames run in the same forward, as a second half of the
        batch prepared from the same canvas with the records' FLIP bit toggled."""
        self.model = model.eval()
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.topk, self.max_objs, self.in_flight = int(topk), int(max_objs), int(in_flight)
        assert self.in_flight >= 1
        self.decode = None
        if decode is not None:
            cms = torch.from_numpy(np.ascontiguousarray(decode[0], dtype=np.float64))
            self.decode = (cms.to(self.device), float(decode[1]))
        self.fuse = None
        if fuse is not None:
            if self.decode is None:
                raise ValueError("InferenceEngine(fuse=...) needs decode=(cls_mean_size, threshold): rows are what is fused")
            self.fuse = (float(fuse[0]), bool(fuse[1]), fuse[2])
        self.graphs = collections.OrderedDict()              # (images shape, dtypes) -> _Graph
        self.stamp = None
        self.queue = collections.deque()                     # CUDA: (slot, tag, B, kind) in submission order; CPU: Completed
        self.free_slots = [_Slot() for _ in range(self.in_flight)] if self.cuda else []
        self.error = None
        self.model_seconds, self.images = 0.0, 0
        self.replays = self.eager_forwards = 0

    # ------------------------------------------------------------------------------------------------ the public calls
    def submit(self, inputs, calibs, img_size, height_crop, prep=None, geom=None, tag=None, after=None):
        """Enqueues one batch and returns the batches that have completed, oldest first (possibly none).  ``inputs``: a raw
        batch as ``collate_raw`` makes it (uint8 canvas; ``prep`` = its records) or prepared float32 images; ``calibs``
        ``[B, 3, 4]``; ``img_size`` ``[B, 2]`` and ``height_crop`` ``[B]`` as the loader's ``info`` carries them; ``geom``: float64
        ``[B, 10]`` per-image geometry (kitti_eval.GEOM_DOUBLES) to have the rows decoded on the device.
        ``after(rows, count, slot)`` (a batch with ``geom`` only): called once, behind the decode (and the fuse) and before the batch's
        completion event is recorded, with the device rows -- the fused ones on an engine that fuses -- and the batch's ``_Slot``
        (None on a CPU device).  It may enqueue launches on the current stream and copy into ``slot.pinned(name, like)`` buffers (names
        of its own); the dict it returns comes back as ``Completed.extra``, tensors in it as host arrays.  Without it every launch
        and byte is what it is without the argument."""
        self._raise_pending()
        done = []
        while len(self.queue) >= self.in_flight:                         # bounded: the oldest batch's event, nothing wider
            done.append(self._complete())
        try:
            if self.cuda:
                self._enqueue(inputs, calibs, img_size, height_crop, prep, geom, tag, after)
            else:
                self.queue.append(self._run_on_host(inputs, calibs, img_size, height_crop, prep, geom, tag, after))
        except Exception as e:               # the batches already in flight are delivered first; this surfaces at the next call
            self.error = e
        while self.queue and self._ready(self.queue[0]):
            done.append(self._complete())
        return done

    def drain(self):
        """The batches still in flight, oldest first.  Raises what a failed ``submit`` left behind first (the batches enqueued
        before it stay in flight: a second ``drain()`` returns them)."""
        self._raise_pending()
        done = []
        while self.queue:
            done.append(self._complete())
        return done

    def complete_oldest(self):
        """The oldest batch in flight, waited for on its own event (None with nothing in flight); a failed ``submit`` raises first."""
        self._raise_pending()
        return self._complete() if self.queue else None

    def sync_weights(self):
        """Drops the captured graphs when the model's weights are no longer the ones they were captured from (optimizer steps,
        ``load_state_dict``, ``.to()``): the eval forward derives tensors from parameters (folded convolution weights) outside
        the graph's reach, so the next batch recaptures.  Call between passes, with nothing in flight."""
        assert not self.queue, "sync_weights() with batches in flight"
        self.model.eval()
        if self.graphs and weights_stamp(self.model) != self.stamp:
            self._free_graphs()

    def abandon(self):
        """Waits for the batches in flight and drops them (a consumer that stops early); a pending error stays pending."""
        while self.queue:
            self._complete()

    def close(self):
        """Frees the graphs and returns their memory pools; batches still in flight are waited for and dropped."""
        self.abandon()
        self._free_graphs()
        for slot in self.free_slots:
            slot.buffers.clear()
        if self.cuda:
            torch.cuda.empty_cache()

    # ------------------------------------------------------------------------------------------------ internals
    def _raise_pending(self):
        if self.error is not None:
            e, self.error = self.error, None
            raise e

    def _free_graphs(self):
        for g in self.graphs.values():
            g.free()
        self.graphs.clear()
        self.stamp = None

    def _img_sizes(self, img_size, height_crop):
        img_sizes = img_size.to(self.device).clone()                     # Tester.inference's expression, its integer assignment included
        img_sizes[:, 1] = img_sizes[:, 1] / height_crop.to(self.device)
        return img_sizes

    def _ready(self, item):
        return not self.cuda or item[0].done.query()

    def _complete(self):
        item = self.queue.popleft()
        if not self.cuda:
            return item
        slot, tag, B, geom, extra = item
        try:
            slot.done.synchronize()
            self.model_seconds += slot.start.elapsed_time(slot.end) * 1e-3
            self.images += B
            if extra is not None:
                done = Completed(tag, rows=slot.buffers["rows"][:B].numpy().copy(), count=slot.buffers["count"][:B].numpy().copy(),
                                 extra=_host_copies(extra))
                if geom == "fused":
                    done.support = slot.buffers["support"][:B].numpy().copy()
                return done
            if geom == "fused":
                return Completed(tag, rows=slot.buffers["rows"][:B].numpy().copy(), count=slot.buffers["count"][:B].numpy().copy(),
                                 support=slot.buffers["support"][:B].numpy().copy())
            if geom == "fuse on the host":                                # more candidates than the kernel takes
                views = 2 if self.fuse[1] else 1
                rows, count, support = fuse_rows_host(slot.buffers["rows"][:views * B].numpy(), slot.buffers["count"][:views * B].numpy(),
                                                      slot.buffers["geom"][:B].numpy(), self.fuse[0], self.fuse[2], views)
                return Completed(tag, rows=rows, count=count, support=support)
            if geom:
                return Completed(tag, rows=slot.buffers["rows"][:B].numpy().copy(), count=slot.buffers["count"][:B].numpy().copy())
            return Completed(tag, dets=slot.buffers["dets"][:B].numpy().copy())
        finally:
            self.free_slots.append(slot)

    def _forward_with_flip(self, inputs, prep, calibs, img_sizes, slot):
        """``_forward`` of 2 B images: the frames, then the same frames mirrored -- the canvas goes to the device once and is
        prepared twice, the second time with every record's FLIP bit toggled (flags + 1 - 2 (flags mod 2), on the device)."""
        B = inputs.shape[0]
        shape = (2 * B, 3, RESOLUTION[1], RESOLUTION[0])
        key = (shape, calibs.dtype, img_sizes.dtype, "flip")
        g = self.graphs.get(key)
        eager = g is None and len(self.graphs) >= MAX_GRAPHS
        images = g.images if g is not None else \
            torch.empty(shape, dtype=torch.float32, device=self.device).contiguous(memory_format=torch.channels_last)
        canvas = inputs.to(self.device, non_blocking=True)
        records = prep.to(self.device, non_blocking=True)
        mirrored = records.clone()
        mirrored[:, 8] = records[:, 8] + 1 - 2 * torch.remainder(records[:, 8], 2)
        assert FLIP == 1
        prepare(canvas, records, self.device, out=images[:B])
        prepare(canvas, mirrored, self.device, out=images[B:])
        calibs, img_sizes = torch.cat([calibs, calibs]), torch.cat([img_sizes, img_sizes])
        if eager:
            slot.start.record()
            with torch.no_grad():
                outputs = self.model(images, calibs, None, img_sizes, dn_args=0)
            slot.end.record()
            self.eager_forwards += 1
            return outputs
        if g is None:
            if not self.graphs:
                self.stamp = weights_stamp(self.model)
            g = self.graphs[key] = _Graph(self.model, images, calibs, img_sizes)
        else:
            g.calibs.copy_(calibs, non_blocking=True)
            g.img_sizes.copy_(img_sizes, non_blocking=True)
        slot.start.record()
        g.graph.replay()
        slot.end.record()
        self.replays += 1
        return g.outputs

    def _forward(self, inputs, prep, calibs, img_sizes, slot):
        """The eval forward on the current stream: graph replay for a cached (or cacheable) batch shape, eager otherwise."""
        raw = is_raw_batch(inputs)
        B = inputs.shape[0]
        shape = (B, 3, RESOLUTION[1], RESOLUTION[0]) if raw else tuple(inputs.shape)
        key = (shape, calibs.dtype, img_sizes.dtype)
        g = self.graphs.get(key)
        if g is None and len(self.graphs) >= MAX_GRAPHS:
            images = prepare(inputs, prep, self.device) if raw else inputs.to(self.device, non_blocking=True)
            slot.start.record()
            with torch.no_grad():
                outputs = self.model(images, calibs, None, img_sizes, dn_args=0)
            slot.end.record()
            self.eager_forwards += 1
            return outputs
        if g is None:
            images = torch.empty(shape, dtype=torch.float32, device=self.device).contiguous(memory_format=torch.channels_last) if raw \
                else torch.empty_like(inputs, device=self.device)
        else:
            images = g.images
        if raw:
            prepare(inputs, prep, self.device, out=images)
        else:
            images.copy_(inputs, non_blocking=True)
        if g is None:                                                     # first batch of this shape: warm up and capture on its data
            if not self.graphs:
                self.stamp = weights_stamp(self.model)
            g = self.graphs[key] = _Graph(self.model, images, calibs.clone(), img_sizes.clone())
        else:
            g.calibs.copy_(calibs, non_blocking=True)
            g.img_sizes.copy_(img_sizes, non_blocking=True)
        slot.start.record()
        g.graph.replay()
        slot.end.record()
        self.replays += 1
        return g.outputs

    def _enqueue(self, inputs, calibs, img_size, height_crop, prep, geom, tag, after=None):
        if geom is not None and self.decode is None:
            raise ValueError("a batch with geometry needs InferenceEngine(decode=(cls_mean_size, threshold))")
        _check_after(after, geom)
        extra = None
        self._check_fuse(inputs, geom)
        flip = self.fuse is not None and self.fuse[1]
        kind = geom is not None
        slot = self.free_slots.pop()
        try:
            calibs_dev = calibs.to(self.device, non_blocking=True)
            img_sizes = self._img_sizes(img_size, height_crop)
            outputs = (self._forward_with_flip if flip else self._forward)(inputs, prep, calibs_dev, img_sizes, slot)
            dets = extract_dets_from_outputs(outputs=outputs, K=self.max_objs, topk=self.topk)
            if geom is not None:
                from .kitti_eval import decode_dets_device
                geom_dev = geom.to(self.device, non_blocking=True)
                rows, count = decode_dets_device(dets.contiguous(), torch.cat([geom_dev, geom_dev]) if flip else geom_dev, *self.decode)
                support = None
                if self.fuse is not None:
                    views = 2 if flip else 1
                    if views * rows.shape[1] <= MAX_CANDIDATES:
                        rows, count, support = fuse_rows_device(rows, count, geom_dev, self.fuse[0], self.fuse[2], views)
                        kind = "fused"
                    else:                                                 # fused in _complete, from the unfused rows
                        slot.pinned("geom", geom_dev).copy_(geom_dev, non_blocking=True)
                        kind = "fuse on the host"
                slot.pinned("rows", rows).copy_(rows, non_blocking=True)
                slot.pinned("count", count).copy_(count, non_blocking=True)
                if support is not None:
                    slot.pinned("support", support).copy_(support, non_blocking=True)
                if after is not None:
                    if kind == "fuse on the host":
                        raise ValueError("after= needs the fused rows on the device: more than %d candidates per image are fused on "
                                         "the host" % MAX_CANDIDATES)
                    extra = after(rows, count, slot)
                    extra = {} if extra is None else extra
            else:
                slot.pinned("dets", dets).copy_(dets, non_blocking=True)
            slot.done.record()
        except Exception:
            self.free_slots.append(slot)
            raise
        self.queue.append((slot, tag, inputs.shape[0], kind, extra))

    def _check_fuse(self, inputs, geom):
        if self.fuse is None:
            return
        if geom is None:
            raise ValueError("InferenceEngine(fuse=...): every batch must come with geom")
        if self.fuse[1] and not is_raw_batch(inputs):
            raise ValueError("tester.flip_tta mirrors raw frames (dataset.device_aug / the Detector); prepared float32 images cannot be mirrored")

    def _run_on_host(self, inputs, calibs, img_size, height_crop, prep, geom, tag, after=None):
        if geom is not None and self.decode is None:
            raise ValueError("a batch with geometry needs InferenceEngine(decode=(cls_mean_size, threshold))")
        _check_after(after, geom)
        self._check_fuse(inputs, geom)
        images = prepare(inputs, prep, self.device) if is_raw_batch(inputs) else inputs.to(self.device)
        img_sizes = self._img_sizes(img_size, height_crop)
        flip = self.fuse is not None and self.fuse[1]
        if flip:
            mirrored = prep.clone()
            mirrored[:, 8] = prep[:, 8] + 1 - 2 * torch.remainder(prep[:, 8], 2)
            images = torch.cat([images, prepare(inputs, mirrored, self.device)])
            calibs, img_sizes, geom = torch.cat([calibs, calibs]), torch.cat([img_sizes, img_sizes]), torch.cat([geom, geom])
        t0 = time.time()
        with torch.no_grad():
            outputs = self.model(images, calibs.to(self.device), None, img_sizes, dn_args=0)
        self.model_seconds += time.time() - t0
        self.images += inputs.shape[0]
        self.eager_forwards += 1
        dets = extract_dets_from_outputs(outputs=outputs, K=self.max_objs, topk=self.topk).cpu().numpy()
        if geom is None:
            return Completed(tag, dets=dets)
        rows, count = decode_rows_host(dets, geom.numpy(), self.decode[0].numpy(), self.decode[1])
        support = None
        if self.fuse is not None:
            rows, count, support = fuse_rows_host(rows, count, geom.numpy()[:inputs.shape[0]], self.fuse[0], self.fuse[2], 2 if flip else 1)
        done = Completed(tag, rows=rows, count=count, support=support)
        if after is not None:
            extra = after(torch.from_numpy(rows), torch.from_numpy(count), None)
            done.extra = _host_copies({} if extra is None else extra)
        return done


def _check_after(after, geom):
    if after is not None and geom is None:
        raise ValueError("after= is called with the decoded rows: the batch must come with geom")


def _host_copies(extra):
    """``Completed.extra`` of an ``after=`` hook's dict: host tensors (the slot's pinned buffers) as arrays of the caller's own,
    everything else as it is."""
    return {k: (v.numpy().copy() if isinstance(v, torch.Tensor) and not v.is_cuda else v) for k, v in extra.items()}


class _Camera:
    __slots__ = ("cu", "cv", "fu", "fv", "tx", "ty")


def decode_rows_host(dets, geom, cls_mean_size, threshold):
    """``mono_decode_dets_f64``'s contract through ``decode_detections`` (the CPU device's path): rows ``[B, K, 14]`` with the
    kept rows first and the rest zero, count ``[B]``."""
    B, K, _ = dets.shape
    cams = []
    for g in geom:
        c = _Camera()
        c.cu, c.cv, c.fu, c.fv, c.tx, c.ty = g[4:10]
        cams.append(c)
    info = {"img_size": geom[:, 0:2], "height_crop": geom[:, 2], "canonical_scale": geom[:, 3], "img_id": list(range(B))}
    res = decode_detections(dets, info, cams, cls_mean_size, threshold)
    rows, count = np.zeros((B, K, 14), dtype=np.float64), np.zeros(B, dtype=np.int32)
    for i in range(B):
        count[i] = len(res[i])
        if res[i]:
            rows[i, :count[i]] = np.asarray(res[i], dtype=np.float64)
    return rows, count
