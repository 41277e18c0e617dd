"""Set-prediction criterion of MonoDETR (reference: lib/models/monodetr/monodetr.py --
``SetCriterion.__init__`` :308-340, losses :396-575, index helpers :1159-1169, ``get_loss``
:1171-1186, ``forward`` :1188-1230).

Loss dict keys and normalisation are the reference's: loss_ce, loss_bbox, loss_giou, loss_center,
loss_depth, loss_dim, loss_angle, loss_depth_map, loss_tfl, loss_mask (+ ``_i`` for the auxiliary
decoder layers), class_error / cardinality_error for logging.  The template-fitting / mask losses
(:342-394, :577-1157) are disabled in every shipped config (use_tfl / use_mask_loss False) and
depend on pytorch3d/open3d symbols the reference never imports; they return the same zero
placeholders here and raise if switched on.

``num_boxes`` is all-reduced over the data-parallel group (:1202-1206) so that N GPUs at
per-GPU batch b compute the same loss as one GPU at batch N*b.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import box_ops
from .losses import DDNLoss, sigmoid_focal_loss
from .misc import accuracy, get_world_size, is_dist_avail_and_initialized
from ..pointwise import (focal_classification, focal_classification_supported, focal_classification_weighted_supported, ignore_flags,
                         matched_losses, matched_losses_supported)


def _paired_giou(a, b):
    """GIoU of matched xyxy boxes a[..., 4], b[..., 4] (the diagonal of box_ops.generalized_box_iou)."""
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a + area_b - inter
    wh_c = (torch.max(a[..., 2:], b[..., 2:]) - torch.min(a[..., :2], b[..., :2])).clamp(min=0)
    area_c = wh_c[..., 0] * wh_c[..., 1]
    return inter / union - (area_c - union) / area_c


def _dev(values, dtype, device):
    """Small host values -> device WITHOUT blocking the host: on ROCm ``torch.tensor(list, device=cuda)`` and
    ``torch.as_tensor(list, device=cuda)`` wait for every queued kernel (214 ms behind a 214 ms queue,
    tools/h2d_probe.py), a staged ``.to(device, non_blocking=True)`` of a CPU tensor returns in 70 us."""
    return torch.as_tensor(np.asarray(values)).to(dtype).to(device, non_blocking=True)


def label_weight_sum(weights, mask=None):
    """W of the weighted normaliser: the per-label weights (host values; with ``mask`` the padded [B, max_objs] array and its object
    mask) added up in float64 in flat order."""
    w = np.asarray(weights, dtype=np.float64)
    w = w[np.asarray(mask, dtype=bool)] if mask is not None else w.reshape(-1)
    return float(np.cumsum(w)[-1]) if w.size else 0.0


def _has_label_weight(targets):
    flat = getattr(targets, "flat", None)
    if flat is not None:
        return "label_weight" in flat
    return len(targets) > 0 and all("label_weight" in t for t in targets)


def _host_weight_sum(targets):
    """``TargetList.weight_sum`` where ``prepare_targets`` formed it, else from host-resident weights; never a device read."""
    ws = getattr(targets, "weight_sum", None)
    if ws is not None:
        return float(ws)
    if any(t["label_weight"].is_cuda for t in targets):
        raise ValueError("the weighted normaliser is formed on the host: device-resident label_weight needs the weight_sum that "
                         "synthetic.prepare_targets sets from the host copy (synthetic.attach_host_weight)")
    return label_weight_sum(np.concatenate([t["label_weight"].detach().reshape(-1).numpy() for t in targets]))


def _ignore_regions(targets):
    """(ignore boxes [B, M, 4] xyxy normalised, mask [B, M]) that ``synthetic.prepare_targets`` leaves on the ``TargetList`` of a batch
    with ``ignore_boxes`` in which some image has one; None: nothing below changes."""
    return getattr(targets, "ignore", None)


def check_ignore_ioa(value):
    """``model.ignore_ioa``: the share of a query box's own area that must lie inside an ignore box, a float in (0, 1]."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 < float(value) <= 1.0):
        raise ValueError("model.ignore_ioa = %r is not a number in (0, 1]" % (value,))
    return float(value)


def check_ignore_depth_map(value):
    """``model.ignore_depth_map``: a bool; absent, None or False: off."""
    if value is None:
        return False
    if not isinstance(value, bool):
        raise ValueError("model.ignore_depth_map = %r is not a bool" % (value,))
    return value


FUSED_FOCAL = True       # classification side (focal sums, class / cardinality errors) as one HIP kernel each way
FUSED_MATCHED = True     # matched-pair losses through the HIP kernels on the GPU (False: the PyTorch formulation below)


_PEEK_ZERO = {}          # device -> the zero LossDict.peek hands out for disabled losses


class LossDict(dict):
    """The criterion's loss dictionary (same keys as the reference) that also remembers the [n_keys, n_layers] matrix its
    per-layer entries are views of, so that ``weighted_total`` is one multiply-and-sum instead of ~60 scalar kernels.
    With ``lazy`` set (name -> (row, layer)) the per-layer entries are created on first access: the ~30 select calls are
    host time directly behind the matcher's synchronisation, and the training loop reads them only when it logs."""
    mat = None          # [n_keys, NL] tensor; entry (i, l) is self[keys[i] + suffix(l)]
    keys_ = ()
    extras = ()         # names of the remaining differentiable scalars (loss_depth_map)
    lazy = None
    _zero = None

    def __missing__(self, key):
        if self.lazy is not None and key in self.lazy:
            i, l = self.lazy[key]
            if i >= 0:
                value = self.mat[i, l]
            else:                                    # loss_tfl / loss_mask: disabled losses, one shared zero
                if self._zero is None:
                    self._zero = torch.zeros((), device=self.mat.device, dtype=torch.float32, requires_grad=True)
                value = self._zero
            dict.__setitem__(self, key, value)
            return value
        raise KeyError(key)

    def peek(self, key):
        """The value of ``self[key]``, to be read only (detached for the disabled losses), without creating a lazy entry: the
        dictionary's key order -- what the training log prints in -- stays as it is."""
        if dict.__contains__(self, key) or self.lazy is None or key not in self.lazy:
            return dict.__getitem__(self, key)
        i, l = self.lazy[key]
        if i >= 0:
            return self.mat[i, l]
        zero = _PEEK_ZERO.get(self.mat.device)           # loss_tfl / loss_mask: one constant zero per device, made once (no fill per step)
        if zero is None:
            zero = _PEEK_ZERO[self.mat.device] = torch.zeros((), device=self.mat.device, dtype=torch.float32)
        return zero

    def _all_keys(self):
        seen = list(dict.keys(self))
        if self.lazy:
            have = set(seen)
            seen += [k for k in self.lazy if k not in have]
        return seen

    def __contains__(self, key):
        return dict.__contains__(self, key) or (self.lazy is not None and key in self.lazy)

    def __iter__(self):
        return iter(self._all_keys())

    def __len__(self):
        return len(self._all_keys())

    def keys(self):
        return self._all_keys()

    def items(self):
        return [(k, self[k]) for k in self._all_keys()]

    def values(self):
        return [self[k] for k in self._all_keys()]

    def get(self, key, default=None):
        return self[key] if key in self else default


_WEIGHT_CACHE = {}


def weighted_total(loss_dict, weight_dict):
    """``sum(loss_dict[k] * weight_dict[k] for k in loss_dict if k in weight_dict)`` (trainer_helper.py:140-141).
    For the criterion's own LossDict: one [n_keys, n_layers] multiply-and-sum plus the depth-map term; the ~60 scalar
    multiplies and adds of the literal expression (and their ~60 backward kernels) sit right behind the matcher's host
    sync, where the GPU queue is empty and every launch is exposed."""
    mat = getattr(loss_dict, "mat", None)
    if mat is not None:
        NL = mat.shape[1]
        suffix = lambda l: "" if l == 0 else "_%d" % (l - 1)
        w_host = [[float(weight_dict.get(k + suffix(l), 0.0)) for l in range(NL)] for k in loss_dict.keys_]
        key = (loss_dict.keys_, NL, str(mat.device), tuple(map(tuple, w_host)))
        w = _WEIGHT_CACHE.get(key)
        if w is None:
            w = _WEIGHT_CACHE[key] = torch.tensor(w_host, dtype=mat.dtype).to(mat.device)
        total = (mat * w).sum()
        for k in loss_dict.extras:
            if k in weight_dict:
                total = total + loss_dict[k] * float(weight_dict[k])
        return total
    keys = [k for k in loss_dict if k in weight_dict]
    if not keys:
        return 0
    vals = torch.stack([loss_dict[k].reshape(()) for k in keys])
    w = _dev([float(weight_dict[k]) for k in keys], vals.dtype, vals.device) if vals.is_cuda else \
        torch.tensor([float(weight_dict[k]) for k in keys], dtype=vals.dtype)
    return torch.dot(vals, w)


class SetCriterion(nn.Module):
    # a monosowa_amd.label_audit.LabelAudit: both formulations hand it the final layer's predictions and matched pairs once the pairs are
    # known (``observe``: one launch, nothing waits); None: nothing is launched, allocated or read for it
    audit = None
    _ignore_last = None      # what ignore_report reads: the flags, their per-layer counts and the pairs of the last forward with ignore boxes
    _ignore_depth_last = None      # what ignore_depth_report reads: (ignored-pixel counts, B * H * W) of the last forward that ignored pixels

    def __init__(self, num_classes, matcher, weight_dict, focal_alpha, losses, group_num=11, cfg=None,
                 depth_map_size=(80, 24), fast=True):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.losses = losses
        self.focal_alpha = focal_alpha
        self.ddn_loss = DDNLoss()
        self.group_num = group_num
        # width, height of the stride-16 depth map; the reference hard-codes [80, 24, 80, 24] (:528)
        self.depth_map_size = tuple(depth_map_size)
        # fast=True: all decoder layers matched and scored together with flat indices (one device->host
        # copy per step); fast=False: the layer-by-layer, image-by-image formulation of the reference.
        self.fast = fast
        self.use_tfl = bool(cfg["use_tfl"]) if cfg is not None else False
        self.use_mask_loss = bool(cfg["use_mask_loss"]) if cfg is not None else False
        self.mask_loss = cfg["mask_loss"] if cfg is not None else "DICE"
        # share of a query box's own area inside an ignore box from which an unmatched query is left out of loss_ce; read only when the
        # targets carry ignore boxes (dataset.ignore_regions)
        self.ignore_ioa = check_ignore_ioa(cfg.get("ignore_ioa", 0.5) if cfg is not None else 0.5)
        # depth-map pixels under an ignore box (and under no target box) leave loss_depth_map; acts only on targets with ignore boxes
        self.ignore_depth_map = check_ignore_depth_map(cfg.get("ignore_depth_map") if cfg is not None else None)
        if self.use_tfl or self.use_mask_loss:
            raise NotImplementedError("use_tfl / use_mask_loss need pytorch3d + open3d rendering that the reference "
                                      "itself does not import; they are off in every shipped config")

    # ------------------------------------------------------------------ index helpers
    @staticmethod
    def _get_src_permutation_idx(indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        src_idx = torch.cat([src for (src, _) in indices])
        return batch_idx, src_idx

    @staticmethod
    def _get_tgt_permutation_idx(indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        tgt_idx = torch.cat([tgt for (_, tgt) in indices])
        return batch_idx, tgt_idx

    @staticmethod
    def _matched(targets, indices, key, cols=None):
        parts = [t[key][i] if cols is None else t[key][:, cols][i] for t, (_, i) in zip(targets, indices)]
        return torch.cat(parts, dim=0)

    # ------------------------------------------------------------------ individual losses
    def loss_labels(self, outputs, targets, indices, num_boxes, log=True, info=None):
        src_logits = outputs["pred_logits"]
        idx = self._get_src_permutation_idx(indices)
        target_classes_o = self._matched(targets, indices, "labels")
        target_classes = torch.full(src_logits.shape[:2], self.num_classes, dtype=torch.int64, device=src_logits.device)
        target_classes[idx] = target_classes_o.squeeze().long()
        onehot = torch.zeros([src_logits.shape[0], src_logits.shape[1], src_logits.shape[2] + 1],
                             dtype=src_logits.dtype, device=src_logits.device)
        onehot.scatter_(2, target_classes.unsqueeze(-1), 1)
        regions = _ignore_regions(targets)
        if regions is not None:                     # unmatched queries on an ignore box: none of their C terms, no gradient
            flags, counts = ignore_flags(outputs["pred_boxes"].detach().unsqueeze(0), regions[0], regions[1], self.ignore_ioa)
            ignored = (flags[0].bool() & (target_classes == self.num_classes)).unsqueeze(-1)
            if self._ignore_last is None or "layers" not in self._ignore_last:
                self._ignore_last = {"layers": []}
            self._ignore_last["layers"].append((flags[0], counts, idx))
            cell_w = None
            if _has_label_weight(targets):
                cell_w = torch.ones(src_logits.shape[:2], dtype=src_logits.dtype, device=src_logits.device)
                cell_w[idx] = self._matched(targets, indices, "label_weight").to(src_logits.dtype)
                cell_w = cell_w.unsqueeze(-1)
            loss_ce = sigmoid_focal_loss(src_logits, onehot[:, :, :-1], num_boxes, alpha=self.focal_alpha, gamma=2, weight=cell_w,
                                         ignore=ignored) * src_logits.shape[1]
        elif _has_label_weight(targets):            # the C terms of a matched query times its label's weight, 1 elsewhere
            cell_w = torch.ones(src_logits.shape[:2], dtype=src_logits.dtype, device=src_logits.device)
            cell_w[idx] = self._matched(targets, indices, "label_weight").to(src_logits.dtype)
            loss_ce = sigmoid_focal_loss(src_logits, onehot[:, :, :-1], num_boxes, alpha=self.focal_alpha, gamma=2,
                                         weight=cell_w.unsqueeze(-1)) * src_logits.shape[1]
        else:
            loss_ce = sigmoid_focal_loss(src_logits, onehot[:, :, :-1], num_boxes, alpha=self.focal_alpha, gamma=2) \
                * src_logits.shape[1]
        losses = {"loss_ce": loss_ce}
        if log:
            losses["class_error"] = 100 - accuracy(src_logits[idx], target_classes_o)[0]
        return losses

    @torch.no_grad()
    def loss_cardinality(self, outputs, targets, indices, num_boxes, info=None):
        pred_logits = outputs["pred_logits"]
        tgt_lengths = torch.as_tensor([len(v["labels"]) for v in targets], device=pred_logits.device)
        card_pred = (pred_logits.argmax(-1) != pred_logits.shape[-1] - 1).sum(1)
        return {"cardinality_error": F.l1_loss(card_pred.float(), tgt_lengths.float())}

    def loss_3dcenter(self, outputs, targets, indices, num_boxes, info=None):
        idx = self._get_src_permutation_idx(indices)
        src = outputs["pred_boxes"][:, :, 0:2][idx]
        tgt = self._matched(targets, indices, "boxes_3d", slice(0, 2))
        if _has_label_weight(targets):
            w = self._matched(targets, indices, "label_weight").to(src.dtype)
            return {"loss_center": (F.l1_loss(src, tgt, reduction="none") * w[:, None]).sum() / num_boxes}
        return {"loss_center": F.l1_loss(src, tgt, reduction="none").sum() / num_boxes}

    def loss_boxes(self, outputs, targets, indices, num_boxes, info=None):
        idx = self._get_src_permutation_idx(indices)
        src_lrtb = outputs["pred_boxes"][:, :, 2:6][idx]
        tgt_lrtb = self._matched(targets, indices, "boxes_3d", slice(2, 6))
        w = self._matched(targets, indices, "label_weight").to(src_lrtb.dtype) if _has_label_weight(targets) else None
        l1 = F.l1_loss(src_lrtb, tgt_lrtb, reduction="none")
        losses = {"loss_bbox": (l1 if w is None else l1 * w[:, None]).sum() / num_boxes}
        src_boxes = outputs["pred_boxes"][idx]
        tgt_boxes = self._matched(targets, indices, "boxes_3d")
        giou = torch.diag(box_ops.generalized_box_iou(box_ops.box_cxcylrtb_to_xyxy(src_boxes),
                                                      box_ops.box_cxcylrtb_to_xyxy(tgt_boxes), check=False))
        losses["loss_giou"] = ((1 - giou) if w is None else (1 - giou) * w).sum() / num_boxes
        return losses

    def loss_depths(self, outputs, targets, indices, num_boxes, info=None):
        idx = self._get_src_permutation_idx(indices)
        src = outputs["pred_depth"][idx]
        tgt = self._matched(targets, indices, "depth").squeeze()
        depth, log_var = src[:, 0], src[:, 1]
        loss = 1.4142 * torch.exp(-log_var) * torch.abs(depth - tgt) + log_var     # Laplacian aleatoric
        if _has_label_weight(targets):
            loss = loss * self._matched(targets, indices, "label_weight").to(loss.dtype)
        return {"loss_depth": loss.sum() / num_boxes}

    def loss_dims(self, outputs, targets, indices, num_boxes, info=None):
        idx = self._get_src_permutation_idx(indices)
        src = outputs["pred_3d_dim"][idx]
        tgt = self._matched(targets, indices, "size_3d")
        dim_loss = torch.abs(src - tgt) / tgt.clone().detach()
        if _has_label_weight(targets):              # sum w |s - s*| / sum w |s - s*| / s*, as two means over the same count
            w = self._matched(targets, indices, "label_weight").to(src.dtype)[:, None]
            dim_loss = dim_loss * w
            with torch.no_grad():
                compensation = (torch.abs(src - tgt) * w).mean() / dim_loss.mean()
            return {"loss_dim": (dim_loss * compensation).sum() / num_boxes}
        with torch.no_grad():
            compensation = F.l1_loss(src, tgt) / dim_loss.mean()
        return {"loss_dim": (dim_loss * compensation).sum() / num_boxes}

    def loss_angles(self, outputs, targets, indices, num_boxes, info=None):
        idx = self._get_src_permutation_idx(indices)
        heading = outputs["pred_angle"][idx].view(-1, 24)
        cls_t = self._matched(targets, indices, "heading_bin").view(-1).long()
        res_t = self._matched(targets, indices, "heading_res").view(-1)
        cls_loss = F.cross_entropy(heading[:, 0:12], cls_t, reduction="none")
        onehot = torch.zeros(cls_t.shape[0], 12, device=heading.device, dtype=heading.dtype).scatter_(
            dim=1, index=cls_t.view(-1, 1), value=1)
        res_pred = torch.sum(heading[:, 12:24] * onehot, 1)
        reg_loss = F.l1_loss(res_pred, res_t, reduction="none")
        if _has_label_weight(targets):
            return {"loss_angle": ((cls_loss + reg_loss) * self._matched(targets, indices, "label_weight").to(cls_loss.dtype)).sum() / num_boxes}
        return {"loss_angle": (cls_loss + reg_loss).sum() / num_boxes}

    def loss_depth_map(self, outputs, targets, indices, num_boxes, info=None):
        logits = outputs["pred_depth_map_logits"]
        num_gt_per_img = [len(t["boxes"]) for t in targets]
        w, h = self.depth_map_size
        scale = torch.tensor([w, h, w, h], device=logits.device, dtype=logits.dtype)
        boxes = box_ops.box_cxcywh_to_xyxy(torch.cat([t["boxes"] for t in targets], dim=0) * scale)
        centre_depth = torch.cat([t["depth"] for t in targets], dim=0).squeeze(dim=1)
        ignore = self._ignore_depth_pair(targets, logits.device)
        if ignore is not None:
            box_weight = torch.cat([t["label_weight"] for t in targets], dim=0) if _has_label_weight(targets) else None
            loss = self.ddn_loss(logits, boxes, num_gt_per_img, centre_depth, box_weight=box_weight, ignore=ignore)
            self._ignore_depth_last = (self.ddn_loss.ign_count, logits.shape[0] * logits.shape[2] * logits.shape[3])
            return {"loss_depth_map": loss}
        if _has_label_weight(targets):
            return {"loss_depth_map": self.ddn_loss(logits, boxes, num_gt_per_img, centre_depth,
                                                    box_weight=torch.cat([t["label_weight"] for t in targets], dim=0))}
        return {"loss_depth_map": self.ddn_loss(logits, boxes, num_gt_per_img, centre_depth)}

    def _ignore_depth_pair(self, targets, device):
        """(ignore boxes [B, M, 4] in depth-map pixels -- the normalised boxes times (w, h, w, h) in float32, one rounding per coordinate,
        the multiply the target boxes get --, mask [B, M] bool) for the depth-map loss; None with model.ignore_depth_map off or on a
        batch without ignore boxes."""
        regions = _ignore_regions(targets)
        if not self.ignore_depth_map or regions is None:
            return None
        w, h = self.depth_map_size
        return regions[0].to(torch.float32) * _dev([w, h, w, h], torch.float32, device), regions[1].to(torch.bool)

    def loss_tfl(self, outputs, targets, indices, num_boxes, info=None):
        dev = outputs["pred_logits"].device
        return {"loss_tfl": torch.tensor(0., device=dev, dtype=torch.float32, requires_grad=True),
                "loss_mask": torch.tensor(0., device=dev, dtype=torch.float32, requires_grad=True)}

    def get_loss(self, loss, outputs, targets, indices, num_boxes, **kwargs):
        loss_map = {"labels": self.loss_labels, "cardinality": self.loss_cardinality, "boxes": self.loss_boxes,
                    "depths": self.loss_depths, "dims": self.loss_dims, "angles": self.loss_angles,
                    "center": self.loss_3dcenter, "depth_map": self.loss_depth_map, "tfl": self.loss_tfl}
        assert loss in loss_map, f"do you really want to compute {loss} loss?"
        return loss_map[loss](outputs, targets, indices, num_boxes, **kwargs)

    def forward(self, outputs, targets, mask_dict=None, info=None, num_boxes=None):
        """``num_boxes`` (a float or a 0-d device tensor): the normaliser to use in place of this forward's own box count, already
        job-wide -- nothing is all-reduced then.  The Trainer's gradient accumulation passes the cycle-wide count."""
        if _ignore_regions(targets) is None:
            self._ignore_last = None
        self._ignore_depth_last = None
        if self.fast:
            return self.forward_fast(outputs, targets, num_boxes)
        return self.forward_layerwise(outputs, targets, mask_dict, info, num_boxes)

    # ------------------------------------------------------------------ batched formulation
    def _num_boxes(self, targets, group_num, device):
        """max(n * group_num / ranks, 1), n the label count -- with ``label_weight`` in the targets the sum of the weights."""
        if _has_label_weight(targets):
            n = float(_host_weight_sum(targets) * group_num)
        else:
            n = float(sum(len(t["labels"]) for t in targets) * group_num)
        if is_dist_avail_and_initialized():       # stays on the device: dividing by a tensor needs no sync
            t = _dev([n], torch.float, device)
            torch.distributed.all_reduce(t)
            return torch.clamp(t / get_world_size(), min=1)[0]
        return max(n / get_world_size(), 1.0)

    def forward_fast(self, outputs, targets, num_boxes=None):
        """Same losses as ``forward_layerwise`` (same keys, same normalisation); the matching of all decoder
        layers is one cost pass + one host copy + one native call, and every loss is evaluated for all layers
        at once through flat (layer, batch, query) / target index tensors."""
        layers = [{k: v for k, v in outputs.items() if k != "aux_outputs"}] + list(outputs.get("aux_outputs", []))
        NL = len(layers)
        group_num = self.group_num if self.training else 1
        logits = torch.stack([o["pred_logits"] for o in layers])          # [NL,B,Q,C]
        boxes = torch.stack([o["pred_boxes"] for o in layers])            # [NL,B,Q,6]
        dims = torch.stack([o["pred_3d_dim"] for o in layers])
        depth = torch.stack([o["pred_depth"] for o in layers])
        angle = torch.stack([o["pred_angle"] for o in layers])
        _, B, Q, C = logits.shape
        dev = logits.device
        sizes = [len(t["labels"]) for t in targets]
        T = sum(sizes)
        flat_keys = ("labels", "boxes_3d", "boxes", "depth", "size_3d", "heading_bin", "heading_res")
        flat = getattr(targets, "flat", None)              # prepare_targets hands the batch-flat tensors along (7 launches fewer)
        weighted = _has_label_weight(targets)
        if flat is None or any(k not in flat for k in flat_keys) or flat["labels"].shape[0] != T:
            flat = {k: torch.cat([t[k] for t in targets], dim=0) for k in flat_keys + (("label_weight",) if weighted else ())}
        # per-label weights [T] (float32, finite, >= 0): every loss term a label feeds times its weight; None: nothing below changes
        t_weight = flat["label_weight"].reshape(-1) if weighted else None
        if num_boxes is None:
            num_boxes = self._num_boxes(targets, group_num, dev)

        pending = self.matcher.match_layers_begin(logits, boxes, flat, sizes, group_num)      # cost pass + async D2H

        # depth map (final layer only): padded per-image boxes, rasterised on the device.  Independent of the matching,
        # so it is enqueued between the two halves of the matcher: the GPU works on it while the host waits for the
        # cost blocks and solves the assignments.
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        maxn = max(sizes) if sizes else 0
        w, h = self.depth_map_size
        if maxn:
            slot = np.minimum(offs[:, None] + np.arange(maxn)[None, :], max(T - 1, 0))
            valid = np.arange(maxn)[None, :] < np.asarray(sizes)[:, None]
            slot_t = torch.as_tensor(slot, dtype=torch.int64).to(dev, non_blocking=True)
            valid_t = torch.as_tensor(valid).to(dev, non_blocking=True)
            scale = _dev([w, h, w, h], logits.dtype, dev)
            boxes2d = box_ops.box_cxcywh_to_xyxy(flat["boxes"] * scale)[slot_t]
            depth2d = flat["depth"].squeeze(1)[slot_t]
        else:
            valid_t = torch.zeros((B, 1), dtype=torch.bool, device=dev)
            boxes2d = torch.zeros((B, 1, 4), device=dev, dtype=logits.dtype)
            depth2d = torch.zeros((B, 1), device=dev, dtype=logits.dtype)
        regions = _ignore_regions(targets)
        ignore_px = self._ignore_depth_pair(targets, dev)
        if ignore_px is not None:                   # model.ignore_depth_map: the ignore-region kernels, the same place in the queue
            map_logits = outputs["pred_depth_map_logits"]
            weight2d = None
            if weighted:
                weight2d = t_weight.to(logits.dtype)[slot_t] if maxn else torch.ones((B, 1), device=dev, dtype=logits.dtype)
            loss_depth_map = self.ddn_loss.forward_padded(map_logits, boxes2d, depth2d, valid_t, box_weight=weight2d, ignore=ignore_px)
            self._ignore_depth_last = (self.ddn_loss.ign_count, map_logits.shape[0] * map_logits.shape[2] * map_logits.shape[3])
        elif weighted:
            weight2d = t_weight.to(logits.dtype)[slot_t] if maxn else torch.ones((B, 1), device=dev, dtype=logits.dtype)
            loss_depth_map = self.ddn_loss.forward_padded(outputs["pred_depth_map_logits"], boxes2d, depth2d, valid_t, box_weight=weight2d)
        else:
            loss_depth_map = self.ddn_loss.forward_padded(outputs["pred_depth_map_logits"], boxes2d, depth2d, valid_t)
        # ignore regions: which queries sit on an ignore box does not depend on the matching either -- one launch, here
        flags = None
        if regions is not None:
            flags, flag_counts = ignore_flags(boxes.detach(), regions[0], regions[1], self.ignore_ioa)

        # everything the fused tail needs that does not depend on the assignment is made ready BEFORE the wait: behind it the
        # GPU queue is empty and every microsecond of host time is step time (measured: 1.05 ms from indices to total)
        fused_tail = FUSED_FOCAL and FUSED_MATCHED and T > 0 and logits.is_cuda and logits.dtype == torch.float32
        if fused_tail:
            f32, i64 = torch.float32, torch.int64
            prep = [t.contiguous() for t in (logits, boxes, depth, dims, angle)]
            prep_t = [flat["boxes_3d"].to(f32).contiguous(), flat["depth"].reshape(-1).to(f32).contiguous(), flat["size_3d"].to(f32).contiguous(),
                      flat["heading_bin"].reshape(-1).to(i64).contiguous(), flat["heading_res"].reshape(-1).to(f32).contiguous()]
            labels64 = flat["labels"].to(i64).contiguous()
            weight32 = t_weight.to(f32).contiguous() if weighted else None
            sizes_dev = _dev(sizes, f32, dev)
            nb = num_boxes if torch.is_tensor(num_boxes) else float(num_boxes)
            # rows of the loss matrix: focal sum, class error, cardinality error, six matched-pair sums; divided by num_boxes
            # where the reference does (a [9, 1] column, 1 for the two logging entries)
            inv = (1.0 / nb) if not torch.is_tensor(nb) else None
            scale_col = _dev([inv, 1.0, 1.0] + [inv] * 6, f32, dev).view(9, 1) if inv is not None else \
                torch.cat([1.0 / nb.reshape(1), nb.new_ones(2), (1.0 / nb.reshape(1)).expand(6)]).view(9, 1)

        idx_host = self.matcher.match_layers_end_flat(pending)                 # [3, NL, K] int64 (host: numpy, or a pinned tensor)
        K = idx_host.shape[2]
        # from the matcher's pinned buffer the copy is queued behind the depth-map kernels still running; from pageable memory
        # the host would wait for them here, with the whole backward still to enqueue
        idx = (idx_host if torch.is_tensor(idx_host) else torch.from_numpy(idx_host)).to(dev, non_blocking=True)
        if self.audit is not None:                                             # layer 0 of the stack is the model's final output
            with torch.no_grad():
                self.audit.observe(*[t.detach() for t in (prep if fused_tail else (logits, boxes, depth, dims, angle))], idx,
                                   dict(flat, labels=labels64) if fused_tail else flat, layer=0)
        if flags is not None:
            self._ignore_last = {"flags": flags, "counts": flag_counts, "idx": idx}
        if weighted and fused_tail and K > 0 and focal_classification_weighted_supported(logits, idx):
            # the same four launches through the weighted entry points
            from ..pointwise import _FocalClassificationIgnore, _FocalClassificationWeighted, _MatchedLossesWeighted
            if flags is not None:
                cls3 = _FocalClassificationIgnore.apply(prep[0], idx, labels64, sizes_dev, weight32, flags, float(self.focal_alpha), 2.0)
            else:
                cls3 = _FocalClassificationWeighted.apply(prep[0], idx, labels64, sizes_dev, weight32, float(self.focal_alpha), 2.0)
            sums = _MatchedLossesWeighted.apply(prep[1], prep[2], prep[3], prep[4], idx, *prep_t, weight32)
            mat = torch.cat([cls3, sums], 1).t() * scale_col                     # [9, NL]
            keys = ("loss_ce", "class_error", "cardinality_error", "loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim",
                    "loss_angle")
            return self._finish(keys, NL, dev, loss_depth_map, mat=mat)
        if not weighted and fused_tail and K > 0 and focal_classification_supported(logits, idx):
            # the whole criterion behind the matching in four launches: classification side + matched-pair losses, forward
            # and backward (csrc/matched_losses.hip), the loss matrix in two more
            from ..pointwise import _FocalClassification, _FocalClassificationIgnore, _MatchedLosses
            if flags is not None:
                cls3 = _FocalClassificationIgnore.apply(prep[0], idx, labels64, sizes_dev, None, flags, float(self.focal_alpha), 2.0)
            else:
                cls3 = _FocalClassification.apply(prep[0], idx, labels64, sizes_dev, float(self.focal_alpha), 2.0)
            sums = _MatchedLosses.apply(prep[1], prep[2], prep[3], prep[4], idx, *prep_t)
            mat = torch.cat([cls3, sums], 1).t() * scale_col                     # [9, NL]
            keys = ("loss_ce", "class_error", "cardinality_error", "loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim",
                    "loss_angle")
            return self._finish(keys, NL, dev, loss_depth_map, mat=mat)
        b_idx, q_idx, t_idx = idx[0], idx[1], idx[2]
        l_idx = torch.arange(NL, device=dev).view(NL, 1).expand(NL, K)
        take = lambda t: t[l_idx, b_idx, q_idx]                             # [NL,K,...] matched predictions
        per_layer = {}

        # labels (focal), class error, cardinality
        tgt_cls = flat["labels"].long()[t_idx] if T else torch.zeros((NL, 0), dtype=torch.int64, device=dev)
        target_classes = torch.full((NL, B, Q), self.num_classes, dtype=torch.int64, device=dev)
        target_classes[l_idx, b_idx, q_idx] = tgt_cls
        onehot = torch.zeros((NL, B, Q, C + 1), dtype=logits.dtype, device=dev).scatter_(3, target_classes.unsqueeze(-1), 1)[..., :-1]
        cls_logits = logits
        if flags is not None:                       # an ignored cell: selected away on both sides, its logits reach nothing
            ignored = (flags.bool() & (target_classes == self.num_classes)).unsqueeze(-1)
            cls_logits = torch.where(ignored, logits.new_zeros(()), logits)
        prob = cls_logits.sigmoid()
        ce = F.binary_cross_entropy_with_logits(cls_logits, onehot, reduction="none")
        p_t = prob * onehot + (1 - prob) * (1 - onehot)
        focal = ce * ((1 - p_t) ** 2)
        if self.focal_alpha >= 0:
            focal = (self.focal_alpha * onehot + (1 - self.focal_alpha) * (1 - onehot)) * focal
        pair_w = None
        if weighted:                                # [NL, K] weight of every pair; a matched cell carries its target's, the others 1
            pair_w = t_weight.to(logits.dtype)[t_idx] if T else torch.zeros((NL, 0), dtype=logits.dtype, device=dev)
            cell_w = torch.ones((NL, B, Q), dtype=logits.dtype, device=dev)
            cell_w[l_idx, b_idx, q_idx] = pair_w
            focal = focal * cell_w.unsqueeze(-1)
        if flags is not None:
            focal = torch.where(ignored, focal.new_zeros(()), focal)
        per_layer["loss_ce"] = focal.mean(2).sum((1, 2)) / num_boxes * Q
        matched_logits = take(logits)
        if K:
            # 100 * wrong / K, not 100 - 100 * correct / K: the subtraction cancels the leading digits of a small error
            wrong = K - matched_logits.argmax(-1).eq(tgt_cls).float().sum(1)
            per_layer["class_error"] = wrong * 100.0 / K
        else:
            per_layer["class_error"] = torch.full((NL,), 100.0, device=dev)
        tgt_lengths = _dev(sizes, torch.float, dev)
        card_pred = (logits.argmax(-1) != C - 1).sum(2).float()
        per_layer["cardinality_error"] = (card_pred - tgt_lengths).abs().mean(1)

        if FUSED_MATCHED and matched_losses_supported(boxes, idx):
            # all six matched-pair losses of all layers: one HIP launch forward, one backward (csrc/matched_losses.hip)
            if weighted:
                sums = matched_losses(boxes, depth, dims, angle, idx, flat["boxes_3d"], flat["depth"], flat["size_3d"],
                                      flat["heading_bin"], flat["heading_res"], weight=t_weight) / num_boxes
            else:
                sums = matched_losses(boxes, depth, dims, angle, idx, flat["boxes_3d"], flat["depth"], flat["size_3d"],
                                      flat["heading_bin"], flat["heading_res"]) / num_boxes
            for j, k in enumerate(("loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim", "loss_angle")):
                per_layer[k] = sums[:, j]
            return self._finish(per_layer, NL, dev, loss_depth_map)
        # boxes: 3D-centre L1, l/r/t/b L1, GIoU of matched pairs
        wk = (lambda x: x) if pair_w is None else (lambda x: x * (pair_w if x.dim() == 2 else pair_w.unsqueeze(-1)))   # a pair's terms x w_t
        src_box, tgt_box = take(boxes), flat["boxes_3d"][t_idx]
        per_layer["loss_center"] = wk((src_box[..., 0:2] - tgt_box[..., 0:2]).abs()).sum((1, 2)) / num_boxes
        per_layer["loss_bbox"] = wk((src_box[..., 2:6] - tgt_box[..., 2:6]).abs()).sum((1, 2)) / num_boxes
        giou = _paired_giou(box_ops.box_cxcylrtb_to_xyxy(src_box), box_ops.box_cxcylrtb_to_xyxy(tgt_box))
        per_layer["loss_giou"] = wk(1 - giou).sum(1) / num_boxes
        # depth (Laplacian aleatoric uncertainty)
        src_d, tgt_d = take(depth), flat["depth"][t_idx].squeeze(-1)
        per_layer["loss_depth"] = wk(1.4142 * torch.exp(-src_d[..., 1]) * (src_d[..., 0] - tgt_d).abs() + src_d[..., 1]).sum(1) / num_boxes
        # 3D size (dimension-aware L1 with the per-layer compensation weight; weighted: sum w |s - s*| / sum w |s - s*| / s*)
        src_s, tgt_s = take(dims), flat["size_3d"][t_idx]
        l1 = wk((src_s - tgt_s).abs())
        dim_loss = l1 / tgt_s.detach()
        with torch.no_grad():
            comp = l1.mean((1, 2)) / dim_loss.mean((1, 2))
        per_layer["loss_dim"] = (dim_loss * comp.view(NL, 1, 1)).sum((1, 2)) / num_boxes
        # heading: 12-bin classification + residual of the target bin
        heading = take(angle)
        cls_t = flat["heading_bin"][t_idx].view(NL, K).long()
        res_t = flat["heading_res"][t_idx].view(NL, K)
        cls_loss = F.cross_entropy(heading[..., 0:12].reshape(NL * K, 12), cls_t.reshape(-1), reduction="none").view(NL, K)
        res_pred = torch.gather(heading[..., 12:24], 2, cls_t.unsqueeze(-1)).squeeze(-1)
        per_layer["loss_angle"] = wk(cls_loss + (res_pred - res_t).abs()).sum(1) / num_boxes

        return self._finish(per_layer, NL, dev, loss_depth_map)

    def ignore_report(self):
        """(ignored, cells) of the last forward whose targets carried ignore boxes: per layer (the final one first) the number of
        queries that were flagged by ``ignore_flags`` AND unmatched, i.e. left out of loss_ce, and the number of queries B * Q of a
        layer.  Reads the device (a synchronisation); None before the first such forward."""
        rec = self._ignore_last
        if rec is None:
            return None
        if "layers" in rec:
            if not rec["layers"]:
                return None
            ignored = [int(c.sum()) - int(f[i].sum()) for f, c, i in rec["layers"]]
            return ignored, int(rec["layers"][0][0].numel())
        flags, counts, idx = rec["flags"], rec["counts"], rec["idx"]
        NL, K = idx.shape[1:]
        matched = flags[torch.arange(NL, device=flags.device).view(NL, 1).expand(NL, K), idx[0], idx[1]].sum(1, dtype=torch.int64)
        ignored = (counts.to(torch.int64) - matched).tolist()
        return [int(v) for v in ignored], int(flags[0].numel())

    def ignore_depth_report(self):
        """(ignored_pixels, B * H * W) of the last forward that left depth-map pixels out of loss_depth_map (model.ignore_depth_map on a
        batch with ignore boxes): the pixels under a valid ignore box and under no target box.  Reads the device (a synchronisation)
        like ``ignore_report``; None before any such forward, and after a forward without regions or with the key off."""
        rec = self._ignore_depth_last
        if rec is None or rec[0] is None:
            return None
        return int(rec[0].sum()), int(rec[1])

    @staticmethod
    def _finish(per_layer, NL, dev, loss_depth_map, mat=None):
        losses = LossDict()
        keys = tuple(per_layer) if mat is None else per_layer
        if mat is None:
            mat = torch.stack([per_layer[k] for k in keys])                  # [n_keys, NL]
        lazy = {}
        for l in range(NL):
            suffix = "" if l == 0 else "_%d" % (l - 1)
            for i, k in enumerate(keys):
                lazy[k + suffix] = (i, l)
            lazy["loss_tfl" + suffix] = (-1, l)
            lazy["loss_mask" + suffix] = (-1, l)
        losses.lazy = lazy
        dict.__setitem__(losses, "loss_depth_map", loss_depth_map)
        losses.mat, losses.keys_, losses.extras = mat, keys, ("loss_depth_map",)
        return losses

    # ------------------------------------------------------------------ reference formulation
    def _observe_layerwise(self, outputs, targets, indices):
        """``audit.observe`` with the final layer's per-image ``indices`` as the flat [3, 1, K] index tensor ``forward_fast`` builds:
        (image, query, offset of the image's targets + target), images in order."""
        dev = outputs["pred_logits"].device
        offs = np.concatenate([[0], np.cumsum([len(t["labels"]) for t in targets])[:-1]]).astype(np.int64)
        idx = torch.stack([torch.cat([torch.full_like(src, b) for b, (src, _) in enumerate(indices)]),
                           torch.cat([src for src, _ in indices]),
                           torch.cat([tgt + int(offs[b]) for b, (_, tgt) in enumerate(indices)])]).view(3, 1, -1).to(dev)
        flat = getattr(targets, "flat", None)
        keys = ("labels", "boxes_3d", "depth", "size_3d", "heading_bin", "heading_res")
        if flat is None or any(k not in flat for k in keys):
            flat = {k: torch.cat([t[k] for t in targets], dim=0) for k in keys}
        with torch.no_grad():
            self.audit.observe(*[outputs[k].detach().unsqueeze(0) for k in ("pred_logits", "pred_boxes", "pred_depth", "pred_3d_dim", "pred_angle")],
                               idx, flat, layer=0)

    def forward_layerwise(self, outputs, targets, mask_dict=None, info=None, num_boxes=None):
        outputs_without_aux = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        group_num = self.group_num if self.training else 1
        if _ignore_regions(targets) is not None:
            self._ignore_last = {"layers": []}
        indices = self.matcher(outputs_without_aux, targets, group_num=group_num)
        if self.audit is not None:
            self._observe_layerwise(outputs_without_aux, targets, indices)

        if num_boxes is None:
            if _has_label_weight(targets):
                num_boxes = _host_weight_sum(targets) * group_num
            else:
                num_boxes = sum(len(t["labels"]) for t in targets) * group_num
            num_boxes = torch.as_tensor([num_boxes], dtype=torch.float, device=next(iter(outputs.values())).device)
            if is_dist_avail_and_initialized():
                torch.distributed.all_reduce(num_boxes)
            num_boxes = torch.clamp(num_boxes / get_world_size(), min=1).item()

        losses = {}
        for loss in self.losses:
            losses.update(self.get_loss(loss, outputs, targets, indices, num_boxes, info=info))
        if "aux_outputs" in outputs:
            for i, aux in enumerate(outputs["aux_outputs"]):
                indices = self.matcher(aux, targets, group_num=group_num)
                for loss in self.losses:
                    if loss == "depth_map":     # the depth map has no per-layer prediction
                        continue
                    l_dict = self.get_loss(loss, aux, targets, indices, num_boxes, info=info)
                    losses.update({k + f"_{i}": v for k, v in l_dict.items()})
        return losses
