"""Ignore regions (``ignore_boxes`` / ``ignore_mask``, ``model.ignore_ioa``): an independent restatement.

* ``flags``: numpy float32, one rounding per operation, written from the rule and from nothing in ``monosowa_amd``: a predicted box
  (cx, cy, l, r, t, b) -> p = (cx - l, cy - t, cx + r, cy + b), A = (p.x2 - p.x1)(p.y2 - p.y1); flagged when for a valid box g of its
  image A > 0, iw = min(p.x2, g.x2) - max(p.x1, g.x1) > 0, ih likewise > 0 and iw ih >= ioa A.  ``np.minimum`` / ``np.maximum`` hand
  NaNs on, every comparison with a NaN is false.
* ``focal_sums``: ``label_weights_reference.focal_sums``' conventions (dtype-agnostic torch, autograd) with a cell mask: a cell that is
  flagged and unmatched adds none of its C terms -- its logits are replaced by a constant before anything is computed from them, so a
  non-finite one reaches nothing and its gradient is zero.  class_error and cardinality_error see every cell.
* ``criterion_losses``: the whole loss dictionary under given matched triples, with or without ``label_weight``.
"""
import numpy as np
import torch

import criterion_reference as CR
import label_weights_reference as LW


def flags(boxes, ignore_boxes, ignore_mask, ioa):
    """boxes [NL, B, Q, 6], ignore_boxes [B, M, 4] xyxy, ignore_mask [B, M] -> (uint8 [NL, B, Q], per-layer counts int64 [NL])"""
    p = np.asarray(boxes, dtype=np.float32)
    g = np.asarray(ignore_boxes, dtype=np.float32)
    m = np.asarray(ignore_mask).astype(bool)
    ioa = np.float32(ioa)
    NL, B, Q = p.shape[:3]
    out = np.zeros((NL, B, Q), dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        x1, y1 = p[..., 0] - p[..., 2], p[..., 1] - p[..., 4]
        x2, y2 = p[..., 0] + p[..., 3], p[..., 1] + p[..., 5]
        area = ((x2 - x1) * (y2 - y1)).astype(np.float32)
        need = (ioa * area).astype(np.float32)
        for b in range(B):
            for j in np.nonzero(m[b])[0]:
                iw = (np.minimum(x2[:, b], g[b, j, 2]) - np.maximum(x1[:, b], g[b, j, 0])).astype(np.float32)
                ih = (np.minimum(y2[:, b], g[b, j, 3]) - np.maximum(y1[:, b], g[b, j, 1])).astype(np.float32)
                inter = (iw * ih).astype(np.float32)
                out[:, b] |= ((area[:, b] > 0) & (iw > 0) & (ih > 0) & (inter >= need[:, b])).astype(np.uint8)
    return out, out.reshape(NL, -1).sum(1).astype(np.int64)


def ignored_cells(flag, idx):
    """bool [NL, B, Q]: flagged AND unmatched under the triples idx [3, NL, K]"""
    flag = torch.as_tensor(np.asarray(flag)).bool().clone()
    for l in range(idx.shape[1]):
        flag[l, idx[0, l], idx[1, l]] = False
    return flag


def focal_sums(logits, idx, labels, sizes, weight, ignored, alpha, gamma=2.0):
    """-> [NL, 3] like ``label_weights_reference.focal_sums`` (``weight`` None: all ones), the cells of ``ignored`` [NL, B, Q] left out
    of the focal sum"""
    if weight is None:
        weight = torch.ones(labels.shape[0], dtype=logits.dtype, device=logits.device)
    ignored = ignored.to(logits.device)
    full = LW.focal_sums(logits.detach(), idx, labels, sizes, weight, alpha, gamma) if not ignored.any() else None
    NL, B, Q, C = logits.shape
    out = []
    for l in range(NL):
        b, q, t = idx[0, l], idx[1, l], idx[2, l]
        cls = torch.full((B, Q), C, dtype=torch.int64, device=logits.device)
        cls[b, q] = labels.long()[t]
        cw = torch.ones((B, Q), dtype=logits.dtype, device=logits.device)
        cw[b, q] = weight.reshape(-1)[t].to(logits.dtype)
        keep = ~ignored[l]
        x = logits[l][keep]                                   # [n_kept, C]: the ignored cells' logits are never touched
        one = (cls[keep][:, None] == torch.arange(C, device=logits.device)).to(logits.dtype)
        p = torch.sigmoid(x)
        sp = torch.nn.functional.softplus
        term = (one * sp(-x) + (1 - one) * sp(x)) * (one * (1 - p) + (1 - one) * p) ** gamma
        if alpha >= 0:
            term = term * (alpha * one + (1 - alpha) * (1 - one))
        rest = LW.focal_sums(logits[l:l + 1].detach(), idx[:, l:l + 1], labels, sizes, weight, alpha, gamma)[0]
        out.append(torch.stack([(term * cw[keep][:, None]).sum(), rest[1], rest[2]]))
    out = torch.stack(out)
    if full is not None:                                      # nothing ignored: the weighted reference itself
        assert torch.allclose(out.detach(), full, rtol=1e-12, atol=0) or out.dtype != torch.float64
    return out


def criterion_losses(outputs, targets, idx, n_boxes, alpha, map_wh, ignore_boxes, ignore_mask, ioa, gamma=2.0):
    """The criterion's loss dictionary with ignore regions: ``label_weights_reference.criterion_losses`` (targets without
    'label_weight' count with weight 1), loss_ce of every layer from ``focal_sums`` above.  -> (losses, ignored bool [NL, B, Q])"""
    if not all("label_weight" in t for t in targets):
        targets = [dict(t, label_weight=torch.ones(len(t["labels"]), dtype=t["boxes_3d"].dtype)) for t in targets]
    out = LW.criterion_losses(outputs, targets, idx, n_boxes, alpha, map_wh, gamma)
    st, ft = CR.stack_layers(outputs), CR.flat_targets(targets)
    w = torch.cat([t["label_weight"] for t in targets], 0)
    flag, _ = flags(st["pred_boxes"].detach().cpu().numpy().astype(np.float32), ignore_boxes, ignore_mask, ioa)
    ignored = ignored_cells(flag, idx)
    sizes = torch.tensor([len(t["labels"]) for t in targets], dtype=st["pred_boxes"].dtype)
    foc = focal_sums(st["pred_logits"], idx, ft["labels"], sizes, w, ignored, alpha, gamma)
    for l in range(idx.shape[1]):
        s = "" if l == 0 else "_%d" % (l - 1)
        assert float(out["class_error" + s].detach()) == float(foc[l, 1].detach()) and float(out["cardinality_error" + s].detach()) == float(foc[l, 2].detach())
        out["loss_ce" + s] = foc[l, 0] / n_boxes
    return out, ignored


# ------------------------------------------------------------------------------------------------------------------ cases
def make_flag_case(seed, NL, B, Q, M, ioa=0.5, empty_image=None):
    """Predicted boxes [NL, B, Q, 6] and ignore boxes [B, M, 4] on a dyadic grid (multiples of 2**-6, so that areas and intersections
    are exact in float32), all M slots of every image valid but ``empty_image``'s; planted in the first queries of every image that has
    a box (as far as Q reaches):
      0  a box with exactly ioa of its area inside ignore box 0 (inter == ioa * A)            -> flagged
      1  the same box 2**-25 wider on the outer side (inter one ulp below ioa * A')           -> not flagged
      2  a zero-area box (l = r = 0) inside ignore box 0                                      -> not flagged
      3  a box with a NaN coordinate                                                          -> not flagged
      4  a box wholly inside ignore box 0                                                     -> flagged
    and a NaN in the last ignore box of the last image with boxes (when M > 1): it flags nothing."""
    assert ioa == 0.5
    rng = np.random.default_rng(seed)
    step = 2.0 ** -6
    c = rng.integers(8, 56, (NL, B, Q, 2)) * step
    ext = rng.integers(1, 8, (NL, B, Q, 4)) * step
    boxes = np.concatenate([c, ext], -1).astype(np.float32)
    lo = rng.integers(0, 40, (B, M, 2)) * step
    wh = rng.integers(4, 24, (B, M, 2)) * step
    ign = np.concatenate([lo, np.minimum(lo + wh, 1.0)], -1).astype(np.float32)
    mask = np.ones((B, M), dtype=bool)
    if empty_image is not None:
        mask[empty_image] = False
    for b in range(B):
        if not mask[b].any():
            continue
        ign[b, 0] = [0.25, 0.25, 0.75, 0.75]
        # row 0: p = (0.125, 0.375, 0.375, 0.625), A = 2**-4, iw = 0.375 - 0.25 = 2**-3, ih = 2**-2: inter = 2**-5 = 0.5 A exactly.
        # row 1: l = 2**-3 + 2**-25 moves p.x1 to 0.125 - 2**-25 (exact), A = 2**-4 + 2**-27 (exact), 0.5 A = 2**-5 + 2**-28: one ulp
        # above the same inter
        planted = [[0.25, 0.5, 0.125, 0.125, 0.125, 0.125],
                   [0.25, 0.5, 0.125 + 2.0 ** -25, 0.125, 0.125, 0.125],
                   [0.5, 0.5, 0.0, 0.0, 0.125, 0.125],
                   [0.5, float("nan"), 0.125, 0.125, 0.125, 0.125],
                   [0.5, 0.5, 0.125, 0.0625, 0.03125, 0.125]]
        for q, row in enumerate(planted[:Q]):
            boxes[:, b, q] = row
    if M > 1:
        last = [b for b in range(B) if mask[b].any()][-1]
        ign[last, M - 1, 2] = np.nan
    return boxes, ign, mask


PLANTED_FLAGS = (1, 0, 0, 0, 1)          # of the planted queries against ignore box 0 alone (M == 1)
