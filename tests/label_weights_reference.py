"""Per-label loss weights (``label_weight``): the weighted criterion evaluated from GIVEN matched triples, as a float64 reference.

Plain indexed PyTorch, dtype-agnostic and differentiable by autograd, written from the semantics and from nothing in ``monosowa_amd``:

* matched-pair terms: every pair (l, b, q, t) enters its layer's sum times w_t; the size term's compensation of a layer is
  sum w |s - s*| / sum w |s - s*| / s* (detached);
* classification: all C focal terms of a matched cell (l, b, q) times the w_t of its target, unmatched cells times 1; class_error and
  cardinality_error unweighted;
* depth map: the target depth of a pixel is the nearest valid covering box's (boxes of weight 0 still paint); its factor is
  fg_weight * w_i, i the lowest slot among the covering boxes with that nearest depth (slot order, strict <); background pixels
  bg_weight; divided by the pixel count;
* normaliser: max(W * group_num / ranks, 1), W the float64 sum of the weights in flat order.

The case generators are those of tests/criterion_reference.py; ``draw_weights`` adds the weights."""
import numpy as np
import torch

import criterion_reference as CR

LOSS6 = CR.LOSS6
WEIGHT_VALUES = (0.0, 0.25, 0.5, 1.0, 2.0)


def draw_weights(seed, T):
    """[T] float32: per target one of WEIGHT_VALUES or a draw from U(0, 1.5), half and half; with T >= 2 at least one exact 0 and one
    value above 1 (planted at two drawn places)."""
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(T) < 0.5, rng.choice(WEIGHT_VALUES, T), rng.uniform(0.0, 1.5, T))
    if T >= 2:
        a, b = rng.permutation(T)[:2]
        w[a], w[b] = 0.0, 2.0
    elif T == 1:
        w[0] = 2.0
    return torch.from_numpy(w.astype(np.float32))


def weight_sum(weights):
    """W: the weights added up in float64, one after the other in flat order"""
    total = 0.0
    for x in np.asarray(weights, dtype=np.float64).reshape(-1).tolist():
        total += x
    return total


def num_boxes(weights, group_num, ranks=1):
    return max(weight_sum(weights) * group_num / ranks, 1.0)


def _rows(pred, idx):
    """pred [NL, B, Q, D], idx [3, NL, K] -> [NL, K, D]"""
    NL, K = idx.shape[1:]
    return torch.stack([pred[l, idx[0, l], idx[1, l]] for l in range(NL)]) if K else pred.new_zeros((NL, 0, pred.shape[-1]))


def matched_sums(boxes, depth, dims, angle, idx, t_box, t_depth, t_size, t_bin, t_res, weight):
    """-> [NL, 6] weighted per-layer sums {center, bbox, giou, depth, dim, angle}"""
    NL, K = idx.shape[1:]
    out = []
    for l in range(NL):
        b, q, t = idx[0, l], idx[1, l], idx[2, l]
        w = weight.reshape(-1)[t].to(boxes.dtype)
        pb, tb = boxes[l, b, q], t_box[t]
        center = (w * ((pb[:, 0] - tb[:, 0]).abs() + (pb[:, 1] - tb[:, 1]).abs())).sum()
        bbox = (w * (pb[:, 2:6] - tb[:, 2:6]).abs().sum(1)).sum()
        ax0, ay0, ax1, ay1 = pb[:, 0] - pb[:, 2], pb[:, 1] - pb[:, 4], pb[:, 0] + pb[:, 3], pb[:, 1] + pb[:, 5]
        bx0, by0, bx1, by1 = tb[:, 0] - tb[:, 2], tb[:, 1] - tb[:, 4], tb[:, 0] + tb[:, 3], tb[:, 1] + tb[:, 5]
        iw = (torch.minimum(ax1, bx1) - torch.maximum(ax0, bx0)).clamp(min=0)
        ih = (torch.minimum(ay1, by1) - torch.maximum(ay0, by0)).clamp(min=0)
        inter = iw * ih
        union = (ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter
        hull = (torch.maximum(ax1, bx1) - torch.minimum(ax0, bx0)).clamp(min=0) * (torch.maximum(ay1, by1) - torch.minimum(ay0, by0)).clamp(min=0)
        giou = (w * (1 - (inter / union - (hull - union) / hull))).sum()
        pd, td = depth[l, b, q], t_depth.reshape(-1)[t]
        dep = (w * (1.4142 * torch.exp(-pd[:, 1]) * (pd[:, 0] - td).abs() + pd[:, 1])).sum()
        ps, ts = dims[l, b, q], t_size[t]
        l1 = (ps - ts).abs()
        rel = l1 / ts
        comp = ((w[:, None] * l1).sum() / (w[:, None] * rel).sum()).detach()
        dim = (w[:, None] * rel).sum() * comp
        pa = angle[l, b, q]
        bins = t_bin.reshape(-1)[t].long()
        ce = torch.logsumexp(pa[:, 0:12], dim=1) - pa[torch.arange(K, device=pa.device), bins]
        res = pa[torch.arange(K, device=pa.device), 12 + bins]
        ang = (w * (ce + (res - t_res.reshape(-1)[t]).abs())).sum()
        out.append(torch.stack([center, bbox, giou, dep, dim, ang]))
    return torch.stack(out)


def focal_sums(logits, idx, labels, sizes, weight, alpha, gamma=2.0):
    """-> [NL, 3]: {weighted sigmoid focal SUM, class_error, cardinality_error (both unweighted)}"""
    NL, B, Q, C = logits.shape
    K = idx.shape[2]
    out = []
    for l in range(NL):
        b, q, t = idx[0, l], idx[1, l], idx[2, l]
        cls = torch.full((B, Q), C, dtype=torch.int64, device=logits.device)
        cls[b, q] = labels.long()[t]
        cw = torch.ones((B, Q), dtype=logits.dtype, device=logits.device)
        cw[b, q] = weight.reshape(-1)[t].to(logits.dtype)
        x = logits[l]
        one = (cls[..., None] == torch.arange(C, device=logits.device)).to(logits.dtype)
        p = torch.sigmoid(x)
        sp = torch.nn.functional.softplus
        ce = one * sp(-x) + (1 - one) * sp(x)
        term = ce * (one * (1 - p) + (1 - one) * p) ** gamma
        if alpha >= 0:
            term = term * (alpha * one + (1 - alpha) * (1 - one))
        best = x.argmax(-1)
        if K:
            hit = (best[b, q] == labels.long()[t]).to(logits.dtype).sum()
            class_error = (K - hit) * 100.0 / K
        else:
            class_error = torch.tensor(100.0, dtype=logits.dtype, device=logits.device)
        card = (best != C - 1).to(logits.dtype).sum(1)
        card_error = (card - sizes.to(logits.dtype)).abs().mean()
        out.append(torch.stack([(term * cw[..., None]).sum(), class_error, card_error]))
    return torch.stack(out)


def depth_map_targets(boxes, depth, valid, weight, H, W):
    """Painting by the rule, box by box in slot order on the host's indices: -> (target depth [B, H, W] (0 without a box), foreground
    mask, weight of the deciding box (1 without one)).  boxes [B, N, 4] xyxy in pixels, floor / ceil to the integer box, sliced like
    ``canvas[v1:v2, u1:u2]``."""
    B, N = depth.shape
    inf = float("inf")
    nearest = torch.full((B, H, W), inf, dtype=depth.dtype)
    wmap = torch.ones((B, H, W), dtype=weight.dtype)
    fg = torch.zeros((B, H, W), dtype=torch.bool)
    bx, dp, vl, wt = boxes.detach().cpu(), depth.detach().cpu(), valid.cpu(), weight.detach().cpu()
    nearest, wmap = nearest.to(dp.dtype), wmap.to(wt.dtype)
    for b in range(B):
        for i in range(N):
            if not bool(vl[b, i]):
                continue
            u1, v1 = int(np.floor(float(bx[b, i, 0]))), int(np.floor(float(bx[b, i, 1])))
            u2, v2 = int(np.ceil(float(bx[b, i, 2]))), int(np.ceil(float(bx[b, i, 3])))
            cover = torch.zeros((H, W), dtype=torch.bool)
            cover[v1:v2, u1:u2] = True
            take = cover & ((dp[b, i] < nearest[b]) | (~fg[b] & (dp[b, i] == nearest[b])))
            nearest[b][take] = dp[b, i]
            wmap[b][take] = wt[b, i]
            fg[b] |= cover
    return torch.where(fg, nearest, torch.zeros((), dtype=dp.dtype)), fg, wmap


def depth_map_loss(logits, boxes, depth, valid, weight, alpha=0.25, gamma=2.0, fg_weight=13.0, bg_weight=1.0, depth_min=1e-3,
                   depth_max=60.0, eps=1e-6):
    """The weighted depth-map loss of logits [B, C, H, W] (any strides) against padded boxes; also returns the painted maps."""
    B, C, H, W = logits.shape
    num_bins = C - 1
    d, fg, wmap = depth_map_targets(boxes, depth, valid, weight, H, W)
    d, fg, wmap = d.to(logits.device), fg.to(logits.device), wmap.to(device=logits.device, dtype=logits.dtype)
    bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
    pos = -0.5 + 0.5 * torch.sqrt(1 + 8 * (d.double() - depth_min) / bin_size)
    bad = (pos < 0) | (pos > num_bins) | ~torch.isfinite(pos)
    bins = torch.where(bad, torch.full_like(pos, num_bins), pos).long()
    logp = torch.log_softmax(logits, dim=1)
    p = logp.exp()
    one = (bins.unsqueeze(1) == torch.arange(C, device=logits.device).view(1, C, 1, 1)).to(logits.dtype)
    pixel = ((one + eps) * (-alpha * (1 - p) ** gamma * logp)).sum(1)
    factor = torch.where(fg, fg_weight * wmap, torch.full_like(wmap, bg_weight))
    return (pixel * factor).sum() / (B * H * W), (bins, fg, wmap)


def padded_depth_map_inputs(targets, map_wh, dtype):
    """The criterion's padded depth-map inputs from per-image target dicts (with 'label_weight'): boxes [B, N, 4] xyxy in depth-map
    pixels from the cxcywh 'boxes', depth, valid, weight."""
    w, h = map_wh
    sizes = [len(t["labels"]) for t in targets]
    N = max(max(sizes, default=0), 1)
    B = len(targets)
    boxes = torch.zeros((B, N, 4), dtype=dtype)
    depth, weight = torch.zeros((B, N), dtype=dtype), torch.ones((B, N), dtype=dtype)
    valid = torch.zeros((B, N), dtype=torch.bool)
    scale = torch.tensor([w, h, w, h], dtype=dtype)
    for b, t in enumerate(targets):
        n = sizes[b]
        c = t["boxes"].detach().cpu().to(dtype) * scale
        boxes[b, :n] = torch.stack([c[:, 0] - 0.5 * c[:, 2], c[:, 1] - 0.5 * c[:, 3], c[:, 0] + 0.5 * c[:, 2], c[:, 1] + 0.5 * c[:, 3]], 1)
        depth[b, :n] = t["depth"].detach().cpu().to(dtype).reshape(-1)
        weight[b, :n] = t["label_weight"].detach().cpu().to(dtype).reshape(-1)
        valid[b, :n] = True
    return boxes, depth, valid, weight


def criterion_losses(outputs, targets, idx, n_boxes, alpha, map_wh, gamma=2.0):
    """The weighted criterion's loss dictionary (every key but the disabled loss_tfl / loss_mask) from the matched triples ``idx``;
    ``targets`` carry 'label_weight'.  Suffix '' for the final layer, '_i' for auxiliary layer i."""
    st, ft = CR.stack_layers(outputs), CR.flat_targets(targets)
    w = torch.cat([t["label_weight"] for t in targets], 0)
    dt, dev = st["pred_boxes"].dtype, st["pred_boxes"].device
    sizes = torch.tensor([len(t["labels"]) for t in targets], dtype=dt, device=dev)
    six = matched_sums(st["pred_boxes"], st["pred_depth"], st["pred_3d_dim"], st["pred_angle"], idx, ft["boxes_3d"], ft["depth"],
                       ft["size_3d"], ft["heading_bin"], ft["heading_res"], w) / n_boxes
    foc = focal_sums(st["pred_logits"], idx, ft["labels"], sizes, w, alpha, gamma)
    out = {}
    for l in range(idx.shape[1]):
        s = "" if l == 0 else "_%d" % (l - 1)
        out["loss_ce" + s] = foc[l, 0] / n_boxes
        out["class_error" + s], out["cardinality_error" + s] = foc[l, 1], foc[l, 2]
        for j, k in enumerate(LOSS6):
            out[k + s] = six[l, j]
    pb, pd, pv, pw = padded_depth_map_inputs(targets, map_wh, dt)
    out["loss_depth_map"], _ = depth_map_loss(outputs["pred_depth_map_logits"], pb, pd, pv, pw)
    return out


def with_weights(targets, weights):
    """per-image target dicts with 'label_weight' sliced from the flat ``weights`` [T]"""
    out, start = [], 0
    for t in targets:
        n = len(t["labels"])
        out.append(dict(t, label_weight=weights[start:start + n].clone()))
        start += n
    return out
