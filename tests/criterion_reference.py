"""An independent evaluation of MonoDETR's set criterion from GIVEN matched triples, for use as a float64 reference.

``matched_sums`` / ``focal_sums`` / ``criterion_losses`` are plain PyTorch, dtype-agnostic and differentiable by autograd,
written from the formulas (header of csrc/matched_losses.hip; the ``loss_*`` methods of monodetr/criterion.py name the lines
of the reference) without calling any part of ``SetCriterion``.  tests/test_criterion_reference.py pins them to the
layer-by-layer, image-by-image formulation (``SetCriterion(fast=False)``) in float64 on the CPU; the GPU tests then use
them as the reference of the HIP kernels.

The generators return float32 tensors; a float64 run casts the same values up, so both precisions see identical inputs.
``census`` returns, from a float64 evaluation, the geometry class of every matched pair and the smallest magnitude of every
quantity whose SIGN selects a branch of the loss (or of its hand-derived gradient): a float32 and a float64 run are only
comparable when both take the same side everywhere.

Keeping the branch quantities away from zero.  Box components are placed on a grid of step H = 2**-14 with fixed residues
modulo 4: target components = 0, prediction centres = 1, prediction l / r / t / b = 2 (a zero-area prediction keeps
l = r = t = b = 0).  Then every prediction-minus-target component is = 1 or 2 (mod 4), every prediction corner cx -+ l is
= 3 (a zero-area prediction's: 1) and every target corner = 0, so no component difference and no corner difference between
a prediction and ANY target can be smaller than H = 6.1e-5 -- whatever pairs a matcher forms -- and all of these numbers, and
their sums and differences, are exact in float32 (14 fractional bits).  Depths, sizes and heading residuals of the layout
generator use the same odd / even scheme on their own grids.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

H = 2.0 ** -14
LOSS6 = ("loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim", "loss_angle")
PRED_KEYS = ("pred_logits", "pred_boxes", "pred_3d_dim", "pred_depth", "pred_angle")
CLASSES = ("partial", "disjoint_x", "disjoint_y", "disjoint_xy", "pred_inside", "target_inside", "zero_pred", "zero_target")
# the smallest magnitude a branch-selecting quantity may have in any test case (about 16 float32 ulps at 0.5)
MARGIN = 1e-6


# ----------------------------------------------------------------------------------------------------------------- formulas
def _xyxy(box):
    cx, cy, l, r, t, b = box.unbind(-1)
    return cx - l, cy - t, cx + r, cy + b


def _giou(a, b):
    """GIoU of matched boxes given as corner tuples (x0, y0, x1, y1), and the clamped-before quantities (iw, ih)."""
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    iw = torch.min(a[2], b[2]) - torch.max(a[0], b[0])
    ih = torch.min(a[3], b[3]) - torch.max(a[1], b[1])
    inter = iw.clamp(min=0) * ih.clamp(min=0)
    union = area_a + area_b - inter
    cw = (torch.max(a[2], b[2]) - torch.min(a[0], b[0])).clamp(min=0)
    ch = (torch.max(a[3], b[3]) - torch.min(a[1], b[1])).clamp(min=0)
    hull = cw * ch
    return inter / union - (hull - union) / hull, iw, ih


def _gather(pred, idx):
    """pred [NL, B, Q, D], idx [3, NL, K] -> the matched rows [NL, K, D]"""
    NL, K = idx.shape[1:]
    lay = torch.arange(NL, device=pred.device).view(NL, 1).expand(NL, K)
    return pred[lay, idx[0], idx[1]]


def matched_sums(boxes, depth, dims, angle, idx, t_box, t_depth, t_size, t_bin, t_res):
    """-> [NL, 6]: per decoder layer the SUMS over the matched pairs of {3D-centre L1, l/r/t/b L1, 1 - GIoU, Laplacian
    aleatoric depth loss, dimension-aware size loss times the detached compensation mean|s-s*| / mean(|s-s*| / s*),
    12-bin heading cross entropy + L1 of the target bin's residual}.  Predictions [NL, B, Q, 6|2|3|24], idx [3, NL, K]
    (image, query, flat target), targets [T, 6], [T], [T, 3], [T] int64, [T]."""
    NL, K = idx.shape[1:]
    t = idx[2]
    pb, tb = _gather(boxes, idx), t_box[t]
    center = (pb[..., 0:2] - tb[..., 0:2]).abs().sum((1, 2))
    bbox = (pb[..., 2:6] - tb[..., 2:6]).abs().sum((1, 2))
    g, _, _ = _giou(_xyxy(pb), _xyxy(tb))
    giou = (1 - g).sum(1)
    pd, td = _gather(depth, idx), t_depth.reshape(-1)[t]
    dep = (1.4142 * torch.exp(-pd[..., 1]) * (pd[..., 0] - td).abs() + pd[..., 1]).sum(1)
    ps, ts = _gather(dims, idx), t_size[t]
    l1 = (ps - ts).abs()
    rel = l1 / ts
    comp = (l1.mean((1, 2)) / rel.mean((1, 2))).detach() if K else torch.ones(NL, dtype=boxes.dtype, device=boxes.device)
    dim = rel.sum((1, 2)) * comp
    pa = _gather(angle, idx)
    bins = t_bin.reshape(-1)[t].long()
    logp = torch.log_softmax(pa[..., 0:12], dim=-1)
    ce = -torch.gather(logp, 2, bins.unsqueeze(-1)).squeeze(-1)
    res = torch.gather(pa[..., 12:24], 2, bins.unsqueeze(-1)).squeeze(-1)
    ang = (ce + (res - t_res.reshape(-1)[t]).abs()).sum(1)
    return torch.stack([center, bbox, giou, dep, dim, ang], 1)


def class_map(idx, labels, NL, B, Q, C):
    """[NL, B, Q] int64: the class of the target a query is matched to, C ("no object") elsewhere"""
    K = idx.shape[2]
    out = torch.full((NL, B, Q), C, dtype=torch.int64, device=idx.device)
    lay = torch.arange(NL, device=idx.device).view(NL, 1).expand(NL, K)
    out[lay, idx[0], idx[1]] = labels.long()[idx[2]]
    return out


def focal_sums(logits, idx, labels, sizes, alpha, gamma=2.0):
    """-> [NL, 3]: {sigmoid focal loss SUMMED over (image, query, class) against the matched one-hot map (alpha < 0: no
    alpha weighting), class_error = 100 - top-1 accuracy of the matched queries in %, cardinality_error = mean over images
    of |#(queries whose arg-max is not the last class) - #targets|}.  logits [NL, B, Q, C], sizes [B]."""
    NL, B, Q, C = logits.shape
    K = idx.shape[2]
    cls = class_map(idx, labels, NL, B, Q, C)
    one = (cls.unsqueeze(-1) == torch.arange(C, device=logits.device)).to(logits.dtype)
    p = torch.sigmoid(logits)
    ce = -(one * F.logsigmoid(logits) + (1 - one) * F.logsigmoid(-logits))
    q = one * (1 - p) + (1 - one) * p                                        # 1 - p_t
    term = ce * q ** gamma
    if alpha >= 0:
        term = term * (alpha * one + (1 - alpha) * (1 - one))
    best = logits.argmax(-1)                                                  # first maximum
    if K:
        hit = (_gather(best.unsqueeze(-1), idx).squeeze(-1) == labels.long()[idx[2]]).to(logits.dtype).sum(1)
        class_error = (K - hit) * 100.0 / K                                   # not 100 - 100 * hit / K, which cancels
    else:
        class_error = torch.full((NL,), 100.0, dtype=logits.dtype, device=logits.device)
    card = (best != C - 1).to(logits.dtype).sum(2)
    card_error = (card - sizes.to(logits.dtype).view(1, B)).abs().mean(1)
    return torch.stack([term.sum((1, 2, 3)), class_error, card_error], 1)


def stack_layers(outputs):
    """criterion outputs (final layer + 'aux_outputs') -> {key: [NL, B, Q, D]}, layer 0 = the final layer"""
    layers = [{k: v for k, v in outputs.items() if k != "aux_outputs"}] + list(outputs.get("aux_outputs", []))
    return {k: torch.stack([o[k] for o in layers]) for k in PRED_KEYS}


def flat_targets(targets):
    keys = ("labels", "boxes_3d", "depth", "size_3d", "heading_bin", "heading_res")
    return {k: torch.cat([t[k] for t in targets], 0) for k in keys}


def criterion_losses(outputs, targets, idx, num_boxes, alpha, gamma=2.0):
    """The criterion's loss dictionary (every key but loss_depth_map and the disabled loss_tfl / loss_mask) from the matched
    triples ``idx``; suffix '' for the final layer, '_i' for auxiliary layer i."""
    st, ft = stack_layers(outputs), flat_targets(targets)
    sizes = torch.tensor([len(t["labels"]) for t in targets], dtype=st["pred_boxes"].dtype, device=idx.device)
    six = matched_sums(st["pred_boxes"], st["pred_depth"], st["pred_3d_dim"], st["pred_angle"], idx, ft["boxes_3d"], ft["depth"],
                       ft["size_3d"], ft["heading_bin"], ft["heading_res"]) / num_boxes
    foc = focal_sums(st["pred_logits"], idx, ft["labels"], sizes, alpha, gamma)
    out = {}
    for l in range(idx.shape[1]):
        s = "" if l == 0 else "_%d" % (l - 1)
        out["loss_ce" + s] = foc[l, 0] / num_boxes
        out["class_error" + s], out["cardinality_error" + s] = foc[l, 1], foc[l, 2]
        for j, k in enumerate(LOSS6):
            out[k + s] = six[l, j]
    return out


# ------------------------------------------------------------------------------------------------------------------ census
@torch.no_grad()
def census(boxes, depth, dims, angle, idx, t_box, t_depth, t_size, t_bin, t_res):
    """From a float64 evaluation: ``classes`` [NL, K] (index into CLASSES) and ``margins`` {name: smallest magnitude over all
    pairs} of the quantities whose sign selects a branch: iw, ih (intersection extents before the clamp), the four corner
    differences, the six box-component differences, d - d*, s - s*, residual - residual*."""
    f = lambda x: x.double()
    t = idx[2]
    pb, tb = _gather(f(boxes), idx), f(t_box)[t]
    a, b = _xyxy(pb), _xyxy(tb)
    _, iw, ih = _giou(a, b)
    zero_t = (tb[..., 2:6] == 0).all(-1)
    zero_p = (pb[..., 2:6] == 0).all(-1)
    inside = (a[0] > b[0]) & (a[1] > b[1]) & (a[2] < b[2]) & (a[3] < b[3])
    around = (a[0] < b[0]) & (a[1] < b[1]) & (a[2] > b[2]) & (a[3] > b[3])
    cls = torch.zeros(iw.shape, dtype=torch.int64, device=iw.device)                       # partial
    cls[(iw <= 0) & (ih > 0)] = 1
    cls[(iw > 0) & (ih <= 0)] = 2
    cls[(iw <= 0) & (ih <= 0)] = 3
    cls[inside] = 4
    cls[around] = 5
    cls[zero_p] = 6
    cls[zero_t] = 7
    bins = t_bin.reshape(-1)[t].long()
    res = torch.gather(_gather(f(angle), idx)[..., 12:24], 2, bins.unsqueeze(-1)).squeeze(-1)
    smallest = lambda x: float(x.abs().min()) if x.numel() else float("inf")
    margins = {"iw": smallest(iw), "ih": smallest(ih),
               "corners": smallest(torch.stack([a[k] - b[k] for k in range(4)])),
               "box": smallest(pb - tb),
               "depth": smallest(_gather(f(depth), idx)[..., 0] - f(t_depth).reshape(-1)[t]),
               "size": smallest(_gather(f(dims), idx) - f(t_size)[t]),
               "residual": smallest(res - f(t_res).reshape(-1)[t])}
    return cls, margins


def class_shares(cls):
    """{class name: share of the pairs}, plus 'disjoint' = the three classes without an intersection"""
    n = max(cls.numel(), 1)
    shares = {name: float((cls == i).sum()) / n for i, name in enumerate(CLASSES)}
    shares["disjoint"] = shares["disjoint_x"] + shares["disjoint_y"] + shares["disjoint_xy"]
    return shares


def row_error(g, ref, width=None):
    """The gradient metric of these tests: the MAXIMUM over all rows of ||g_row - ref_row|| / max(||ref_row||, floor), a row
    being the last dimension (one (layer, image, query) slice of a prediction tensor), floor = 1e-4 * the largest row norm of
    ``ref``.  The floor: float32 under-flows where float64 does not (a logit of -90 has a float64 gradient of 1e-39), and a row
    four orders of magnitude below the largest cannot change a float32 weight update.  Same for every run compared."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    g, ref = g.reshape(-1, g.shape[-1]), ref.reshape(-1, ref.shape[-1])
    norms = ref.norm(dim=1)
    floor = 1e-4 * float(norms.max()) if norms.numel() else 0.0
    if floor == 0.0:
        return float((g - ref).norm(dim=1).max()) if g.numel() else 0.0       # an all-zero reference: any non-zero is an error
    return float(((g - ref).norm(dim=1) / norms.clamp_min(floor)).max())


# -------------------------------------------------------------------------------------------------------------- generators
def _grid(x, step, residue, mod):
    """x -> the nearest multiple k * step with k = residue (mod ``mod``)"""
    return (np.round((np.asarray(x, np.float64) / step - residue) / mod) * mod + residue) * step


def _span(rng, lo, w, kind, s):
    """One axis of a prediction box relative to the target interval [lo, lo + w]: -> (p0, p1).  kind: 0 partial overlap,
    1 disjoint, 2 prediction strictly inside, 3 target strictly inside, 4 a point beside the interval; s = +-1 picks the side."""
    n = lo.shape[0]
    u0, u1 = rng.uniform(0.2, 0.8, n), rng.uniform(0.2, 0.8, n)
    hi = lo + w
    part = (lo + s * u0 * w, hi + s * u1 * w)
    right = hi + u0 * w
    left = lo - u0 * w
    disj = (np.where(s > 0, right, left - (0.5 + u1) * w), np.where(s > 0, right + (0.5 + u1) * w, left))
    ins = (lo + 0.5 * u0 * w, hi - 0.5 * u1 * w)
    out = (lo - 0.5 * u0 * w, hi + 0.5 * u1 * w)
    pt = np.where(s > 0, right, left)
    p0 = np.choose(kind, [part[0], disj[0], ins[0], out[0], pt])
    p1 = np.choose(kind, [part[1], disj[1], ins[1], out[1], pt])
    return p0, p1


# per geometry class: the kind of the x axis and of the y axis for _span
_AXES = {0: (0, 0), 1: (1, 0), 2: (0, 1), 3: (1, 1), 4: (2, 2), 5: (3, 3), 6: (4, 4)}


def make_matched_case(seed, NL, B, Q, K):
    """Inputs of the matched-pair kernels with every geometry class of CLASSES built on purpose (an eighth of the pairs each,
    so three eighths are disjoint) and the other heads at their edges.  Triples are unique per (layer, image, query) and
    differ between layers; T = K targets, every layer pairs them with other queries.  -> dict of float32 / int64 CPU tensors."""
    assert K <= B * Q
    rng = np.random.default_rng(seed)
    T = K
    zero_t = (np.arange(T) % 8 == 7) if T >= 8 else np.zeros(T, bool)
    tb = np.concatenate([rng.uniform(0.25, 0.75, (T, 2)), rng.uniform(0.02, 0.1, (T, 4))], 1)
    tb[zero_t, 2:] = 0
    tb = _grid(tb, H, 0, 4)
    t_depth = _grid(rng.uniform(1, 60, T), 2.0 ** -9, 0, 1)
    t_size = np.exp(rng.uniform(math.log(0.3), math.log(12.0), (T, 3))).astype(np.float32)
    t_size[0, 0], t_size[T - 1, 1] = 0.3, 12.0
    t_bin = rng.integers(0, 12, T)
    t_bin[0], t_bin[T - 1] = (0, 11) if T > 1 else (t_bin[0], t_bin[0])
    t_res = rng.uniform(-math.pi / 12, math.pi / 12, T).astype(np.float32)

    boxes = rng.uniform(0, 1, (NL, B, Q, 6))
    depth = rng.standard_normal((NL, B, Q, 2)) * 3
    dims = rng.standard_normal((NL, B, Q, 3)) + 2
    angle = rng.standard_normal((NL, B, Q, 24))
    angle[..., :12] *= 20                                                  # saturated soft-max
    idx = np.zeros((3, NL, K), np.int64)
    for l in range(NL):
        cells = rng.permutation(B * Q)[:K]
        t = rng.permutation(T)
        b, q = cells // Q, cells % Q
        idx[:, l] = b, q, t
        cls = np.where(zero_t[t], 7, (np.arange(K) + l) % 7)
        # ---- boxes: the prediction's corners relative to its target's
        x0, y0 = tb[t, 0] - tb[t, 2], tb[t, 1] - tb[t, 4]
        w, h = tb[t, 2] + tb[t, 3], tb[t, 4] + tb[t, 5]
        kx = np.array([_AXES.get(c, (0, 0))[0] for c in cls])
        ky = np.array([_AXES.get(c, (0, 0))[1] for c in cls])
        sx, sy = rng.choice([-1.0, 1.0], K), rng.choice([-1.0, 1.0], K)
        px0, px1 = _span(rng, x0, w, kx, sx)
        py0, py1 = _span(rng, y0, h, ky, sy)
        # a zero-area target (a point): a proper prediction diagonally beside it
        z = cls == 7
        ex, ey = 0.02 + 0.06 * rng.uniform(size=K), 0.02 + 0.06 * rng.uniform(size=K)
        wx, wy = 0.04 + 0.1 * rng.uniform(size=K), 0.04 + 0.1 * rng.uniform(size=K)
        px0 = np.where(z, np.where(sx > 0, tb[t, 0] + ex, tb[t, 0] - ex - wx), px0)
        px1 = np.where(z, px0 + wx, px1)
        py0 = np.where(z, np.where(sy > 0, tb[t, 1] + ey, tb[t, 1] - ey - wy), py0)
        py1 = np.where(z, py0 + wy, py1)
        vx, vy = rng.uniform(0.2, 0.8, K), rng.uniform(0.2, 0.8, K)
        cx, cy = px0 + vx * (px1 - px0), py0 + vy * (py1 - py0)
        lrtb = np.stack([cx - px0, px1 - cx, cy - py0, py1 - cy], 1)
        pred = np.concatenate([_grid(np.stack([cx, cy], 1), H, 1, 4), _grid(lrtb, H, 2, 4)], 1)
        pred[cls == 6, 2:] = 0
        boxes[l, b, q] = pred
        # ---- depth: log-variance over [-8, 8], |d - d*| from 1e-3 to 60, both signs
        delta = np.maximum(_grid(np.exp(rng.uniform(math.log(1e-3), math.log(60.0), K)), 2.0 ** -10, 0, 1), 2.0 ** -10)
        delta[0] = 2.0 ** -10
        delta[K - 1] = 60.0 if K > 1 else delta[0]
        sd = rng.choice([-1.0, 1.0], K)
        lv = rng.uniform(-8, 8, K)
        lv[0], lv[K - 1] = (-8.0, 8.0) if K > 1 else (-8.0, -8.0)
        depth[l, b, q, 0], depth[l, b, q, 1] = t_depth[t] + sd * delta, lv
        # ---- sizes and the target bin's residual: off the target by 0.01 .. 1, both signs
        dims[l, b, q] = t_size[t] + rng.choice([-1.0, 1.0], (K, 3)) * rng.uniform(0.01, 1.0, (K, 3))
        angle[l, b, q, 12 + t_bin[t]] = t_res[t] + rng.choice([-1.0, 1.0], K) * rng.uniform(0.01, 1.0, K)
    f32 = lambda x: torch.from_numpy(np.asarray(x, np.float32))
    return {"boxes": f32(boxes), "depth": f32(depth), "dims": f32(dims), "angle": f32(angle), "idx": torch.from_numpy(idx),
            "t_box": f32(tb), "t_depth": f32(t_depth), "t_size": f32(t_size), "t_bin": torch.from_numpy(t_bin.astype(np.int64)),
            "t_res": f32(t_res)}


MATCHED_ARGS = ("boxes", "depth", "dims", "angle", "idx", "t_box", "t_depth", "t_size", "t_bin", "t_res")

# planted logit rows: p rounds to 0 / 1 in float32 (+-30, +-90), and exact arg-max ties (first maximum wins; a tie with the
# last class counts the query as an object)
_EXTREME_ROWS = ((30., -30., 90.), (-90., -90., -90.), (90., -30., 30.), (-30., 30., -90.), (-90., 90., -30.), (30., 30., 30.))
_TIE_ROWS = ((2.5, 2.5, 1.0), (1.0, 3.0, 3.0), (0.5, 0.5, 0.5), (-1.0, 2.0, 2.0), (4.0, -2.0, 4.0), (-3.0, -3.0, -5.0))


def make_focal_case(seed, NL, B, Q, sizes, groups=1, C=3):
    """Inputs of the focal kernels: logits N(0, 3) with the planted rows above on matched and on unmatched queries, labels 0..C-1
    all present, ``sizes[b]`` targets in image b each matched by ``groups`` queries, other queries per layer."""
    assert C == 3 and len(sizes) == B and groups * max(sizes) <= Q
    rng = np.random.default_rng(seed)
    T = int(sum(sizes))
    labels = rng.permutation(np.arange(T) % C)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    logits = (rng.standard_normal((NL, B, Q, C)) * 3).astype(np.float32)
    planted = np.array(_EXTREME_ROWS + _TIE_ROWS, np.float32)
    per_layer = []
    for l in range(NL):
        bs, qs, ts = [], [], []
        for b in range(B):
            n = groups * sizes[b]
            qs.append(rng.permutation(Q)[:n])
            bs.append(np.full(n, b))
            ts.append(offs[b] + np.tile(np.arange(sizes[b]), groups))
        tri = np.stack([np.concatenate(bs), np.concatenate(qs), np.concatenate(ts)]).astype(np.int64)
        per_layer.append(tri)
        K = tri.shape[1]
        for j in range(min(K, 2 * len(planted))):                          # on matched queries (every other pair)
            k = (j * 2 + l) % K
            logits[l, tri[0, k], tri[1, k]] = planted[j % len(planted)]
        cells = rng.permutation(B * Q)[:4 * len(planted)]                    # and anywhere
        for j, c in enumerate(cells):
            logits[l, c // Q, c % Q] = planted[j % len(planted)]
    idx = np.stack(per_layer, 1)
    return {"logits": torch.from_numpy(logits), "idx": torch.from_numpy(idx), "labels": torch.from_numpy(labels.astype(np.int64)),
            "sizes": torch.tensor(sizes, dtype=torch.float32)}


def _off_bin_edges(d):
    """depths moved off the edges of the depth map's LID bins (monodetr/losses.py lid_bin_indices, 80 bins over 1e-3 .. 60),
    so that float32 and float64 bin them alike"""
    bin_size = 2 * (60 - 1e-3) / (80 * 81)
    pos = -0.5 + 0.5 * np.sqrt(1 + 8 * (d - 1e-3) / bin_size)
    near = np.abs(pos - np.round(pos)) < 2e-2
    return np.where(near, d + 2.0 ** -5, d)


def make_layout_case(seed, sizes, Q, NL=3, map_hw=(24, 80)):
    """A KITTI-like batch for the whole criterion: ``sizes[b]`` targets in image b (0 .. 50) with mixed labels, small boxes
    (centres U(0.1, 0.9), l / r / t / b U(0.01, 0.1)); predictions of NL layers whose boxes are as small, half of them scattered
    around the image's targets and half anywhere, so that a matcher forms overlapping and disjoint pairs.  Every quantity whose
    sign selects a branch sits on the odd / even grids described at the top of the file.
    -> (outputs with 'aux_outputs' and 'pred_depth_map_logits', list of per-image target dicts), float32 / int64 CPU tensors."""
    rng = np.random.default_rng(seed)
    B = len(sizes)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))
    targets, centres = [], []
    for n in sizes:
        c, lrtb = rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.01, 0.1, (n, 4))
        b3 = _grid(np.concatenate([c, lrtb], 1), H, 0, 4)
        x0, x1, y0, y1 = b3[:, 0] - b3[:, 2], b3[:, 0] + b3[:, 3], b3[:, 1] - b3[:, 4], b3[:, 1] + b3[:, 5]
        depth = _grid(_off_bin_edges(_grid(rng.uniform(5, 60, n), 2.0 ** -10, 0, 2)), 2.0 ** -10, 0, 2)
        targets.append({"labels": torch.from_numpy((rng.permutation(n) % 3).astype(np.int64)),
                        "boxes_3d": f32(b3), "boxes": f32(np.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], 1)),
                        "depth": f32(depth.reshape(n, 1)), "size_3d": f32(_grid(rng.uniform(0.5, 4.0, (n, 3)), 2.0 ** -8, 0, 2)),
                        "heading_bin": torch.from_numpy(rng.integers(0, 12, (n, 1)).astype(np.int64)),
                        "heading_res": f32(_grid(rng.uniform(-math.pi / 12, math.pi / 12, (n, 1)), 2.0 ** -12, 0, 2))})
        centres.append(b3[:, :2])

    def layer():
        c = rng.uniform(0.1, 0.9, (B, Q, 2))
        for b, n in enumerate(sizes):
            if n:
                near = rng.permutation(Q)[:Q // 2]
                c[b, near] = centres[b][rng.integers(0, n, near.size)] + 0.04 * rng.standard_normal((near.size, 2))
        boxes = np.concatenate([_grid(c, H, 1, 4), _grid(rng.uniform(0.01, 0.1, (B, Q, 4)), H, 2, 4)], 2)
        depth = np.stack([_grid(rng.uniform(5, 60, (B, Q)), 2.0 ** -10, 1, 2), rng.uniform(-2, 2, (B, Q))], 2)
        angle = rng.standard_normal((B, Q, 24)) * 2
        angle[..., 12:] = _grid(0.3 * rng.standard_normal((B, Q, 12)), 2.0 ** -12, 1, 2)
        return {"pred_logits": f32(rng.standard_normal((B, Q, 3)) * 2), "pred_boxes": f32(boxes),
                "pred_3d_dim": f32(_grid(rng.uniform(0.5, 4.0, (B, Q, 3)), 2.0 ** -8, 1, 2)), "pred_depth": f32(depth),
                "pred_angle": f32(angle)}
    outputs = layer()
    outputs["aux_outputs"] = [layer() for _ in range(NL - 1)]
    outputs["pred_depth_map_logits"] = f32(rng.standard_normal((B, 81) + tuple(map_hw)))
    return outputs, targets


def cast_case(outputs, targets, device, dtype, requires_grad=True):
    """the generator's tensors on ``device`` in ``dtype`` (integers stay), predictions as fresh leaves"""
    leaf = lambda v: v.to(device=device, dtype=dtype).requires_grad_(requires_grad)
    out = {k: leaf(v) for k, v in outputs.items() if k != "aux_outputs"}
    out["aux_outputs"] = [{k: leaf(v) for k, v in o.items()} for o in outputs["aux_outputs"]]
    tg = [{k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)) for k, v in t.items()} for t in targets]
    return out, tg


def leaves_of(outputs):
    """{name: leaf}: 'l<layer>.<key>' for every prediction tensor (layer 0 = the final one) and 'depth_map_logits'"""
    layers = [outputs] + list(outputs["aux_outputs"])
    named = {"l%d.%s" % (l, k): o[k] for l, o in enumerate(layers) for k in PRED_KEYS}
    named["depth_map_logits"] = outputs["pred_depth_map_logits"]
    return named
