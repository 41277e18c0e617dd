"""Duplicate suppression and flip-view fusion of decoded KITTI rows (``tester.nms_iou`` / ``tester.flip_tta`` / ``tester.fuse``).

    fuse_config(tester_cfg)                  -> None (keys absent) or (iou, flip_tta, mode); raises ValueError on a bad key
    fuse_rows_device(rows, count, geom, ...) one launch of mono_fuse_dets_f64 (include/monosowa_kitti.h) on the current stream
    fuse_rows_host(rows, count, geom, ...)   the same contract in float64 numpy (the CPU device, and V * K > MAX_CANDIDATES)
    unmirror_rows(rows, geom_row)            rows decoded from the mirrored frame, brought back into the frame

The contract (include/monosowa_kitti.h has it in full).  ``rows`` float64 ``[V * B, K, 14]`` and ``count`` ``[V * B]`` are
``mono_decode_dets_f64``'s output with view ``v`` of image ``b`` at index ``v * B + b``; view 1 is the mirrored frame, decoded with
the image's own geometry row.  The candidates of an image -- id ``j`` for view 0, ``K + j`` for the un-mirrored view 1 -- are walked
by score descending (exact ties: lower id first; NaN last); a candidate joins the first seed of its class whose BEV rectangle
``(x, z, l, w, ry)`` it overlaps by ``IoU >= iou``, else it becomes a seed.  Output: a row per seed in seed order (``'seed'``: the
seed's row; ``'mean'``: the score-weighted mean of the members, the score averaged over the views so that a detection the other
view does not confirm keeps half of it), ``count`` per image and ``support`` = members per cluster.

The host function clips the rectangles in float64 (one rectangle's corners in the other's frame, clipped against its four sides)
where the kernel runs the evaluation's float32 routine: the two agree on every pair whose IoU is not within the float32 routine's
error of the threshold (the routine clips the same way, in float32).  On degenerate input both follow one rule: a rectangle with a
side that is not > 0 overlaps nothing, and two rectangles with the same five float32 numbers overlap by 1.
"""
import numpy as np
import torch

MODES = {"seed": 0, "mean": 1}
MAX_CANDIDATES = 256          # V * K of one image in the kernel (csrc/fuse_dets.h)
ROW = 14
_PI, _TWO_PI = 3.141592653589793, 2 * 3.141592653589793


def fuse_config(tester_cfg):
    """The three keys of ``cfg["tester"]`` -> None when all are absent / off, else ``(iou, flip_tta, mode)``."""
    iou, flip, mode = tester_cfg.get("nms_iou"), tester_cfg.get("flip_tta"), tester_cfg.get("fuse", "seed")
    if mode not in MODES:
        raise ValueError("tester.fuse must be 'seed' or 'mean', got %r" % (mode,))
    if flip is not None and not isinstance(flip, bool):
        raise ValueError("tester.flip_tta must be true or false, got %r" % (flip,))
    if iou is None or (not isinstance(iou, bool) and isinstance(iou, (int, float)) and iou == 0):
        iou = None
    elif isinstance(iou, bool) or not isinstance(iou, (int, float)) or not 0.0 < float(iou) <= 1.0:
        raise ValueError("tester.nms_iou must be a number in (0, 1] (absent or 0: off), got %r" % (iou,))
    if flip and iou is None:
        raise ValueError("tester.flip_tta needs tester.nms_iou: the two views are paired by that overlap")
    return None if iou is None else (float(iou), bool(flip), mode)


def _wrap(a):
    a = np.where(a > _PI, a - _TWO_PI, a)
    return np.where(a < -_PI, a + _TWO_PI, a)


def unmirror_rows(rows, geom_row):
    """Rows ``[n, 14]`` decoded from the mirrored frame (u -> W - u, calibration unchanged) -> the same rows in the frame."""
    rows = np.array(rows, dtype=np.float64).reshape(-1, ROW)
    W, cu, fu, tx = (np.float64(geom_row[k]) for k in (0, 4, 6, 8))
    with np.errstate(invalid="ignore"):
        x1, x2 = W - rows[:, 4], W - rows[:, 2]
        alpha = _wrap(_PI - rows[:, 1])
        rows[:, 9] = ((W - 2 * cu) * rows[:, 11]) / fu - rows[:, 9] + 2 * tx
        rows[:, 12] = _wrap(alpha + np.arctan2((x1 + x2) / 2 - cu, fu))
        rows[:, 1], rows[:, 2], rows[:, 4] = alpha, x1, x2
    return rows


def _clip(poly, normal, limit):
    """The part of a convex polygon (list of points) with ``normal . p <= limit``."""
    out = []
    for k, p in enumerate(poly):
        q = poly[(k + 1) % len(poly)]
        dp, dq = normal[0] * p[0] + normal[1] * p[1] - limit, normal[0] * q[0] + normal[1] * q[1] - limit
        if dp <= 0:
            out.append(p)
        if (dp <= 0) != (dq <= 0):
            t = dp / (dp - dq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def bev_iou(a, b):
    """IoU of two rectangles ``(cx, cy, w, h, angle)`` in float64: ``b``'s corners in ``a``'s frame, clipped against ``a``'s sides."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if not all(np.isfinite(a + b)) or not (a[2] > 0 and a[3] > 0 and b[2] > 0 and b[3] > 0):
        return float("nan")                                       # no polygon, or a rectangle without an area: never a match
    if a == b:
        return 1.0
    d = b[4] - a[4]                                           # corners of b, rotated clockwise by its angle, seen from a
    ca, sa, cd, sd = np.cos(a[4]), np.sin(a[4]), np.cos(d), np.sin(d)
    ox, oy = b[0] - a[0], b[1] - a[1]
    ox, oy = ca * ox - sa * oy, sa * ox + ca * oy
    poly = [(cd * x + sd * y + ox, -sd * x + cd * y + oy) for x, y in
            ((-b[2] / 2, -b[3] / 2), (-b[2] / 2, b[3] / 2), (b[2] / 2, b[3] / 2), (b[2] / 2, -b[3] / 2))]
    for normal, limit in (((1.0, 0.0), a[2] / 2), ((-1.0, 0.0), a[2] / 2), ((0.0, 1.0), a[3] / 2), ((0.0, -1.0), a[3] / 2)):
        poly = _clip(poly, normal, limit)
        if not poly:
            break
    inter = 0.0
    for k in range(len(poly)):
        p, q = poly[k], poly[(k + 1) % len(poly)]
        inter += p[0] * q[1] - q[0] * p[1]
    inter = abs(inter) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(inter) / np.float64(a[2] * a[3] + b[2] * b[3] - inter))


def candidate_order(score):
    """Indices by score descending, exact ties by lower index, NaN last in index order."""
    score = np.asarray(score, dtype=np.float64)
    nan = np.isnan(score)
    idx = np.arange(len(score))
    good = idx[~nan]
    return np.concatenate([good[np.argsort(-score[good], kind="stable")], idx[nan]]).astype(np.int64)


def fuse_image(cands, ids, K, geom_row, iou, mode, views):
    """One image: candidates ``[n, 14]`` in the frame with their ids -> (rows ``[seeds, 14]``, support ``[seeds]``)."""
    thr = np.float32(iou)
    order = candidate_order(cands[:, 13])
    boxes = cands[:, [9, 11, 8, 7, 12]].astype(np.float32).astype(np.float64)        # the kernel's rectangles are float32
    seeds, members = [], []
    for r in order:
        c = cands[r]
        home = None
        for s, q in enumerate(seeds):
            if cands[q, 0] == c[0] and np.float32(bev_iou(boxes[q], boxes[r])) >= thr:
                home = s
                break
        if home is None:
            seeds.append(r)
            members.append([r])
        else:
            members[home].append(r)
    out = np.zeros((len(seeds), ROW), dtype=np.float64)
    cu, fu = np.float64(geom_row[4]), np.float64(geom_row[6])
    for s, (q, mem) in enumerate(zip(seeds, members)):
        if mode == "seed":
            out[s] = cands[q]
            continue
        sw = ss = sc = np.float64(0.0)
        acc = np.zeros(10, dtype=np.float64)
        best = [None] * views
        with np.errstate(invalid="ignore", divide="ignore"):
            for m in mem:
                w = cands[m, 13]
                sw = sw + w
                acc = acc + w * cands[m, 2:12]
                ss, sc = ss + w * np.sin(cands[m, 12]), sc + w * np.cos(cands[m, 12])
                v = int(ids[m]) // K
                if best[v] is None:                                   # members come in score order: the first of a view is its best
                    best[v] = w
            acc = acc / sw
            ry = np.arctan2(ss, sc)
            out[s, 0], out[s, 2:12], out[s, 12] = cands[q, 0], acc, ry
            out[s, 1] = _wrap(ry - np.arctan2((acc[0] + acc[2]) / 2 - cu, fu))
            out[s, 13] = sum(np.float64(0.0 if w is None else w) for w in best) / views
    return out, np.array([len(m) for m in members], dtype=np.int32)


def fuse_rows_host(rows, count, geom, iou, mode="seed", views=1):
    """``mono_fuse_dets_f64``'s contract in numpy: rows ``[V * B, K, 14]``, count ``[V * B]``, geom ``[B, 10]`` -> out rows
    ``[B, V * K, 14]``, count int32 ``[B]``, support int32 ``[B, V * K]``."""
    rows, count, geom = np.asarray(rows, dtype=np.float64), np.asarray(count), np.asarray(geom, dtype=np.float64)
    _check_arguments(iou, mode, views)
    VB, K, _ = rows.shape
    B = VB // views
    if B * views != VB or count.shape != (VB,) or geom.shape[0] != B:
        raise ValueError("rows %s, count %s and geom %s do not describe %d view(s)" % (rows.shape, count.shape, geom.shape, views))
    out = np.zeros((B, views * K, ROW), dtype=np.float64)
    out_count, support = np.zeros(B, dtype=np.int32), np.zeros((B, views * K), dtype=np.int32)
    for b in range(B):
        cands, ids = [], []
        for v in range(views):
            n = int(min(max(count[v * B + b], 0), K))
            part = rows[v * B + b, :n]
            cands.append(unmirror_rows(part, geom[b]) if v else part.reshape(-1, ROW))
            ids.append(v * K + np.arange(n))
        got, sup = fuse_image(np.concatenate(cands), np.concatenate(ids), K, geom[b], iou, mode, views)
        out[b, :len(got)], support[b, :len(got)], out_count[b] = got, sup, len(got)
    return out, out_count, support


def _check_arguments(iou, mode, views):
    if mode not in MODES:
        raise ValueError("fuse mode must be 'seed' or 'mean', got %r" % (mode,))
    if views not in (1, 2):
        raise ValueError("fuse takes 1 or 2 views, got %r" % (views,))
    if not 0.0 < float(iou) <= 1.0:
        raise ValueError("the fuse overlap must lie in (0, 1], got %r" % (iou,))


def fuse_rows_device(rows, count, geom, iou, mode="seed", views=1, out_rows=None, out_count=None, out_support=None):
    """One launch of ``mono_fuse_dets_f64`` on the current stream: rows float64 ``[V * B, K, 14]``, count int32 ``[V * B]``, geom
    float64 ``[B, GEOM_DOUBLES]`` (contiguous CUDA tensors) -> out rows ``[B, V * K, 14]``, count int32 ``[B]``, support int32
    ``[B, V * K]``."""
    from .kitti_eval import GEOM_DOUBLES, load
    _check_arguments(iou, mode, views)
    if rows.dim() != 3 or rows.shape[2] != ROW or rows.dtype != torch.float64 or not rows.is_cuda or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float64 CUDA tensor [V * B, K, 14], got %s %s" % (rows.dtype, tuple(rows.shape)))
    VB, K, _ = rows.shape
    B = VB // views
    if B * views != VB or B == 0:
        raise ValueError("%d rows blocks do not hold %d view(s) per image" % (VB, views))
    if views * K > MAX_CANDIDATES:
        raise ValueError("the fuse kernel takes at most %d candidates per image, got %d x %d" % (MAX_CANDIDATES, views, K))
    for name, t, dtype, shape in (("count", count, torch.int32, (VB,)), ("geom", geom, torch.float64, (B, GEOM_DOUBLES))):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != rows.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor %s on %s, got %s %s on %s"
                             % (name, dtype, shape, rows.device, t.dtype, tuple(t.shape), t.device))
    if out_rows is None:
        out_rows = torch.empty((B, views * K, ROW), dtype=torch.float64, device=rows.device)
    if out_count is None:
        out_count = torch.empty((B,), dtype=torch.int32, device=rows.device)
    if out_support is None:
        out_support = torch.empty((B, views * K), dtype=torch.int32, device=rows.device)
    for name, t, dtype, shape in (("out_rows", out_rows, torch.float64, (B, views * K, ROW)), ("out_count", out_count, torch.int32, (B,)),
                                  ("out_support", out_support, torch.int32, (B, views * K))):
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != rows.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor %s on %s" % (name, dtype, shape, rows.device))
    with torch.cuda.device(rows.device):
        code = load().mono_fuse_dets_f64(rows.data_ptr(), count.data_ptr(), geom.data_ptr(), float(iou), MODES[mode], out_rows.data_ptr(),
                                         out_count.data_ptr(), out_support.data_ptr(), B, K, int(views),
                                         torch.cuda.current_stream().cuda_stream)
    if code:
        raise RuntimeError("mono_fuse_dets_f64 failed with code %d" % code)
    return out_rows, out_count, out_support
