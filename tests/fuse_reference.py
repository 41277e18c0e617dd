"""Helpers of test_fuse_cpu.py / test_fuse_gpu.py (no tests in here): an independent restatement of the fuse semantics of
include/monosowa_kitti.h (scalar Python on the candidates, the overlaps from oracle/rotate_iou_oracle.py in float64) and the
seeded generator of the kernel test's rows."""
import functools
import math

import numpy as np

from oracle import rotate_iou_oracle as R

MARGIN = 1e-3            # every same-class pair's float64 IoU lies further than this from the threshold: 5 x the 2e-4 that
                         # test_kitti_overlap.py pins for the float32 routine the kernel runs
BEV = [9, 11, 8, 7, 12]  # (x, z, l, w, ry)


def wrap(a):
    if a > math.pi:
        a -= 2 * math.pi
    if a < -math.pi:
        a += 2 * math.pi
    return a


def flip_row(row, g):
    """The map between a row of the frame and the row of the same object in the mirrored frame (u -> W - u, calibration
    unchanged); it is its own inverse up to rounding, so it serves as `mirror` in the generator and as `un-mirror` here."""
    W, cu, fu, tx = float(g[0]), float(g[4]), float(g[6]), float(g[8])
    out = [float(v) for v in row]
    out[2], out[4] = W - float(row[4]), W - float(row[2])
    out[1] = wrap(math.pi - float(row[1])) if not math.isnan(row[1]) else float("nan")
    out[9] = ((W - 2 * cu) * float(row[11])) / fu - float(row[9]) + 2 * tx
    out[12] = wrap(out[1] + math.atan2((out[2] + out[4]) / 2 - cu, fu)) if not math.isnan(out[1]) else float("nan")
    return out


def candidates(rows, count, geom, b, views):
    """Image b's candidates in the frame: (ids, float64 [n, 14])."""
    B, K = rows.shape[0] // views, rows.shape[1]
    ids, out = [], []
    for v in range(views):
        for j in range(int(count[v * B + b])):
            ids.append(v * K + j)
            out.append(flip_row(rows[v * B + b, j], geom[b]) if v else [float(x) for x in rows[v * B + b, j]])
    return ids, np.array(out, dtype=np.float64).reshape(-1, 14)


def same_class_ious(cands):
    """{(i, j), i < j: float64 oracle IoU of the float32 rectangles} over EVERY same-class pair of the candidates."""
    boxes = cands[:, BEV].astype(np.float32).astype(np.float64)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(cands)):
            for j in range(i + 1, len(cands)):
                if cands[i, 0] == cands[j, 0]:
                    # centres further apart than the two half-diagonals: disjoint, IoU exactly 0 (a NaN fails the test and is clipped)
                    apart = math.hypot(boxes[i, 0] - boxes[j, 0], boxes[i, 1] - boxes[j, 1]) > \
                        (math.hypot(boxes[i, 2], boxes[i, 3]) + math.hypot(boxes[j, 2], boxes[j, 3])) / 2
                    area = boxes[i, 2] * boxes[i, 3] + boxes[j, 2] * boxes[j, 3]
                    out[(i, j)] = 0.0 if apart and area > 0 else float(R.rotate_iou(boxes[i:i + 1], boxes[j:j + 1], -1)[0, 0])
    return out


def fuse(ids, cands, ious, K, g, iou, mode, views):
    """One image -> (seed candidate indices, rows [seeds, 14], support [seeds])."""
    n = len(ids)
    order = sorted(range(n), key=lambda i: (1, 0.0, ids[i]) if math.isnan(cands[i, 13]) else (0, -cands[i, 13], ids[i]))
    thr = np.float32(iou)
    clusters = []
    for i in order:
        for members in clusters:
            q = members[0]
            if cands[q, 0] == cands[i, 0] and np.float32(ious[(min(q, i), max(q, i))]) >= thr:
                members.append(i)
                break
        else:
            clusters.append([i])
    out = np.zeros((len(clusters), 14))
    for s, members in enumerate(clusters):
        m = cands[members]
        if mode == "seed":
            out[s] = m[0]
            continue
        w = m[:, 13]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[s, 2:12] = (w[:, None] * m[:, 2:12]).sum(0) / w.sum()
            out[s, 12] = math.atan2((w * np.sin(m[:, 12])).sum(), (w * np.cos(m[:, 12])).sum())
            a = out[s, 12] - math.atan2((out[s, 2] + out[s, 4]) / 2 - g[4], g[6])
            out[s, 1] = a if math.isnan(a) else wrap(a)
            out[s, 0] = m[0, 0]
            total = 0.0
            for v in range(views):
                mine = [w[k] for k, i in enumerate(members) if ids[i] // K == v]
                if mine:
                    total += max(x for x in mine if not math.isnan(x)) if any(not math.isnan(x) for x in mine) else float("nan")
            out[s, 13] = total / views
    return [c[0] for c in clusters], out, np.array([len(c) for c in clusters], dtype=np.int32)


def textbook_nms(rows, iou_of, iou):
    """Classic per-class NMS on rows sorted by score: indices kept."""
    order = sorted(range(len(rows)), key=lambda i: (-rows[i, 13], i))
    keep = []
    while order:
        i = order.pop(0)
        keep.append(i)
        order = [j for j in order if not (rows[j, 0] == rows[i, 0] and np.float32(iou_of(i, j)) >= np.float32(iou))]
    return keep


# ------------------------------------------------------------------------------------------------ the kernel test's rows
GEOM = np.array([[1242, 375, 1.0, 1.0, 609.5593, 172.854, 721.5377, 721.5377, 0.05986, -0.0003],
                 [1224, 370, 1.02, 0.98, 604.0814, 180.5066, 707.0493, 707.0493, 0.0646, 0.0016],
                 [1238, 374, 0.97, 1.01, 650.3, 175.2, 718.3351, 718.3351, -0.0465, 0.0007]], dtype=np.float64)


def _row(rng, g, cls, x, z, l, w, alpha, score):
    u = g[4] + g[6] * (x - g[8]) / z
    half = 0.5 * g[6] * max(l, w) / z
    x1, x2 = u - half, u + half
    ry = alpha if math.isnan(alpha) else wrap(alpha + math.atan2((x1 + x2) / 2 - g[4], g[6]))
    return [float(cls), alpha, x1, rng.uniform(120, 170), x2, rng.uniform(190, 300), rng.uniform(1.4, 1.7), w, l, x, rng.uniform(1.4, 1.8), z, ry,
            score]


def _jitter(rng, g, base, score):
    return _row(rng, g, base[0], base[9] + rng.normal(0, 0.35), base[11] + rng.normal(0, 0.35), base[8] * rng.uniform(0.95, 1.05),
                base[7] * rng.uniform(0.95, 1.05), wrap(base[1] + rng.normal(0, 0.04)), score)


def _draw(seed, K, views):
    """B = 3: image 0 full (count = K in every view), image 1 empty in every view, image 2 partly filled.  Per image a list of
    (view, cluster label, row in the FRAME); clusters of jittered near-duplicates spread over the views, an overlapping box of
    another class, two bit-identical rows, one NaN score, one NaN heading, one zero-width box."""
    rng = np.random.default_rng(seed)
    images = []
    for b, fill in ((0, K), (1, 0), (2, K - 2)):
        g, items, label = GEOM[b], [], 0
        room = {v: (fill if v == 0 else (fill if b == 0 else max(fill - 1, 0))) for v in range(views)}
        scores = iter(rng.permutation(np.linspace(0.05, 0.95, 4 * K * views + 16)).tolist())

        def put(v, lab, row):
            if room[v] > 0:
                room[v] -= 1
                items.append((v, lab, row))
                return True
            return False

        def centre():
            return _row(rng, g, rng.integers(0, 3), rng.uniform(-18, 18), rng.uniform(8, 55), rng.uniform(3.2, 4.6), rng.uniform(1.5, 2.0),
                        rng.uniform(-math.pi, math.pi), next(scores))

        if fill:
            first = centre()
            put(0, label, first)
            for k in range(2 if b == 0 else 1):
                put(k % views, label, _jitter(rng, g, first, next(scores)))
            other = list(first)                                            # the same box as another class: never suppressed by it
            other[0], other[13] = (first[0] + 1) % 3, next(scores)
            assert put(0, label + 1, other)
            label += 2
            if b == 0:
                twin = centre()
                assert put(0, label, twin)
                assert put(0, label, list(twin))                                  # bit-identical, score included: the lower id leads
                label += 1
                lone = centre()
                lone[9], lone[13] = lone[9] + 60.0, float("nan")           # NaN score, away from everything
                assert put(views - 1, label, lone)
                label += 1
            else:
                blind = _row(rng, g, 0, rng.uniform(-18, 18), rng.uniform(8, 55), 4.0, 1.8, float("nan"), next(scores))      # NaN ry
                assert put(0, label, blind)
                flat = _jitter(rng, g, first, next(scores))
                flat[7] = 0.0                                              # zero width, inside a cluster's box
                assert put(views - 1, label + 1, flat)
                label += 2
            while any(room.values()):
                base = centre()
                for k in range(int(rng.integers(1, 5))):
                    v = int(rng.integers(0, views))
                    put(v if room[v] else (1 - v) % views, label, base if k == 0 else _jitter(rng, g, base, next(scores)))
                label += 1
        images.append(items)
    return images


def _assemble(images, K, views):
    B = len(images)
    rows, count = np.zeros((views * B, K, 14)), np.zeros(views * B, dtype=np.int32)
    labels = [[] for _ in range(B)]
    for b, items in enumerate(images):
        for v in range(views):
            for view, lab, row in items:
                if view == v:
                    rows[v * B + b, count[v * B + b]] = flip_row(row, GEOM[b]) if v else row       # view 1 holds the MIRRORED row
                    count[v * B + b] += 1
                    labels[b].append(lab)                                  # in candidate (id) order
    return rows, count, labels


@functools.lru_cache(maxsize=None)
def kernel_case(K, views, iou, first_seed=0):
    """Rows for the kernel test, resampled until every same-class pair keeps MARGIN from the threshold and the generated clusters
    have pairs on both sides of it (at least 30 % above).  -> dict with rows, count,
    geom, per image: ids, cands, ious, labels; tries = how many seeds it took."""
    for tries in range(1, 200):
        rows, count, labels = _assemble(_draw(first_seed + tries - 1, K, views), K, views)
        per_image, ok = [], True
        for b in range(3):
            ids, cands = candidates(rows, count, GEOM, b, views)
            ious = same_class_ious(cands)
            n_c = [int((cands[:, 0] == c).sum()) for c in np.unique(cands[:, 0])] if len(cands) else []
            assert len(ious) == sum(n * (n - 1) // 2 for n in n_c), "a same-class pair was left out of the margin check"
            ok = ok and all(math.isnan(v) or abs(v - iou) > MARGIN for v in ious.values())
            per_image.append({"ids": ids, "cands": cands, "ious": ious, "labels": labels[b]})
        case = {"rows": rows, "count": count, "geom": GEOM.copy(), "images": per_image, "tries": tries, "K": K, "views": views, "iou": iou}
        above, below = in_cluster_split(case)
        if ok and above >= 0.3 * (above + below) and below > 0:          # a draw that does not exercise both sides is redrawn too
            return case
    raise AssertionError("no seed in 200 keeps every pair %g away from the threshold" % MARGIN)


TWIN_KINDS = ("ulp x", "ulp z", "ulp l", "ulp w", "ulp ry", "half turn", "collinear", "shorter")


@functools.lru_cache(maxsize=None)
def twin_case(iou=0.7, seed=0):
    """One view, K = 16, images 0 and 2 full, image 1 empty: per image eight same-class pairs 20 m and more from each other, the
    second of a pair being the first with (TWIN_KINDS) one float32 BEV number moved by one ulp, the heading turned by float32 pi,
    the centre moved 0.2 m along the length (collinear long sides, IoU (l - 0.2) / (l + 0.2)), the length x 0.9 (IoU 0.9).  The
    five BEV numbers of every row are float32 values, so the kernel's cast keeps them.  Every pair's exact IoU is above ``iou``
    by more than MARGIN: each must end as ONE cluster of two.  -> the dict of kernel_case."""
    rng = np.random.default_rng(seed)
    f32 = lambda v: float(np.float32(v))
    K, views, images = 16, 1, []
    for b in range(3):
        g, items = GEOM[b], []
        for k, kind in enumerate(TWIN_KINDS if b != 1 else ()):
            first = _row(rng, g, k % 3, f32(-30 + 20 * (k % 4) + rng.uniform(-2, 2)), f32(15 + 25 * (k // 4) + rng.uniform(-2, 2)),
                         f32(rng.uniform(3.2, 4.6)), f32(rng.uniform(1.5, 2.0)), rng.uniform(-3, 3), 0.9 - 0.02 * k)
            first[12] = f32(rng.uniform(-3, 3))
            twin = list(first)
            twin[13] = 0.5 - 0.02 * k
            if kind.startswith("ulp"):
                col = BEV[("x", "z", "l", "w", "ry").index(kind[4:])]
                twin[col] = float(np.nextafter(np.float32(first[col]), np.float32(np.inf if rng.integers(0, 2) else -np.inf)))
            elif kind == "half turn":
                twin[12] = float(np.float32(first[12]) + np.float32(np.pi))
            elif kind == "collinear":                                      # l is the rectangle's first side: its axis is (cos ry, -sin ry)
                twin[9], twin[11] = f32(first[9] + 0.2 * math.cos(first[12])), f32(first[11] - 0.2 * math.sin(first[12]))
            else:
                twin[8] = f32(first[8] * 0.9)
            assert all(float(np.float32(r[c])) == r[c] for r in (first, twin) for c in BEV) and twin != first
            items += [(0, k, first), (0, k, twin)]
        images.append(items)
    rows, count, labels = _assemble(images, K, views)
    per_image = []
    for b in range(3):
        ids, cands = candidates(rows, count, GEOM, b, views)
        ious = same_class_ious(cands)
        assert all(v - iou > MARGIN or v < iou - MARGIN for v in ious.values())
        assert all(ious[(2 * k, 2 * k + 1)] - iou > MARGIN for k in range(len(ids) // 2))
        per_image.append({"ids": ids, "cands": cands, "ious": ious, "labels": labels[b]})
    return {"rows": rows, "count": count, "geom": GEOM.copy(), "images": per_image, "tries": 1, "K": K, "views": views, "iou": iou}


def in_cluster_split(case):
    """(pairs of one generated cluster above the threshold, below it) over the case's same-class pairs."""
    above = below = 0
    for img in case["images"]:
        for (i, j), v in img["ious"].items():
            if img["labels"][i] == img["labels"][j] and not math.isnan(v):
                above, below = above + (v >= case["iou"]), below + (v < case["iou"])
    return above, below


def reference(case, mode):
    """-> per image (seed candidate indices, rows, support)."""
    return [fuse(img["ids"], img["cands"], img["ious"], case["K"], case["geom"][b], case["iou"], mode, case["views"])
            for b, img in enumerate(case["images"])]
